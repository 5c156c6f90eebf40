"""GPU parity of latent-space rendering (rgb_as_latents):
  * the four small kernels of csrc/asd_glue.hip (asd_latent_input_fwd / _bwd, asd_latent_decode_prep, asd_image_from_decoder) against
    torch on the device, outputs placed inside sentinel-filled buffers;
  * the VAE decoder network asd_vae_dec_* (HipVAEDecoder) against the goldens of the reference's own Decoder
    (tests/golden/diffusion_vae_decoder_*.npz), its resize front and its batch chunking;
  * both guidances in latent mode against the golden of the reference's __call__(rgb_as_latents=True)
    (tests/golden/diffusion_asd_glue_latent.npz), with the golden script's stand-in UNet and injected draws;
  * the multi-prompt system: one training step and a validation image whose first panel is decode_latents of the render.
Tolerances.  Resize forward: 2 ulp of fp32 (same arithmetic in the same order as ATen).  Resize adjoint: 1e-5 of the largest gradient
of the case (fp32 sums of at most a few hundred terms, summed in another order than ATen's atomics).  fp16 stores: half an ulp of
fp16 (2^-11 relative).  Decoder: the project's 1e-2 (relative L2 and max-normalised), the encoder's own full-width bound.  Guidance:
the bounds tests/test_gpu_asd_glue.py uses for the same quantities."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from golden_util import GOLDEN_DIR
from test_goldens_diffusion_cpu import fake_unet, rnd
from test_gpu_vae_hip import _rel

pytestmark = pytest.mark.gpu

SIZES = [((8, 8), (8, 8)), ((5, 7), (8, 8)), ((16, 12), (8, 8)), ((1, 9), (8, 8)), ((9, 1), (8, 8)), ((100, 72), (64, 64)), ((32, 48), (64, 64))]
SENTINEL = 77.0
PAD = 256          # elements in front of and behind an output inside its sentinel buffer (keeps the 16-byte alignment of vector stores)


@pytest.fixture(autouse=True)
def _stop_after_a_device_fault():
    """a kernel fault poisons the process: end the session instead of sending more work to the device"""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"device fault, nothing more is launched: {e}", returncode=3)


def _L():
    from scaledreamer_amd import _lib as L

    return L


def _golden(name):
    return np.load(os.path.join(GOLDEN_DIR, name + ".npz"))


class _Framed:
    """an output tensor inside a larger sentinel-filled buffer"""

    def __init__(self, shape, dtype):
        n = int(np.prod(shape))
        self.buf = torch.full((n + 2 * PAD,), SENTINEL, device="cuda", dtype=dtype)
        self.t = self.buf[PAD:PAD + n].view(shape)

    def untouched(self):
        return bool((self.buf[:PAD] == SENTINEL).all()) and bool((self.buf[-PAD:] == SENTINEL).all())


def _ulps(got, ref):
    spacing = torch.nextafter(ref.abs(), torch.full_like(ref, float("inf"))) - ref.abs()
    return float(((got - ref).abs() / spacing).max())


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("src,dst", SIZES)
def test_latent_input_kernels_match_interpolate_and_its_adjoint(src, dst, B):
    L = _L()
    l = L.lib()
    (h, w), (hl, wl) = src, dst
    g = torch.Generator().manual_seed(h * 1000 + w * 10 + B)
    render = torch.randn(B, h, w, 4, generator=g).cuda()
    noise = torch.randn(B, 4, hl, wl, generator=g).cuda()
    t = torch.randint(20, 980, (B,), generator=g).cuda()
    t_plus = (t + torch.randint(0, 19, (B,), generator=g).cuda()).clamp(1, 999)
    from scaledreamer_amd.guidance import ddpm_alphas_cumprod

    alphas = ddpm_alphas_cumprod().cuda()
    n_rep = 2
    lat, ux, ut = _Framed((B, 4, hl, wl), torch.float32), _Framed(((n_rep + 1) * B, hl, wl, 32), torch.float16), _Framed(((n_rep + 1) * B,), torch.float32)
    L.check(l.asd_latent_input_fwd(L.ptr(render), L.ptr(noise), L.ptr(t), L.ptr(t_plus), L.ptr(alphas), L.i32(B), L.i32(h), L.i32(w), L.i32(hl), L.i32(wl),
                                   L.i32(n_rep), L.ptr(lat.t), L.ptr(ux.t), L.ptr(ut.t), L.stream()))
    rr = render.clone().requires_grad_(True)
    ref = F.interpolate(rr.permute(0, 3, 1, 2), (hl, wl), mode="bilinear", align_corners=False)
    u = _ulps(lat.t, ref.detach())
    print(f"resize {src}->{dst} B={B}: {u:.2f} ulp")
    assert u <= 2.0
    if src == dst:
        assert torch.equal(lat.t, render.permute(0, 3, 1, 2))
    z = lat.t
    a0, a1 = alphas[t].view(-1, 1, 1, 1), alphas[t_plus].view(-1, 1, 1, 1)
    want = torch.cat([a0.sqrt() * z + (1 - a0).sqrt() * noise] * n_rep + [a1.sqrt() * z + (1 - a1).sqrt() * noise], 0)
    got = ux.t[..., :4].float().permute(0, 3, 1, 2)
    assert bool(((got - want).abs() <= want.abs() * 2.0 ** -11 + 1e-7).all())                      # one fp16 rounding of the fp32 value
    assert float(ux.t[..., 4:].abs().max()) == 0.0
    assert torch.equal(ut.t, torch.cat([t] * n_rep + [t_plus]).float())
    assert lat.untouched() and ux.untouched() and ut.untouched()
    # adjoint
    grad = torch.randn(B, 4, hl, wl, generator=g).cuda()
    up = torch.tensor([0.7], device="cuda")
    d = _Framed((B, h, w, 4), torch.float32)
    L.check(l.asd_latent_input_bwd(L.ptr(grad), L.ptr(up), L.i32(B), L.i32(h), L.i32(w), L.i32(hl), L.i32(wl), L.ptr(d.t), L.stream()))
    (want_d,) = torch.autograd.grad(ref, rr, grad * (0.7 / B))
    err = float((d.t - want_d).abs().max()) / float(want_d.abs().max())
    print(f"adjoint {src}->{dst} B={B}: {err:.2e} of the largest gradient")
    assert err <= 1e-5
    assert d.untouched()
    d2 = torch.empty(B, h, w, 4, device="cuda")
    L.check(l.asd_latent_input_bwd(L.ptr(grad), L.ptr(None), L.i32(B), L.i32(h), L.i32(w), L.i32(hl), L.i32(wl), L.ptr(d2), L.stream()))   # upstream NULL = 1
    torch.testing.assert_close(d2 * 0.7, d.t, rtol=1e-6, atol=0)


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("src,dst", SIZES)
def test_decode_prep_matches_resize_scale_and_post_quant_conv(src, dst, B):
    L = _L()
    (h, w), (hl, wl) = src, dst
    g = torch.Generator().manual_seed(h * 1000 + w * 10 + B + 5)
    lat = torch.randn(B, h, w, 4, generator=g).cuda()
    pq = torch.cat([torch.randn(16, generator=g) * 0.5, torch.randn(4, generator=g) * 0.1]).cuda()
    z = _Framed((B, hl, wl, 32), torch.float16)
    L.check(L.lib().asd_latent_decode_prep(L.ptr(lat), L.i32(B), L.i32(h), L.i32(w), L.i32(hl), L.i32(wl), L.f32(1 / 0.18215), L.ptr(pq), L.ptr(z.t), L.stream()))
    r = F.interpolate(lat.permute(0, 3, 1, 2), (hl, wl), mode="bilinear", align_corners=False) * (1 / 0.18215)
    want = F.conv2d(r.double(), pq[:16].view(4, 4, 1, 1).double(), pq[16:].double()).permute(0, 2, 3, 1)
    got = z.t[..., :4].double()
    # fp32 arithmetic (four products per output, each operand good to a few ulp), then one fp16 rounding
    mag = F.conv2d(r.abs().double(), pq[:16].view(4, 4, 1, 1).abs().double(), pq[16:].abs().double()).permute(0, 2, 3, 1)
    assert bool(((got - want).abs() <= want.abs() * 2.0 ** -11 + mag * 2e-6 + 1e-7).all())
    assert float(z.t[..., 4:].abs().max()) == 0.0 and z.untouched()


def test_image_from_decoder_is_exact():
    L = _L()
    n = 3 * 37 * 41
    g = torch.Generator().manual_seed(3)
    x = (torch.randn(n, 32, generator=g) * 1.5).half().cuda()
    x[0, :3] = torch.tensor([1.0, -1.0, 0.0]).half()
    x[1, :3] = torch.tensor([65504.0, -65504.0, 1.0009765625]).half()
    img, raw = _Framed((n, 3), torch.float32), _Framed((n, 3), torch.float32)
    L.check(L.lib().asd_image_from_decoder(L.ptr(x), n, L.ptr(img.t), L.ptr(raw.t), L.stream()))
    assert torch.equal(raw.t, x[:, :3].float()) and torch.equal(img.t, (x[:, :3].float() * 0.5 + 0.5).clamp(0, 1))
    assert img.untouched() and raw.untouched()
    only = torch.empty(n, 3, device="cuda")
    L.check(L.lib().asd_image_from_decoder(L.ptr(x), n, L.ptr(only), L.ptr(None), L.stream()))
    assert torch.equal(only, img.t)


@pytest.mark.parametrize("B,hw,C,silu", [(1, 64, 128, True), (5, 64, 128, False), (3, 100, 96, True), (2, 4096, 32, True), (2, 3000, 512, True), (1, 7, 2048, False)])
def test_ordered_groupnorm_matches_torch_and_is_reproducible_in_any_batch(B, hw, C, silu):
    """asd_groupnorm_ordered_f16: sizes with one and with many statistics blocks per image, rows that do not fill the last block, a
    channel count whose slots do not divide the block (96), the widest (2048).  Bound against fp32 torch: one fp16 rounding of the
    output plus fp32 statistics (1e-3 of the largest output)."""
    L = _L()
    g = torch.Generator().manual_seed(hw + C)
    x = (torch.randn(B, hw, C, generator=g) * 1.5 + 0.3).half().cuda()
    ga, be = (1 + 0.1 * torch.randn(C, generator=g)).half().cuda(), (0.05 * torch.randn(C, generator=g)).half().cuda()

    def run(xs):
        n = xs.shape[0]
        y, stats = _Framed((n, hw, C), torch.float16), _Framed((n * 64 + (512 + n) * 64,), torch.float32)
        L.check(L.lib().asd_groupnorm_ordered_f16(L.ptr(xs), L.i32(C), L.i32(n), L.i32(hw), L.ptr(ga), L.ptr(be), L.f32(1e-6), L.i32(int(silu)), L.ptr(y.t),
                                                  L.ptr(stats.t), L.stream()))
        assert y.untouched() and stats.untouched()
        return y.t
    y = run(x)
    ref = F.group_norm(x.float().permute(0, 2, 1), 32, ga.float(), be.float(), 1e-6)
    ref = (F.silu(ref) if silu else ref).permute(0, 2, 1)
    assert float((y.float() - ref).abs().max()) <= 1e-3 * float(ref.abs().max())
    assert torch.equal(run(x), y)
    for b in range(B):
        assert torch.equal(run(x[b:b + 1].contiguous()), y[b:b + 1])
    assert L.lib().asd_groupnorm_ordered_f16(L.ptr(x), L.i32(C), L.i32(600), L.i32(hw), L.ptr(ga), L.ptr(be), L.f32(1e-6), L.i32(0), L.ptr(y),
                                             L.ptr(y), L.stream()) != 0        # refused before any launch


def _decoder(cfg, seed, **kw):
    from scaledreamer_amd.diffusion import weights as W
    from scaledreamer_amd.diffusion.vae_hip import HipVAEDecoder

    params = W.gen_params(W.vae_decoder_layout(cfg)[0], seed)
    return HipVAEDecoder(params, cfg, "cuda", **kw), params


@pytest.fixture(scope="module")
def small():
    from scaledreamer_amd.diffusion import weights as W

    g = _golden("diffusion_vae_decoder_small")
    dec, params = _decoder(W.VAEConfig(ch=32), int(g["seed"]))
    return g, dec, params


def test_decoder_matches_reference_golden_small(small):
    """measured on an MI355X: see DESIGN.md (VAE decoder) for the figures of this test and of the fp16 library-op run"""
    g, dec, _ = small
    assert float(g["inside"]) >= 0.5 and float(((g["image"] > 0) & (g["image"] < 1)).mean()) >= 0.5     # the clamped comparison compares something
    lat = torch.from_numpy(g["latents"]).cuda().permute(0, 2, 3, 1).contiguous()
    img, raw = dec(lat, (8, 8), return_raw=True)
    assert tuple(img.shape) == (2, 64, 64, 3)
    e_raw, e_img = _rel(raw.permute(0, 3, 1, 2), torch.from_numpy(g["raw"])), _rel(img.permute(0, 3, 1, 2), torch.from_numpy(g["image"]))
    print(f"decoder small: raw l2 {e_raw[0]:.3e} max {e_raw[1]:.3e} | image l2 {e_img[0]:.3e} max {e_img[1]:.3e}")
    assert max(*e_raw, *e_img) < 1e-2
    assert torch.equal(img, (raw * 0.5 + 0.5).clamp(0, 1))


def test_decoder_resizes_to_the_latent_grid_first(small):
    """(5,7) -> 8x8 against prep-then-decode of the fixture path: the torch-resized latents handed over at 8x8, where the resize is the
    identity.  The decoder's input is the same bits on both ways (the resize matches ATen's roundings) and the decoder reproduces its
    bits, so the images are equal."""
    L = _L()
    _, dec, _ = small
    lat = (rnd("in.latents57", (2, 5, 7, 4), 21) * 0.18215).cuda()
    resized = F.interpolate(lat.permute(0, 3, 1, 2), (8, 8), mode="bilinear", align_corners=False).permute(0, 2, 3, 1).contiguous()
    z = [torch.empty(2, 8, 8, 32, device="cuda", dtype=torch.float16) for _ in range(2)]
    for src, dst in ((lat, z[0]), (resized, z[1])):
        L.check(L.lib().asd_latent_decode_prep(L.ptr(src), L.i32(2), L.i32(src.shape[1]), L.i32(src.shape[2]), L.i32(8), L.i32(8), L.f32(1 / 0.18215),
                                               L.ptr(dec.post_quant), L.ptr(dst), L.stream()))
    assert torch.equal(z[0], z[1])
    img, raw = dec(lat, (8, 8), return_raw=True)
    img2, raw2 = dec(resized, (8, 8), return_raw=True)
    e = _rel(raw, raw2)
    print(f"decoder (5,7)->(8,8): l2 {e[0]:.3e} max {e[1]:.3e}")
    assert torch.equal(raw, raw2) and torch.equal(img, img2)
    with pytest.raises(ValueError, match="channels last"):
        dec(lat.permute(0, 3, 1, 2), (8, 8))
    from scaledreamer_amd._lib import AsdError

    with pytest.raises(AsdError, match="VAE decoder"):
        dec(lat, (7, 8))


def test_decoder_batch_chunks_change_no_bit(small):
    """the decoder runs tiles that depend on a layer's width alone and ordered GroupNorm statistics, so an image's bits depend neither on
    the chunk nor on the call (with the shared asd_groupnorm_f16, whose statistics pass sums in arrival order, two identical calls
    differed by 1.8e-3)"""
    from scaledreamer_amd.diffusion import weights as W

    g, dec, params = small
    from scaledreamer_amd.diffusion.vae_hip import HipVAEDecoder

    lat = (rnd("in.latents5", (5, 8, 8, 4), 21) * 0.18215).cuda()
    whole = dec(lat, (8, 8), return_raw=True)
    assert dec.chunk_for(5, 8, 8) == 5
    by2 = HipVAEDecoder(params, W.VAEConfig(ch=32), "cuda", chunk=2)
    assert by2.chunk_for(5, 8, 8) == 2
    parts = by2(lat, (8, 8), return_raw=True)
    print("decoder chunks of 2 vs one call: rel", _rel(parts[1], whole[1]))
    assert torch.equal(whole[0], parts[0]) and torch.equal(whole[1], parts[1])
    again = dec(lat, (8, 8), return_raw=True)
    assert torch.equal(whole[0], again[0]) and torch.equal(whole[1], again[1])
    assert torch.equal(dec(lat[3:4], (8, 8)), whole[0][3:4])


def test_decoder_matches_reference_golden_full():
    """64x64 -> 512x512 at full width, B = 1: the only test at this size"""
    from scaledreamer_amd.diffusion import weights as W

    g = _golden("diffusion_vae_decoder_full_64")
    assert float(((g["image_sub"] > 0) & (g["image_sub"] < 1)).mean()) >= 0.5 and float(g["inside"]) >= 0.5
    dec, _ = _decoder(W.VAEConfig(), int(g["seed"]))
    assert dec.chunk_for(16, 64, 64) == 3                    # the 2 GiB rule at this size
    lat = torch.from_numpy(g["latents"]).cuda().permute(0, 2, 3, 1).contiguous()
    img, raw = dec(lat, (64, 64), return_raw=True)
    assert tuple(img.shape) == (1, 512, 512, 3)
    st = int(g["stride"])
    raw_c, img_c = raw.permute(0, 3, 1, 2), img.permute(0, 3, 1, 2)
    e_raw, e_img = _rel(raw_c[:, :, ::st, ::st], torch.from_numpy(g["raw_sub"])), _rel(img_c[:, :, ::st, ::st], torch.from_numpy(g["image_sub"]))
    print(f"decoder full: raw l2 {e_raw[0]:.3e} max {e_raw[1]:.3e} | image l2 {e_img[0]:.3e} max {e_img[1]:.3e}")
    assert max(*e_raw, *e_img) < 1e-2
    # every pixel takes part in these: per-channel mean (relative to the mean magnitude) and mean magnitude of the whole output
    mean_abs = torch.from_numpy(g["raw_mean_abs"])
    assert float(((raw_c.mean(dim=(0, 2, 3)).cpu() - torch.from_numpy(g["raw_mean"])).abs() / mean_abs).max()) < 1e-2
    assert float((raw_c.abs().mean(dim=(0, 2, 3)).cpu() / mean_abs - 1).abs().max()) < 1e-2


class _StandInBackend:
    """the golden script's cheap UNet behind the buffer protocol adaptors of DiffusionBackend; no encoder — latent mode must not ask for
    one — and a cheap decoder for the system test"""

    def __new__(cls, camera_dim=0, context_dim=1024):
        from scaledreamer_amd.guidance import DiffusionBackend

        class B(DiffusionBackend):
            def unet(self, x, t, ctx, camera=None, num_frames=1):
                self.calls = dict(x=x.clone(), t=t.clone(), nf=num_frames)
                return fake_unet(x, t, ctx, camera)

            def encode(self, imgs):
                raise AssertionError("latent mode reached the VAE encoder")

            def vae_forward(self, x):
                raise AssertionError("latent mode reached the VAE encoder")

            def decode(self, latents):
                up = F.interpolate(latents, scale_factor=8.0, mode="nearest")
                return torch.stack([up[:, 0] - up[:, 1], up[:, 2], 0.5 * up[:, 3] + 0.1], dim=1)
        b = B()
        b.camera_dim, b.context_dim, b.device = camera_dim, context_dim, "cuda"
        return b


def _inject(guid, g, k):
    def no_posterior(like):
        raise AssertionError("latent mode drew a posterior sample")
    guid.posterior_noise_fn = no_posterior
    guid.noise_fn = lambda like: torch.from_numpy(g[k + "_noise"]).cuda()
    guid.timestep_fn = lambda lo, hi, n, device: torch.from_numpy(g[k + "_t"]).cuda()
    guid.rand_fn = lambda shape, device: torch.from_numpy(g[k + "_rand"]).cuda()


def test_sd_guidance_latent_mode_matches_reference_call_golden():
    from scaledreamer_amd.guidance import PromptUtils, SDTimestepShiftedScoreDistillationGuidance as G

    g = _golden("diffusion_asd_glue_latent")
    seed, B = int(g["sd_seed"]), 2
    be = _StandInBackend()
    guid = G({"guidance_scale": 7.5, "plus_ratio": 0.1, "plus_random": True, "guidance_perp_neg": -0.5, "min_step_percent": 0.5,
              "max_step_percent": 0.98}, backend=be)
    _inject(guid, g, "sd")
    pu = PromptUtils(rnd("prompt.vd", (4, 77, 1024), seed).cuda(), rnd("prompt.uncond", (1, 77, 1024), seed).expand(4, -1, -1).contiguous().cuda(),
                     front_threshold=30.0, back_threshold=30.0)
    render = rnd("latent.render", (B, 48, 40, 4), seed).cuda().requires_grad_(True)
    el, az, di = (torch.from_numpy(g[k]).cuda() for k in ("sd_elevation", "sd_azimuth", "sd_camera_distances"))
    out = guid(render, pu, el, az, di, rgb_as_latents=True)
    assert (out["min_step"], out["max_step"]) == (int(g["sd_min_step"]), int(g["sd_max_step"]))
    np.testing.assert_array_equal(be.calls["t"].cpu().numpy(), g["sd_unet_in_t"])
    x = be.calls["x"].cpu().numpy()
    assert x.shape[0] == int(g["sd_unet_batch"])
    for first in (x[r * B:(r + 1) * B] for r in range(4)):
        assert float(np.abs(first - g["sd_unet_in_first"]).max()) < 2e-3 * float(np.abs(g["sd_unet_in_first"]).max())
    assert float(np.abs(x[-B:] - g["sd_unet_in_last"]).max()) < 2e-3 * float(np.abs(g["sd_unet_in_last"]).max())
    rel_loss, rel_norm = out["loss_asd"].item() / float(g["sd_loss_asd"]) - 1, out["grad_norm"].item() / float(g["sd_grad_norm"]) - 1
    print(f"sd latent: loss {rel_loss:+.2e} grad_norm {rel_norm:+.2e}")
    assert abs(rel_loss) < 2e-3 and abs(rel_norm) < 2e-3
    (out["loss_asd"] * 1.0).backward()
    scale = float(np.abs(g["sd_grad_render"]).max())
    err = np.abs(render.grad.cpu().numpy() - g["sd_grad_render"]).max() / scale
    print(f"sd latent: gradient {err:.2e} of the largest")
    assert err < 3e-3
    with pytest.raises(ValueError, match="3 channels"):
        guid(render.detach()[..., :3], pu, el, az, di, rgb_as_latents=True)


def test_mvdream_guidance_latent_mode_matches_reference_call_golden():
    from scaledreamer_amd.guidance import MVDreamTimestepShiftedScoreDistillationGuidance as G, PromptUtils

    g = _golden("diffusion_asd_glue_latent")
    seed, B = int(g["mv_seed"]), 4
    be = _StandInBackend(camera_dim=16)
    guid = G({"guidance_scale": 7.5, "plus_ratio": 0.1, "plus_random": True, "n_view": 4}, backend=be)
    _inject(guid, g, "mv")
    emb, unc = rnd("mv.prompt", (1, 77, 1024), seed), rnd("mv.uncond", (1, 77, 1024), seed)
    pu = PromptUtils(emb.expand(4, -1, -1).cuda(), unc.expand(4, -1, -1).cuda(), emb.cuda(), unc.cuda(), use_perp_neg=False)
    render = rnd("latent.render", (B, 48, 40, 4), seed).cuda().requires_grad_(True)
    el, az, di = (torch.from_numpy(g[k]).cuda() for k in ("mv_elevation", "mv_azimuth", "mv_camera_distances"))
    out = guid(render, pu, el, az, di, torch.from_numpy(g["mv_c2w"]).cuda(), rgb_as_latents=True)
    assert be.calls["nf"] == int(g["mv_num_frames"]) == 4
    np.testing.assert_array_equal(be.calls["t"].cpu().numpy(), g["mv_unet_in_t"].astype(np.float32))
    want = g["mv_unet_in_x"]
    assert float(np.abs(be.calls["x"].cpu().numpy() - want).max()) < 2e-3 * float(np.abs(want).max())
    rel_loss, rel_norm = out["loss_asd"].item() / float(g["mv_loss_asd"]) - 1, out["grad_norm"].item() / float(g["mv_grad_norm"]) - 1
    print(f"mv latent: loss {rel_loss:+.2e} grad_norm {rel_norm:+.2e}")
    assert abs(rel_loss) < 2e-3 and abs(rel_norm) < 2e-3
    (out["loss_asd"] * 1.0).backward()
    scale = float(np.abs(g["mv_grad_render"]).max())
    got = render.grad.cpu().numpy() / scale
    print(f"mv latent: gradient max {np.abs(got - g['mv_grad_render'] / scale).max():.2e} rms {np.sqrt(np.mean((got - g['mv_grad_render'] / scale) ** 2)):.2e}")
    np.testing.assert_allclose(got, g["mv_grad_render"] / scale, rtol=0, atol=1.5e-2)
    assert float(np.sqrt(np.mean((got - g["mv_grad_render"] / scale) ** 2))) < 2e-3


def test_sd_decode_latents_is_the_backends_decoder_behind_the_resize():
    from scaledreamer_amd.guidance import SDTimestepShiftedScoreDistillationGuidance as G

    be = _StandInBackend()
    guid = G({}, backend=be)
    lat = (rnd("dl.latents", (2, 4, 12, 10), 3) * 0.18215).cuda().half()
    img = guid.decode_latents(lat, 8, 6)
    assert tuple(img.shape) == (2, 3, 64, 48) and img.dtype == torch.float16 and float(img.min()) >= 0 and float(img.max()) <= 1
    z = F.interpolate(lat.float(), (8, 6), mode="bilinear", align_corners=False) * (1 / 0.18215)
    torch.testing.assert_close(img.float(), (be.decode(z) * 0.5 + 0.5).clamp(0, 1), rtol=0, atol=1e-3)
    assert tuple(guid.decode_latents(lat.float()[:1]).shape) == (1, 3, 512, 512)          # the reference's defaults: 64 x 64


def test_hip_backend_builds_its_decoder_on_first_use_and_decodes_the_golden():
    """the product backend behind the SD guidance's decode_latents: no decoder until the first call, its weights from the callable it
    was given, then the small fixture within the decoder's bound through both seams"""
    from scaledreamer_amd.diffusion import weights as W
    from scaledreamer_amd.diffusion.engine import HipBackend
    from scaledreamer_amd.guidance import SDTimestepShiftedScoreDistillationGuidance as G

    g = _golden("diffusion_vae_decoder_small")
    cfg = W.VAEConfig(ch=32)
    asked = []

    def load():
        asked.append(1)
        return W.gen_params(W.vae_decoder_layout(cfg)[0], int(g["seed"]))

    be = HipBackend("cuda", unet_cfg=W.UNetConfig(model_channels=64, context_dim=96, channel_mult=(1, 2), attention_resolutions=(1,)), vae_cfg=cfg,
                    seed=3, use_graph=False, decoder_params=load)
    assert be.hip_vae_dec is None and not asked
    guid = G({}, backend=be)
    lat = torch.from_numpy(g["latents"]).cuda()
    img = guid.decode_latents(lat, 8, 8)
    assert asked == [1] and be.hip_vae_dec is not None and tuple(img.shape) == (2, 3, 64, 64) and img.dtype == lat.dtype
    e = _rel(img, torch.from_numpy(g["image"]))
    raw = be.decode(lat * (1 / cfg.scale_factor))
    e2 = _rel(raw, torch.from_numpy(g["raw"]))
    print(f"backend decode_latents: image l2 {e[0]:.3e} max {e[1]:.3e} | decode: raw l2 {e2[0]:.3e} max {e2[1]:.3e}")
    assert max(*e, *e2) < 1e-2 and asked == [1]


class _LatentRenderer(torch.nn.Module):
    """stands in for the renderer of a latent-space run: a 4-channel comp_rgb that depends on one parameter"""

    def __init__(self):
        super().__init__()
        self.gain = torch.nn.Parameter(torch.tensor(1.0))

    def forward(self, rays_o, **kw):
        B, H, W, _ = rays_o.shape
        yy, xx = torch.meshgrid(torch.linspace(-1, 1, H, device=rays_o.device), torch.linspace(-1, 1, W, device=rays_o.device), indexing="ij")
        base = torch.stack([yy, xx, yy * xx, 0.5 - xx * xx], dim=-1)[None].expand(B, -1, -1, -1) * 0.3
        opacity = (0.5 + 0.4 * yy)[None, :, :, None].expand(B, -1, -1, -1).contiguous()
        return {"comp_rgb": base * self.gain, "opacity": opacity, "depth": (1.0 + xx)[None, :, :, None].expand(B, -1, -1, -1).contiguous()}


def test_multi_prompt_system_trains_and_validates_in_latent_space(tmp_path):
    import random

    from test_gpu_views import PROMPTS, _png

    from scaledreamer_amd import presets
    from scaledreamer_amd.multiprompt import SyntheticMultiPromptProcessor
    from scaledreamer_amd.registry import find
    import scaledreamer_amd.plugins  # noqa: F401

    torch.manual_seed(0)
    random.seed(0)
    dev = torch.device("cuda", 0)
    cfg = presets.asd_sd_hyper_ingp(PROMPTS)
    cfg["system"].update(rgb_as_latents=True, validation_via_video=False)
    cfg["system"]["guidance"] = {"guidance_scale": 7.5}
    for k in list(cfg["system"]["loss"]):
        if k != "lambda_asd":
            cfg["system"]["loss"][k] = 0.0
    cfg["data"].update(eval_height=512, eval_width=512, n_val_views=1, n_test_views=1, prompt_library={"train": PROMPTS, "val": PROMPTS[:1], "test": PROMPTS[:1]})
    proc = SyntheticMultiPromptProcessor(PROMPTS, seed=2, device=dev, ctx_dim=128, global_dim=1024)
    be = _StandInBackend(context_dim=128)
    system = find(cfg["system_type"])(cfg["system"], guidance_backend=be, prompt_processor=proc)
    system.renderer = _LatentRenderer().to(dev)
    system.train()
    system.on_train_batch_start()
    dm = find(cfg["data_type"])(cfg["data"], rank=0, n_ranks=1)
    batch = system._batch_to_device(dm.collate())
    loss = system.training_step(batch)["loss"]
    assert bool(torch.isfinite(loss))
    loss.backward()
    gain_grad = system.renderer.gain.grad
    assert gain_grad is not None and bool(torch.isfinite(gain_grad)) and float(gain_grad.abs()) > 0
    # validation: the first panel is decode_latents of the render, the render itself is no panel
    paths = system.validate(dm.val_dataset(), str(tmp_path))
    assert len(paths) == 1 and system.training
    png = _png(paths[0])
    assert png.shape == (512, 3 * 512, 3)                       # decoded_rgb | opacity | depth
    system.eval()
    with torch.no_grad():
        val = system._batch_to_device(next(iter(dm.val_dataset())))
        render = system.renderer(**val)["comp_rgb"]
        assert render.shape[-1] == 4
        want = system.guidance.decode_latents(render.permute(0, 3, 1, 2)).permute(0, 2, 3, 1)[0]
        out = system(val)
        assert torch.equal(out["decoded_rgb"][0], want)
    system.train()
    want_u8 = (want.clamp(0, 1) * 255.0).cpu().numpy()
    assert float(np.abs(png[:, :512].astype(np.float64) - want_u8).max()) <= 1.0
    # training mode never decodes
    assert "decoded_rgb" not in system(batch)
