"""Golden vectors for latent-space rendering (rgb_as_latents), produced by the REFERENCE's own classes.

  python tests/golden/make_goldens_latent.py     # writes tests/golden/diffusion_vae_decoder_*.npz, diffusion_asd_glue_latent.npz  (CPU)

Runs, imported in place from the reference tree under ref_harness.py:
  * extern.mvdream ... model.Decoder (+ a 1x1 post_quant_conv as in autoencoder.py:33,87-90) behind the arithmetic of
    decode_latents (stable_diffusion_asd_guidance.py:180-194): / scaling_factor, decode, clamp(0.5 x + 0.5, 0, 1)
  * SDTimestepShiftedScoreDistillationGuidance.__call__ and MVDreamTimestepShiftedScoreDistillationGuidance.__call__ with
    rgb_as_latents=True, driven with the stand-in UNet of make_goldens_diffusion.py (no VAE is reached in this mode)
Weights follow scaledreamer_amd.diffusion.weights.gen_params over vae_decoder_layout: load_state_dict(strict=True) proves that the
layout's names and shapes are the reference Decoder's; the name list is written into the fixtures for the CPU tests.
"""
from __future__ import annotations

import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_harness as H  # noqa: E402

H.install()

from scaledreamer_amd.diffusion import weights as W  # noqa: E402

from extern.mvdream.ldm.modules.diffusionmodules.model import Decoder  # noqa: E402


def rnd(name, shape, seed=0):
    """seeded input tensors share the name-keyed rule of the weights (plain N(0,1))."""
    import zlib
    g = torch.Generator().manual_seed((seed * 1_000_003 + zlib.crc32(name.encode())) & 0x7FFFFFFF)
    return torch.randn(shape, generator=g)


def reference_decoder(cfg: W.VAEConfig, seed: int, resolution: int):
    shapes, _ = W.vae_decoder_layout(cfg)
    dec = Decoder(ch=cfg.ch, out_ch=cfg.in_channels, ch_mult=cfg.ch_mult, num_res_blocks=cfg.num_res_blocks, attn_resolutions=[], dropout=0.0,
                  in_channels=cfg.in_channels, resolution=resolution, z_channels=cfg.z_channels).eval()
    post = torch.nn.Conv2d(cfg.embed_dim, cfg.z_channels, 1)
    p = W.gen_params(shapes, seed)
    dec.load_state_dict({k[len("decoder."):]: v for k, v in p.items() if k.startswith("decoder.")}, strict=True)
    post.load_state_dict({"weight": p["post_quant_conv.weight"], "bias": p["post_quant_conv.bias"]}, strict=True)
    names = ["decoder." + k for k in dec.state_dict()] + ["post_quant_conv." + k for k in post.state_dict()]
    name_shapes = [tuple(v.shape) for v in dec.state_dict().values()] + [tuple(v.shape) for v in post.state_dict().values()]
    assert sorted(names) == sorted(shapes) and all(tuple(shapes[n]) == s for n, s in zip(names, name_shapes))
    return dec, post, names, name_shapes


def make_decoder_golden(name, cfg: W.VAEConfig, batch, hl, seed, latent_scale, stride):
    """decode_latents(latents) with latents already on the latent grid (the resize is then the identity)"""
    dec, post, names, name_shapes = reference_decoder(cfg, seed, hl * 2 ** (len(cfg.ch_mult) - 1))
    latents = rnd("in.latents", (batch, cfg.z_channels, hl, hl), seed) * latent_scale
    with torch.no_grad():
        z = F.interpolate(latents, (hl, hl), mode="bilinear", align_corners=False)
        z = 1 / cfg.scale_factor * z
        raw = dec(post(z))
        image = (raw * 0.5 + 0.5).clamp(0, 1)
    inside = float(((image > 0) & (image < 1)).float().mean())
    # with random weights the output could sit outside [0,1] altogether, and the clamped comparison would compare constants
    assert inside >= 0.5, f"{name}: only {inside:.3f} of the pixels lie strictly inside (0,1); pick another seed / latent scale"
    save = dict(seed=seed, batch=batch, hl=hl, stride=stride, latent_scale=latent_scale, latents=latents.numpy(), inside=inside,
                names=np.array(names), name_shapes=np.array([",".join(map(str, s)) for s in name_shapes]),
                cfg=np.array([cfg.ch, cfg.num_res_blocks, cfg.z_channels, cfg.embed_dim]), ch_mult=np.array(cfg.ch_mult))
    if stride == 1:
        save.update(raw=raw.numpy(), image=image.numpy())
    else:
        save.update(raw_sub=raw[:, :, ::stride, ::stride].contiguous().numpy(), image_sub=image[:, :, ::stride, ::stride].contiguous().numpy(),
                    raw_mean=raw.mean(dim=(0, 2, 3)).numpy(), raw_mean_abs=raw.abs().mean(dim=(0, 2, 3)).numpy())
    np.savez_compressed(os.path.join(HERE, name + ".npz"), **save)
    print(f"{name}: params={W.count_params(W.vae_decoder_layout(cfg)[0])} raw mean|.|={raw.abs().mean():.4f} std={raw.std():.4f} inside(0,1)={inside:.3f}")


def _record_draws(seed, call):
    """run `call` with torch's random draws recorded, in call order"""
    rec = {"order": []}
    real = dict(randn_like=torch.randn_like, randint=torch.randint, rand=torch.rand)

    def wrap(name):
        def f(*a, **k):
            out = real[name](*a, **k)
            rec[name] = out.clone()
            rec["order"].append(name)
            return out
        return f
    torch.manual_seed(seed)
    torch.randn_like, torch.randint, torch.rand = wrap("randn_like"), wrap("randint"), wrap("rand")
    try:
        out = call()
    finally:
        torch.randn_like, torch.randint, torch.rand = real["randn_like"], real["randint"], real["rand"]
    return out, rec


def sd_latent_case(seed=11):
    dummy = type("Dummy", (), {})
    H._mod("diffusers", DDPMScheduler=dummy, DPMSolverMultistepScheduler=dummy, StableDiffusionPipeline=dummy, UNet2DConditionModel=dummy)
    H._mod("diffusers.utils")
    H._mod("diffusers.utils.import_utils", is_xformers_available=lambda: False)
    from threestudio.models.guidance.stable_diffusion_asd_guidance import SDTimestepShiftedScoreDistillationGuidance as G
    from threestudio.models.prompt_processors.base import DirectionConfig, PromptProcessorOutput, shift_azimuth_deg

    B = 2
    guid = object.__new__(G)
    guid.cfg = G.Config(guidance_scale=7.5, plus_ratio=0.1, plus_random=True, guidance_perp_neg=-0.5, min_step_percent=0.5, max_step_percent=0.98)
    guid.device = torch.device("cpu")
    guid.weights_dtype = torch.float32
    guid.num_train_timesteps = 1000
    guid.set_min_max_steps(0.5, 0.98)
    ac = torch.from_numpy(np.load(os.path.join(HERE, "diffusion_schedule.npz"))["alphas_cumprod"]).float()
    guid.alphas = ac
    guid.grad_clip_val = None
    guid.use_perp_neg = True

    class Sched:  # DDPMScheduler.add_noise (diffusers, un-vendored): x_t = sqrt(abar) x + sqrt(1-abar) eps
        def add_noise(self, x, noise, t):
            a = ac[t].view(-1, 1, 1, 1)
            return a.sqrt() * x + (1 - a).sqrt() * noise
    guid.scheduler = Sched()
    calls = {}

    def fake_unet(latents, t, encoder_hidden_states=None):
        calls.update(latents=latents.clone(), t=t.clone(), ctx=encoder_hidden_states.clone())
        s = encoder_hidden_states.mean(dim=(1, 2)).view(-1, 1, 1, 1)
        out = torch.tanh(0.7 * latents + 3.0 * s) * (1.0 + t.view(-1, 1, 1, 1) / 1000.0) + 0.1 * latents.flip(-1)
        return types.SimpleNamespace(sample=out)
    guid.unet = fake_unet

    class NoVAE:      # latent mode must not reach the VAE
        config = types.SimpleNamespace(scaling_factor=0.18215)

        def encode(self, imgs):
            raise AssertionError("rgb_as_latents=True reached vae.encode")
    guid.vae = NoVAE()

    emb_vd = rnd("prompt.vd", (4, 77, 1024), seed)
    unc_vd = rnd("prompt.uncond", (1, 77, 1024), seed).expand(4, -1, -1).contiguous()
    thr = 30.0
    directions = [
        DirectionConfig("side", lambda s: s, lambda s: s, lambda ele, azi, dis: torch.ones_like(ele, dtype=torch.bool)),
        DirectionConfig("front", lambda s: s, lambda s: s, lambda ele, azi, dis: (shift_azimuth_deg(azi) > -thr) & (shift_azimuth_deg(azi) < thr)),
        DirectionConfig("back", lambda s: s, lambda s: s, lambda ele, azi, dis: (shift_azimuth_deg(azi) > 180 - thr) | (shift_azimuth_deg(azi) < -180 + thr)),
        DirectionConfig("overhead", lambda s: s, lambda s: s, lambda ele, azi, dis: ele > 60.0),
    ]
    pu = PromptProcessorOutput(text_embeddings=emb_vd[0], uncond_text_embeddings=unc_vd[0], text_embeddings_vd=emb_vd, uncond_text_embeddings_vd=unc_vd,
                               directions=directions, direction2idx={d.name: i for i, d in enumerate(directions)}, use_perp_neg=True,
                               perp_neg_f_sb=(1, 0.5, -0.606), perp_neg_f_fsb=(1, 0.5, +0.967), perp_neg_f_fs=(4, 0.5, -2.426),
                               perp_neg_f_sf=(4, 0.5, -2.426), prompt="", prompts_vd=[""] * 4)
    elevation, azimuth, distances = torch.tensor([10.0, 25.0]), torch.tensor([12.0, -100.0]), torch.tensor([1.2, 1.1])
    render = rnd("latent.render", (B, 48, 40, 4), seed).requires_grad_(True)
    out, rec = _record_draws(seed, lambda: guid(render, pu, elevation, azimuth, distances, rgb_as_latents=True))
    out["loss_asd"].backward()
    latents = F.interpolate(render.detach().permute(0, 3, 1, 2), (64, 64), mode="bilinear", align_corners=False)
    assert rec["order"].count("randn_like") == 1, rec["order"]       # only `noise` is drawn: no posterior sample in this mode
    x_in = calls["latents"]       # [x_t] * 4 (text | uncond | 2 negatives per sample), then x_{t+}: the file keeps one copy of each
    assert x_in.shape[0] == 5 * B and all(torch.equal(x_in[:B], x_in[r * B:(r + 1) * B]) for r in range(4))
    return dict(sd_seed=seed, sd_elevation=elevation.numpy(), sd_azimuth=azimuth.numpy(), sd_camera_distances=distances.numpy(),
                sd_noise=rec["randn_like"].numpy(), sd_t=rec["randint"].numpy(), sd_rand=rec["rand"].numpy(), sd_min_step=guid.min_step,
                sd_max_step=guid.max_step, sd_latents=latents.numpy(), sd_unet_in_t=calls["t"].numpy(), sd_t_plus=calls["t"][-B:].numpy(),
                sd_unet_in_first=x_in[:B].numpy(), sd_unet_in_last=x_in[-B:].numpy(), sd_unet_batch=x_in.shape[0], sd_loss_asd=np.float64(out["loss_asd"].item()),
                sd_grad_norm=np.float64(out["grad_norm"].item()), sd_grad_render=render.grad.numpy(), sd_draw_order=np.array(rec["order"]))


def mv_latent_case(seed=12):
    H._mod("extern.mvdream.model_zoo", build_model=None)
    from threestudio.models.guidance.mvdream_asd_guidance import MVDreamTimestepShiftedScoreDistillationGuidance as G
    from threestudio.models.prompt_processors.base import DirectionConfig, PromptProcessorOutput

    B = 4
    guid = object.__new__(G)
    guid.cfg = G.Config(guidance_scale=7.5, plus_ratio=0.1, plus_random=True, n_view=4)
    guid.device = torch.device("cpu")
    guid.num_train_timesteps = 1000
    guid.min_step, guid.max_step = 20, 980
    guid.grad_clip_val = None
    ac = torch.from_numpy(np.load(os.path.join(HERE, "diffusion_schedule.npz"))["alphas_cumprod"]).float()
    guid.alphas = ac
    calls = {}

    class Model:
        alphas_cumprod = ac

        def q_sample(self, x, t, noise=None):
            a = ac[t].view(-1, 1, 1, 1)
            return a.sqrt() * x + (1 - a).sqrt() * noise

        def apply_model(self, x, t, cond):
            calls.update(x=x.clone(), t=t.clone(), ctx=cond["context"].clone(), camera=cond["camera"].clone(), nf=cond["num_frames"])
            s = cond["context"].mean(dim=(1, 2)).view(-1, 1, 1, 1) + cond["camera"].mean(dim=1).view(-1, 1, 1, 1)
            return torch.tanh(0.7 * x + 3.0 * s) * (1.0 + t.view(-1, 1, 1, 1) / 1000.0) + 0.1 * x.flip(-1)

        def encode_first_stage(self, imgs):
            raise AssertionError("rgb_as_latents=True reached encode_first_stage")
    guid.model = Model()
    emb, unc = rnd("mv.prompt", (1, 77, 1024), seed), rnd("mv.uncond", (1, 77, 1024), seed)
    side = DirectionConfig("side", lambda s: s, lambda s: s, lambda ele, azi, dis: torch.ones_like(ele, dtype=torch.bool))
    pu = PromptProcessorOutput(text_embeddings=emb, uncond_text_embeddings=unc, text_embeddings_vd=emb.expand(4, -1, -1),
                               uncond_text_embeddings_vd=unc.expand(4, -1, -1), directions=[side], direction2idx={"side": 0}, use_perp_neg=False,
                               perp_neg_f_sb=(1, 0.5, -0.606), perp_neg_f_fsb=(1, 0.5, 0.967), perp_neg_f_fs=(4, 0.5, -2.426),
                               perp_neg_f_sf=(4, 0.5, -2.426), prompt="", prompts_vd=[""] * 4)
    elevation, azimuth, distances = torch.full((4,), 10.0), torch.tensor([12.0, 102.0, -168.0, -78.0]), torch.full((4,), 1.2)
    c2w = torch.eye(4).repeat(4, 1, 1)
    c2w[:, :3, :3] = torch.linalg.qr(rnd("mv.rot", (4, 3, 3), seed))[0]
    c2w[:, :3, 3] = rnd("mv.pos", (4, 3), seed) * 1.3
    render = rnd("latent.render", (B, 48, 40, 4), seed).requires_grad_(True)
    out, rec = _record_draws(seed, lambda: guid(render, pu, elevation, azimuth, distances, c2w.clone(), rgb_as_latents=True))
    out["loss_asd"].backward()
    latents = F.interpolate(render.detach().permute(0, 3, 1, 2), (32, 32), mode="bilinear", align_corners=False)
    assert rec["order"].count("randn_like") == 1, rec["order"]
    return dict(mv_seed=seed, mv_elevation=elevation.numpy(), mv_azimuth=azimuth.numpy(), mv_camera_distances=distances.numpy(), mv_c2w=c2w.numpy(),
                mv_noise=rec["randn_like"].numpy(), mv_t=rec["randint"].numpy(), mv_rand=rec["rand"].numpy(), mv_latents=latents.numpy(),
                mv_unet_in_t=calls["t"].numpy(), mv_t_plus=calls["t"][-B:].numpy(), mv_unet_in_x=calls["x"].numpy(),
                mv_unet_in_camera=calls["camera"].numpy(), mv_num_frames=calls["nf"], mv_loss_asd=np.float64(out["loss_asd"].item()),
                mv_grad_norm=np.float64(out["grad_norm"].item()), mv_grad_render=render.grad.numpy(), mv_draw_order=np.array(rec["order"]))


def make_latent_glue_golden():
    save = {**sd_latent_case(), **mv_latent_case()}
    np.savez_compressed(os.path.join(HERE, "diffusion_asd_glue_latent.npz"), **save)
    print(f"latent glue: sd loss={float(save['sd_loss_asd']):.5f} grad_norm={float(save['sd_grad_norm']):.5f} t={save['sd_t'].tolist()} "
          f"t+={save['sd_t_plus'].tolist()} draws={save['sd_draw_order'].tolist()} | mv loss={float(save['mv_loss_asd']):.5f} "
          f"t={save['mv_t'].tolist()} draws={save['mv_draw_order'].tolist()}")


if __name__ == "__main__":
    torch.set_num_threads(8)
    make_latent_glue_golden()
    if "--glue-only" in sys.argv:
        sys.exit(0)
    # seed and latent scale: chosen so that at least half of the image lies strictly inside (0,1) (asserted above)
    make_decoder_golden("diffusion_vae_decoder_small", W.VAEConfig(ch=32), batch=2, hl=8, seed=21, latent_scale=0.18215, stride=1)
    make_decoder_golden("diffusion_vae_decoder_full_64", W.VAEConfig(), batch=1, hl=64, seed=22, latent_scale=0.18215, stride=3)
