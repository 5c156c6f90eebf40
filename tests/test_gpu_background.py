"""`textured-background` and `solid-color-background` on the HIP entries (asd_bg_texture_fwd / _bwd, asd_bg_solid_fwd / _bwd).

The reference of every comparison is the float64 restatement of tests/background_util.py evaluated on the same fp32 inputs (the restatement
itself is held against the reference's goldens by tests/test_background_cpu.py).  Tolerances (background_util.forward_tolerance /
backward_unit):
  forward   8 * 2^-23 * max(H, W) * D * A' + 2^-22 per ray (fp32 rounding of the sample point; D = largest adjacent-texel difference)
  backward  8 units of 2^-23 * (max(H, W) + n_t) * G_t per texel and channel; texels no ray reaches are exactly +0.0f
  solid     R * 2^-24 * sum |terms| per output (a plain sum of R terms); the forward is exact
Every case prints the largest ratio it reaches."""
import ctypes as C

import pytest
import torch

import background_util as U

pytestmark = pytest.mark.gpu

# (C, H, W, n): the default | non-square and odd, C = 4 (a u/v or H/W swap) | every index clamped, C = 1 | n no multiple of a wave or a
# block | 122,880 B: just under the LDS budget of 128 KiB | 196,608 B: the large-texture (global-atomic) path | empty call
SHAPES = [(3, 64, 64, 4096), (4, 5, 7, 1000), (1, 1, 1, 64), (3, 2, 3, 257), (4, 96, 80, 3000), (3, 128, 128, 20000), (3, 64, 64, 0)]
CONTENDED = (3, 64, 64, 16384)          # one camera's solid angle: about 2.5 k rays on one texel, many workgroups on few texels
ACTS = ("sigmoid", "none")


def _act_id(name):
    from scaledreamer_amd import _lib

    return {"sigmoid": _lib.ASD_BG_ACT_SIGMOID, "none": _lib.ASD_BG_ACT_NONE}[name]


_CASES = {}


def _case(shape, contended=False):
    """inputs and the float64 reference of one shape, computed once and shared by the activations"""
    key = (shape, contended)
    if key not in _CASES:
        Cc, H, W, n = shape
        g = torch.Generator().manual_seed(1000 + 7 * Cc + 3 * H + W + n)
        texture = torch.randn(Cc, H, W, generator=g)
        if n == 0:
            dirs = torch.zeros(0, 3)
        else:
            dirs = U.with_special(U.contended_dirs(n, 5) if contended else U.random_dirs(n, 6))
        d_color = torch.randn(dirs.shape[0], Cc, generator=g)
        ref = {}
        for act in ACTS:
            unit, n_t = U.backward_unit(texture, dirs, d_color, act)
            ref[act] = (U.texture_color(texture, dirs, act), U.texture_grad(texture, dirs, d_color, act), unit, n_t)
        _CASES[key] = (texture, dirs, d_color, ref)
    return _CASES[key]


def _check_texture(shape, act, contended=False):
    from scaledreamer_amd import ops

    texture, dirs, d_color, ref = _case(shape, contended)
    want_color, want_grad, unit, n_t = ref[act]
    tex_d, dirs_d, dcol_d = texture.cuda(), dirs.cuda(), d_color.cuda()
    color = ops.bg_texture_fwd(tex_d, dirs_d, _act_id(act))
    grad = ops.bg_texture_bwd(tex_d, dirs_d, dcol_d, _act_id(act))
    torch.cuda.synchronize()
    assert color.shape == want_color.shape and grad.shape == texture.shape
    tol = U.forward_tolerance(texture, act)
    err = float((color.cpu().double() - want_color).abs().max()) if dirs.shape[0] else 0.0
    diff = (grad.cpu().double() - want_grad).abs()
    touched = (n_t > 0)[None].expand_as(diff)
    ratio = float((diff[touched] / unit[touched].clamp_min(1e-300)).max()) if touched.any() else 0.0
    print(f"{shape}{' contended' if contended else ''} {act}: forward error {err:.3e} (tolerance {tol:.3e}), largest backward ratio {ratio:.3f} units, "
          f"most rays on one texel's neighbourhood {int(n_t.max())}")
    assert err <= tol
    assert float((diff - 8.0 * unit).max()) <= 0.0, ratio
    untouched = grad.cpu()[~touched]
    assert not untouched.any() and not torch.signbit(untouched).any()           # exactly +0.0f
    return n_t


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_texture_kernels_against_float64(shape, act):
    n_t = _check_texture(shape, act)
    if shape[3] == 0:
        assert not n_t.any()


@pytest.mark.parametrize("act", ACTS)
def test_texture_kernels_on_the_contended_view(act):
    n_t = _check_texture(CONTENDED, act, contended=True)
    assert int(n_t.max()) > 2000


def test_backward_overwrites_and_needs_no_zeroed_output():
    """d_texture is written, not accumulated: a second pass over the same inputs gives the same image within the order of the LDS adds"""
    from scaledreamer_amd import ops

    texture, dirs, d_color, ref = _case(SHAPES[0])
    _, want_grad, unit, _ = ref["sigmoid"]
    a = ops.bg_texture_bwd(texture.cuda(), dirs.cuda(), d_color.cuda())
    b = ops.bg_texture_bwd(texture.cuda(), dirs.cuda(), d_color.cuda())
    for got in (a, b):
        assert float(((got.cpu().double() - want_grad).abs() - 8.0 * unit).max()) <= 0.0


def test_workspace_follows_the_ray_count():
    """the slabs of the backward pass are sized from n: a 4,096-ray call writes a handful, not one per CU"""
    from scaledreamer_amd._lib import check, i32, lib

    def floats(Cc, H, W, n):
        nf = C.c_int64(-1)
        check(lib().asd_bg_texture_bwd_workspace(i32(Cc), i32(H), i32(W), i32(n), C.byref(nf)))
        return nf.value

    image = 3 * 64 * 64
    assert floats(3, 64, 64, 0) == 0 and floats(3, 64, 64, 64) == 0                 # one workgroup writes d_texture itself
    assert 2 * image <= floats(3, 64, 64, 4096) <= 16 * image
    assert floats(3, 64, 64, 4096) < floats(3, 64, 64, 16384) <= 64 * image
    assert floats(3, 64, 64, 1 << 24) <= 256 * image
    assert floats(3, 128, 128, 20000) == 0                                          # global atomics: no slabs


def test_entries_refuse_bad_sizes_without_a_launch():
    from scaledreamer_amd._lib import i32, lib, ptr, stream

    l = lib()
    tex, dirs = torch.zeros(3, 4, 4, device="cuda"), torch.zeros(8, 3, device="cuda")
    out, dcol, dtex = torch.full((8, 9), 7.0, device="cuda"), torch.zeros(8, 9, device="cuda"), torch.full((9, 4, 4), 7.0, device="cuda")
    nf = C.c_int64(-1)
    for Cc, H, W in ((0, 4, 4), (9, 4, 4), (3, 0, 4), (3, 4, 0), (3, -1, 4)):
        assert l.asd_bg_texture_fwd(ptr(tex), i32(Cc), i32(H), i32(W), i32(1), ptr(dirs), i32(8), ptr(out), stream()) == 1
        assert l.asd_last_error()
        assert l.asd_bg_texture_bwd_workspace(i32(Cc), i32(H), i32(W), i32(8), C.byref(nf)) == 1 and nf.value == -1
        assert l.asd_bg_texture_bwd(ptr(tex), i32(Cc), i32(H), i32(W), i32(1), ptr(dirs), ptr(dcol), i32(8), ptr(dtex), None, stream()) == 1
    assert l.asd_bg_texture_fwd(ptr(tex), i32(3), i32(4), i32(4), i32(2), ptr(dirs), i32(8), ptr(out), stream()) == 1       # no such activation
    assert l.asd_bg_texture_fwd(ptr(tex), i32(3), i32(4), i32(4), i32(1), ptr(dirs), i32(-1), ptr(out), stream()) == 1
    for Cc, V, R in ((0, 1, 8), (9, 1, 8), (3, -1, 8), (3, 1, -8)):
        assert l.asd_bg_solid_fwd(ptr(tex), i32(Cc), i32(V), i32(R), ptr(out), stream()) == 1
        assert l.asd_bg_solid_bwd(ptr(dcol), i32(Cc), i32(V), i32(R), ptr(dtex), stream()) == 1
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((dtex == 7.0).all())                 # nothing was launched
    assert l.asd_bg_texture_fwd(ptr(tex), i32(3), i32(4), i32(4), i32(1), ptr(dirs), i32(0), ptr(out), stream()) == 0        # n = 0: success, nothing written
    assert l.asd_bg_solid_fwd(ptr(tex), i32(3), i32(0), i32(8), ptr(out), stream()) == 0
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


def _plugin(name, cfg):
    import scaledreamer_amd.plugins  # noqa: F401
    from scaledreamer_amd.registry import find

    return find(name)(cfg).cuda().train()


def test_textured_plugin_with_a_composed_activation():
    """color_activation "tanh": the kernels run with "none", networks.get_activation on top, autograd composes the two"""
    texture, dirs, d_color, _ = _case(SHAPES[1])
    Cc, H, W, _n = SHAPES[1]
    bg = _plugin("textured-background", {"n_output_dims": Cc, "height": H, "width": W, "color_activation": "tanh"})
    bg.load_state_dict({"texture": texture[None]})
    view = dirs[:1000].view(2, 20, 25, 3).cuda()
    color = bg(view)
    assert color.shape == (2, 20, 25, Cc)
    (color * d_color[:1000].view(2, 20, 25, Cc).cuda()).sum().backward()
    want = U.texture_color(texture, dirs[:1000], "tanh")
    err = float((color.detach().cpu().double().view(-1, Cc) - want).abs().max())
    tol = U.forward_tolerance(texture, "none")                  # max |tanh'| = 1
    t64 = texture.double().requires_grad_(True)
    s = U.texture_sample(t64, dirs[:1000])
    want_grad = torch.autograd.grad(torch.tanh(s), t64, d_color[:1000].double())[0]
    # the backward unit with d_color tanh' as the kernel's d_color and no fused activation
    unit, n_t = U.backward_unit(texture, dirs[:1000], d_color[:1000].double() * (1 - torch.tanh(s.detach()) ** 2), "none")
    diff = (bg.texture.grad[0].cpu().double() - want_grad).abs()
    print(f"tanh plugin: forward error {err:.3e} (tolerance {tol:.3e}), largest backward ratio {float((diff / unit.clamp_min(1e-300)).max()):.3f} units")
    assert err <= tol + 2.0 ** -23                             # + tanh's own fp32 rounding of a value in [-1, 1]
    assert float((diff - 8.0 * unit).max()) <= 0.0
    with torch.no_grad():                                       # validation / export: the forward entry alone
        again = bg.eval()(view)
    assert torch.equal(again, color.detach()) and not again.requires_grad


@pytest.mark.parametrize("Cc", (1, 3, 4, 8))
@pytest.mark.parametrize("R", (1, 257, 4096))
@pytest.mark.parametrize("V", (1, 3))
def test_solid_kernels(V, R, Cc):
    from scaledreamer_amd import ops

    g = torch.Generator().manual_seed(V * 100000 + R * 10 + Cc)
    colors = torch.rand(V, Cc, generator=g)
    d_out = torch.randn(V * R, Cc, generator=g)
    out = ops.bg_solid_fwd(colors.cuda(), R)
    assert torch.equal(out.cpu(), U.solid_color(colors, R))                        # the forward is exact
    grad = ops.bg_solid_bwd(d_out.cuda(), V).cpu().double()
    bound = R * 2.0 ** -24 * d_out.double().abs().view(V, R, Cc).sum(1)
    diff = (grad - U.solid_grad(d_out, V)).abs()
    print(f"solid V={V} R={R} C={Cc}: largest backward ratio {float((diff / bound).max()):.2e} of R 2^-24 sum|terms|")
    assert float((diff - bound).max()) <= 0.0


def test_solid_plugin_on_the_device():
    dirs = torch.nn.functional.normalize(torch.randn(3, 8, 8, 3, generator=torch.Generator().manual_seed(2)), dim=-1).cuda()
    d_color = torch.randn(3, 8, 8, 4, generator=torch.Generator().manual_seed(3)).cuda()
    bg = _plugin("solid-color-background", {"n_output_dims": 4, "color": (0.1, 0.2, 0.3, 0.4), "learned": True, "random_aug": True})
    bg.rand_fn = lambda: 0.9
    out = bg(dirs)
    assert out.shape == (3, 8, 8, 4) and torch.equal(out.detach(), bg.env_color.detach().expand(3, 8, 8, 4))
    (out * d_color).sum().backward()
    want = d_color.double().sum((0, 1, 2))
    assert float((bg.env_color.grad.double() - want).abs().max()) <= 192 * 2.0 ** -24 * float(d_color.double().abs().sum((0, 1, 2)).max())
    bg.env_color.grad = None
    rc = torch.rand(3, 1, 1, 4, generator=torch.Generator().manual_seed(4))
    bg.rand_fn, bg.rand_color_fn = (lambda: 0.1), (lambda b, c: rc)
    out = bg(dirs)                                              # per-view random colours: V = B
    assert torch.equal(out.detach().cpu(), rc.expand(3, 8, 8, 4))
    (out * d_color).sum().backward()
    assert bg.env_color.grad is not None and not bg.env_color.grad.any()           # `color * 0 +`: in the graph, zero gradient
    fixed = _plugin("solid-color-background", {}).eval()
    with torch.no_grad():
        white = fixed(dirs)
    assert white.shape == (3, 8, 8, 3) and bool((white == 1.0).all())


def test_textured_background_under_the_fused_training_pass(monkeypatch):
    """A reduced `nerf-volume-renderer` system with background_type "textured-background", 1 x 16 x 16 rays, one forward + backward on
    the fused training pass: texture.grad equals, within the backward tolerance, the gradient obtained when the same renderer is fed
    the float64 restatement's background (cast to fp32) as a leaf tensor and that leaf's gradient is pushed through the restatement."""
    from scaledreamer_amd import presets
    from scaledreamer_amd.registry import find
    from scaledreamer_amd.renderer import NeRFVolumeRenderer

    torch.manual_seed(0)
    with presets.random_weights_allowed():
        cfg = presets.asd_sd_nerf()["system"]
    cfg.update(guidance_type="", optimizer={}, background_type="textured-background", background={})
    cfg["renderer"] = {**cfg["renderer"], "num_samples_per_ray": 64, "grid_prune": False}
    cfg["material"]["requires_normal"] = False
    system = find("scaledreamer-system")(cfg).train()
    ren, bg = system.renderer, system.background
    assert type(bg).__name__ == "TexturedBackground" and ren.background is bg
    fused_calls, real = [], NeRFVolumeRenderer._forward_fused_pass
    monkeypatch.setattr(NeRFVolumeRenderer, "_forward_fused_pass", lambda self, *a, **k: fused_calls.append(1) or real(self, *a, **k))

    n = 16
    px = (torch.arange(n, dtype=torch.float32) + 0.5) / n - 0.5
    eye = torch.tensor([1.5, 1.2, 0.9])
    fwd = -eye / eye.norm()
    right = torch.nn.functional.normalize(torch.linalg.cross(fwd, torch.tensor([0.0, 0.0, 1.0])), dim=0)
    up = torch.linalg.cross(right, fwd)
    rays_d = torch.nn.functional.normalize(fwd + 0.8 * px[None, :, None] * right + 0.8 * px[:, None, None] * up, dim=-1)[None].contiguous().cuda()
    rays_o = eye.expand(1, n, n, 3).contiguous().cuda()
    jitter = torch.rand(n * n, generator=torch.Generator().manual_seed(1)).cuda()
    ren.jitter_fn = lambda m, device: jitter
    weight = torch.linspace(0.5, 1.5, 3, device="cuda")

    def step():
        out = system.renderer(rays_o=rays_o, rays_d=rays_d, light_positions=rays_o[:, 0, 0])
        (out["comp_rgb"] * weight).sum().backward()
        return out

    out = step()
    assert fused_calls == [1]
    got = bg.texture.grad[0].detach().cpu().double()
    assert torch.isfinite(got).all() and float(got.abs().max()) > 0

    texture, dirs = bg.texture.detach()[0].cpu(), rays_d.view(-1, 3).cpu()
    leaf = U.texture_color(texture, dirs, "sigmoid").float().view(1, n, n, 3).cuda().requires_grad_(True)
    ren.set_background(lambda dirs: leaf)
    out2 = step()
    assert fused_calls == [1, 1] and torch.allclose(out2["comp_rgb"], out["comp_rgb"], rtol=0, atol=1e-5)
    d_color = leaf.grad.view(-1, 3).cpu()
    want = U.texture_grad(texture, dirs, d_color, "sigmoid")
    unit, n_t = U.backward_unit(texture, dirs, d_color, "sigmoid")
    diff = (got - want).abs()
    print(f"fused training pass: largest texture.grad ratio {float((diff / unit.clamp_min(1e-300)).max()):.3f} units, |grad| max {float(got.abs().max()):.3e}")
    assert float((diff - 8.0 * unit).max()) <= 0.0
    assert not got[:, n_t == 0].any()
