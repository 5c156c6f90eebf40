"""The analytic-normal field kernels (asd_field_analytic_fwd / _bwd, csrc/field_analytic.hip) against the float64 oracle of
field_analytic_util.py, and the `implicit-volume` route (normal_type "analytic") built on them.

Tolerance: an output must be within MARGIN x E32 of the float64 oracle (max-norm, relative to the oracle's max magnitude), where E32 is
the error of the same mathematics evaluated in float32 on the CPU (field_analytic_util.E32, guarded by test_field_analytic_cpu.py).
MARGIN = 4 covers what that float32 evaluation does not share with the kernels: fma contraction, the order of the 64-term and 8-corner
sums, the arbitrary order of the atomic scatter.  Samples on a discontinuity of the derivative (cell faces, ReLU kinks:
field_analytic_util.left_out) are left out of the comparisons, at most 10 % of a test's samples; they take part in every launch and their
outputs must be finite.

Measured on an MI355X, kernel error / E32 (n = 257 unless stated; no term needs more than the margin of 4):

forward (kernel error / E32)      sigma              features           grad               normal
  A softplus+magic3d            1.60e-07/1.60e-07  5.91e-06/5.91e-06  3.33e-06/3.37e-06  2.47e-05/2.45e-05
  A exp+const                   2.29e-06/2.18e-06  5.91e-06/5.91e-06  9.43e-06/9.30e-06  3.46e-05/3.46e-05
  A none+sphere (SDF)           2.25e-06/2.10e-06  5.91e-06/5.91e-06  1.08e-05/1.09e-05  2.85e-05/2.84e-05
  A trunc_exp+dreamfusion       3.61e-07/4.87e-07  5.91e-06/5.91e-06  3.46e-06/3.50e-06  2.73e-05/2.74e-05
  A softplus+magic3d n=1        1.32e-07/1.32e-07  2.04e-06/1.97e-06  1.12e-06/1.12e-06  5.31e-07/4.49e-07
  B softplus+magic3d            3.20e-06/3.20e-06  1.18e-04/1.18e-04  3.49e-04/3.49e-04  5.81e-04/5.80e-04
backward, cotangents: all           d_grid             d_w1d             d_w2d             d_w1f             d_w2f
  A softplus+magic3d            1.88e-05/1.88e-05  1.35e-05/1.34e-05  1.01e-05/9.62e-06  7.41e-06/7.40e-06  5.17e-06/5.32e-06
  A exp+const                   1.91e-05/1.93e-05  1.78e-05/1.76e-05  2.91e-05/2.94e-05  7.41e-06/7.40e-06  5.17e-06/5.32e-06
  A none+sphere (SDF)           2.93e-05/2.93e-05  3.14e-05/3.25e-05  2.53e-05/2.55e-05  7.41e-06/7.40e-06  5.17e-06/5.32e-06
  A trunc_exp+dreamfusion       6.42e-06/6.51e-06  9.66e-06/9.68e-06  9.73e-06/9.80e-06  7.41e-06/7.40e-06  5.17e-06/5.32e-06
  A softplus+magic3d n=1        7.24e-06/7.22e-06  7.45e-06/7.45e-06  1.01e-05/1.02e-05  6.99e-06/7.00e-06  3.75e-06/3.80e-06
  B softplus+magic3d            8.56e-04/8.57e-04  3.57e-04/3.57e-04  3.33e-04/3.32e-04  1.59e-04/1.59e-04  8.99e-05/8.96e-05
backward, cotangents: normal        d_grid             d_w1d             d_w2d
  A softplus+magic3d            1.92e-05/1.92e-05  1.32e-05/1.31e-05  9.96e-06/9.64e-06
  A exp+const                   1.90e-05/1.92e-05  1.78e-05/1.76e-05  3.10e-05/3.13e-05
  A none+sphere (SDF)           2.95e-05/2.94e-05  3.24e-05/3.36e-05  2.44e-05/2.45e-05
  A trunc_exp+dreamfusion       2.35e-05/2.39e-05  3.01e-05/3.00e-05  3.49e-05/3.52e-05
  A softplus+magic3d n=1        6.22e-06/6.22e-06  7.44e-06/7.45e-06  1.00e-05/1.02e-05
  B softplus+magic3d            8.57e-04/8.58e-04  3.55e-04/3.55e-04  3.31e-04/3.31e-04
backward, cotangents: sigma         d_grid             d_w1d             d_w2d
  A softplus+magic3d            6.90e-06/6.89e-06  8.01e-06/8.01e-06  8.55e-06/8.52e-06
  A exp+const                   4.32e-06/4.36e-06  5.78e-06/5.75e-06  4.39e-06/4.09e-06
  A none+sphere (SDF)           5.02e-06/5.02e-06  6.56e-06/6.59e-06  5.08e-06/4.84e-06
  A trunc_exp+dreamfusion       6.46e-06/6.51e-06  9.68e-06/9.68e-06  9.90e-06/9.83e-06
  A softplus+magic3d n=1        3.26e-06/3.27e-06  7.02e-06/7.02e-06  5.01e-06/5.33e-06
  B softplus+magic3d            8.33e-05/8.33e-05  6.56e-05/6.56e-05  6.91e-05/6.91e-05
largest kernel error / E32 over all of them: 1.18

sigma, features and the saved encoding are bit-identical to asd_field_fwd's; with d_sigma alone the gradients equal asd_field_bwd's to
1.7e-7 .. 3.9e-7 of their max magnitude.
"""
import numpy as np
import pytest
import torch

import field_analytic_util as U

pytestmark = pytest.mark.gpu

MARGIN = 4.0
FWD_CASES = [("A", c, 257) for c in ("softplus_magic3d", "exp_const", "none_sphere_sdf", "truncexp_dreamfusion")] + [
    ("A", "softplus_magic3d", 1), ("B", "softplus_magic3d", 257)]
BWD_CASES = FWD_CASES


def _dev(a):
    return torch.as_tensor(np.asarray(a)).cuda()


def _params(c):
    return [_dev(getattr(c.P, k)) for k in U.PARAMS]


def _check(name, got, ref, e32, rows=None, scale=1.0):
    err = U.rel_err(got, scale * torch.as_tensor(ref), rows)
    print(f"    {name:<20s} kernel error {err:.3e}   E32 {e32:.3e}   ratio {err / max(e32, 1e-300):.2f}")
    return err <= MARGIN * e32, f"{name}: error {err:.3e} > {MARGIN} x E32 {e32:.3e}"


def _forward(c):
    from scaledreamer_amd import ops

    return ops.field_analytic_fwd(c.meta, U.field_cfg(c.cfg), *_params(c), _dev(c.pts), want_grad=True)


def _backward(c, on, fwd=None, d_grid=None, dws=None):
    """cotangents of the set `on`, zero at the left-out samples (the oracle's loss runs over the kept samples only)"""
    from scaledreamer_amd import ops

    sigma, feats, normal, grad, enc = fwd if fwd is not None else _forward(c)
    keep = _dev(c.keep.astype(np.float32))
    cot = {k: (_dev(getattr(c.cot, k)) * (keep if k == "sigma" else keep[:, None])).contiguous() if k in on else None
           for k in ("sigma", "features", "normal")}
    grid = _params(c)[0]
    d_grid = torch.zeros_like(grid) if d_grid is None else d_grid
    dws = ops.field_analytic_bwd(c.meta, U.field_cfg(c.cfg), *_params(c), _dev(c.pts), enc, sigma, cot["sigma"], cot["features"],
                                 cot["normal"], d_grid, dws=dws)
    return dict(zip(U.PARAMS, (d_grid,) + tuple(dws))), cot


@pytest.mark.parametrize("meta,cfg,n", FWD_CASES)
def test_forward_matches_the_float64_oracle(meta, cfg, n):
    c = U.case(meta, cfg, n, with_bwd=False)
    assert 1.0 - c.keep.mean() <= U.MAX_LEFT_OUT
    e32 = U.E32[f"{meta}/{cfg}/{n}"]
    sigma, feats, normal, grad, enc = _forward(c)
    got = {"sigma": sigma, "features": feats, "grad": grad, "normal": normal}
    for k, v in got.items():
        assert torch.isfinite(v).all(), k           # the left-out samples too
    fails = [msg for ok, msg in (_check(k, got[k], getattr(c.ref, k), e32[k], c.keep) for k in U.OUTPUTS) if not ok]
    assert not fails, fails
    if cfg == "truncexp_dreamfusion":
        assert int((c.ref.raw[c.keep] > 15).sum()) >= 3          # the clamped branch of trunc_exp's derivative is exercised


@pytest.mark.parametrize("meta,cfg,n", [("A", "softplus_magic3d", 257), ("A", "none_sphere_sdf", 257), ("B", "softplus_magic3d", 257)])
def test_sigma_and_features_are_those_of_the_finite_difference_entry(meta, cfg, n):
    """one call serves geometry(points, output_normal=True): sigma, features and the saved encoding are asd_field_fwd's.
    Measured on MI355X: bit-identical (the MLP runs in mlp1's / mlpC's order of operations on asd_encode's encoding)."""
    from scaledreamer_amd import ops

    c = U.case(meta, cfg, n, with_bwd=False)
    sigma, feats, _, _, enc = _forward(c)
    s0, f0, _, e0 = ops.field_fwd(c.meta, U.field_cfg(c.cfg), *_params(c), _dev(c.pts), False)
    print("    bit-identical:", bool(torch.equal(sigma, s0) and torch.equal(feats, f0) and torch.equal(enc, e0)))
    torch.testing.assert_close(sigma, s0, rtol=1e-6, atol=0)
    torch.testing.assert_close(feats, f0, rtol=1e-6, atol=1e-9)
    torch.testing.assert_close(enc, e0, rtol=1e-6, atol=0)


@pytest.mark.parametrize("meta,cfg,n", BWD_CASES)
@pytest.mark.parametrize("cot_set", ["all", "normal", "sigma"])
def test_backward_matches_the_oracles_double_backward(meta, cfg, n, cot_set):
    from scaledreamer_amd import ops

    c = U.case(meta, cfg, n)
    e32 = U.E32[f"{meta}/{cfg}/{n}"]
    on = U.COT_SETS[cot_set]
    fwd = _forward(c)
    got, cot = _backward(c, on, fwd)
    fails = []
    for k in U.PARAMS:
        assert torch.isfinite(got[k]).all(), k
        ref = c.dref[cot_set][k]
        if float(ref.abs().max()) == 0.0:           # the feature network under a loss on sigma or the normal alone
            assert float(got[k].abs().max()) == 0.0, k
            continue
        ok, msg = _check(f"{cot_set}/d_{k}", got[k].reshape(ref.shape), ref, e32[f"{cot_set}/d_{k}"])
        if not ok:
            fails.append(msg)
    assert not fails, fails
    if cot_set == "sigma":
        # d_sigma alone: the value path only, which asd_field_bwd computes too.  Each is within MARGIN x E32 of float64, so of each other
        # within twice that.
        sigma, feats, normal, grad, enc = fwd
        d0 = torch.zeros_like(got["grid"])
        dw0 = ops.field_bwd(c.meta, U.field_cfg(c.cfg), *_params(c), _dev(c.pts), enc, sigma, cot["sigma"], None, None, d0)
        for k, v in zip(U.PARAMS[:3], (d0, dw0[0], dw0[1])):
            err = U.rel_err(got[k], v.reshape(got[k].shape))
            print(f"    sigma/d_{k} against asd_field_bwd: {err:.3e}")
            assert err <= 2 * MARGIN * e32[f"sigma/d_{k}"], k


def test_backward_accumulates():
    """the += contract: a second call into the same buffers doubles them (against twice the float64 oracle, at the same bound)"""
    meta, cfg, n = "A", "softplus_magic3d", 257
    c = U.case(meta, cfg, n)
    e32 = U.E32[f"{meta}/{cfg}/{n}"]
    fwd = _forward(c)
    got, _ = _backward(c, U.COT_SETS["all"], fwd)
    once = {k: v.clone() for k, v in got.items()}
    got2, _ = _backward(c, U.COT_SETS["all"], fwd, d_grid=got["grid"], dws=tuple(got[k] for k in U.PARAMS[1:]))
    fails = []
    for k in U.PARAMS:
        assert got2[k].data_ptr() == got[k].data_ptr()
        ref = c.dref["all"][k]
        ok, msg = _check(f"2 x all/d_{k}", got2[k].reshape(ref.shape), ref, e32[f"all/d_{k}"], scale=2.0)
        if not ok:
            fails.append(msg)
        assert float((got2[k] - 2 * once[k]).abs().max()) <= 2 * MARGIN * e32[f"all/d_{k}"] * float(once[k].abs().max()), k
    assert not fails, fails


def test_gradient_equals_central_differences_of_the_density_entry():
    """Property against an existing kernel.  With no activation and a constant bias the field is, inside one cell of every level and with
    no ReLU changing side, linear along each axis: the central difference of asd_field_density over +-e is its derivative up to the
    cancellation error 4 * 2^-23 * |sigma| / e, and nothing else.  The points are those whose +-e neighbours stay in the cell of every
    level (with 1e-3 of a cell to spare: positions are rounded to 2^-16 of a cell at scale 204) and keep every hidden unit's sign.
    Measured on an MI355X: max |fd - grad| / tolerance = 0.55, 0.36, 0.49 on the three axes, |grad| up to 20."""
    from scaledreamer_amd import ops

    e = 2.5e-4          # 0.026 of the finest level's cell: about half of the drawn points keep +-e inside their cell on all 16 levels
    meta, P, pts, _ = U.draw("A", 1024)
    cfg = U.CFGS["none_const"]
    ref = U.run(meta, cfg, P, pts, torch.float64)
    ok = torch.ones(len(pts), dtype=torch.bool)
    for l in range(16):
        frac = ref.pos[:, l] - torch.floor(ref.pos[:, l])
        d = float(meta.scale[l]) * e / (2 * U.RADIUS) + 1e-3
        ok &= ((frac > d) & (frac < 1 - d)).all(-1)
    for k in range(3):
        for sgn in (-1.0, 1.0):
            q = pts.astype(np.float64).copy()
            q[:, k] += sgn * e
            ok &= ((U.run(meta, cfg, P, q, torch.float64).a_d > 0) == (ref.a_d > 0)).all(-1)
    ok &= torch.as_tensor(~U.left_out(meta, ref))
    pts = pts[ok.numpy()][:128]
    assert len(pts) >= 32, len(pts)
    fc = U.field_cfg(cfg)
    par = [_dev(getattr(P, k)) for k in U.PARAMS]
    p = _dev(pts)
    sigma, _, _, grad, _ = ops.field_analytic_fwd(meta, fc, *par, p, want_grad=True)
    worst = 0.0
    for k in range(3):
        hi, lo = p.clone(), p.clone()
        hi[:, k] += e
        lo[:, k] -= e
        step = (hi[:, k] - lo[:, k]).double()                     # the step the float32 positions really take
        s_hi = ops.field_density(meta, fc, *par[:3], hi).double()
        s_lo = ops.field_density(meta, fc, *par[:3], lo).double()
        fd = (s_hi - s_lo) / step
        tol = 4 * 2.0 ** -23 * sigma.double().abs() / e
        ratio = ((fd - grad[:, k].double()).abs() / tol).max().item()
        worst = max(worst, ratio)
        print(f"    axis {k}: max |fd - grad| / tolerance = {ratio:.3f}   (|grad| up to {grad[:, k].abs().max().item():.3f})")
    assert worst <= 1.0


def _geometry(c):
    import scaledreamer_amd.plugins  # noqa: F401
    from scaledreamer_amd.registry import find

    geo = find("implicit-volume")({"radius": 1.0, "normal_type": "analytic"})
    sd = {"encoding.encoding.encoding.params": c.P.grid, "density_network.layers.0.weight": c.P.w1d, "density_network.layers.2.weight": c.P.w2d,
          "feature_network.layers.0.weight": c.P.w1f, "feature_network.layers.2.weight": c.P.w2f}
    geo.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
    return geo.cuda().train()


def test_geometry_route():
    """ImplicitVolume({"normal_type": "analytic"}) is meta B with the shipped cfg: the outputs and, for a loss on the normal alone, the
    parameter gradients are those of the kernel tests above."""
    meta, cfg, n = "B", "softplus_magic3d", 257
    c = U.case(meta, cfg, n)
    e32 = U.E32[f"{meta}/{cfg}/{n}"]
    geo = _geometry(c)
    assert geo.fused
    pts = _dev(c.pts).view(1, n, 3)
    with torch.no_grad():
        out = geo(pts, output_normal=True)
    assert set(out) == {"density", "features", "normal", "shading_normal"}
    assert out["density"].shape == (1, n, 1) and out["features"].shape == (1, n, 3) and out["normal"].shape == (1, n, 3)
    assert out["shading_normal"].shape == (1, n, 3) and not any(v.requires_grad for v in out.values())
    with pytest.raises(ValueError, match="n_dev"):
        geo(pts.view(n, 3), output_normal=True, n_dev=torch.tensor(n, dtype=torch.int32, device="cuda"))
    out = geo(pts, output_normal=True)
    assert all(out[k].requires_grad for k in ("density", "features", "normal"))
    fails = [msg for ok, msg in (_check(k, out[o].reshape(getattr(c.ref, k).shape), getattr(c.ref, k), e32[k], c.keep)
                                 for k, o in (("sigma", "density"), ("features", "features"), ("normal", "normal"))) if not ok]
    assert not fails, fails
    cot = _dev(c.cot.normal) * _dev(c.keep.astype(np.float32))[:, None]
    (out["normal"].view(n, 3) * cot).sum().backward()
    got = {"grid": geo.encoding.encoding.encoding.params.grad, "w1d": geo.density_network.layers[0].weight.grad,
           "w2d": geo.density_network.layers[2].weight.grad}
    fails = [msg for ok, msg in (_check(f"normal/d_{k}", got[k].reshape(c.dref["normal"][k].shape), c.dref["normal"][k], e32[f"normal/d_{k}"])
                                 for k in got) if not ok]
    assert not fails, fails
    for w in (geo.feature_network.layers[0].weight, geo.feature_network.layers[2].weight):
        assert w.grad is not None and float(w.grad.abs().max()) == 0.0


class _SolidBackground(torch.nn.Module):
    def forward(self, dirs, **kwargs):
        return torch.full_like(dirs, 0.5)


def test_renderer_route_orientation_loss():
    """nerf-volume-renderer over the analytic geometry, a material that asks for normals, 16 x 16 rays: out["normal"] exists, the reference's
    orientation loss (systems/scaledreamer.py:75-78) is finite and its backward reaches the hash grid."""
    import scaledreamer_amd.plugins  # noqa: F401
    from scaledreamer_amd.registry import find

    torch.manual_seed(0)
    geo = find("implicit-volume")({"radius": 1.0, "normal_type": "analytic"})
    mat = find("no-material")({"n_output_dims": 3, "color_activation": "sigmoid", "requires_normal": True})
    ren = find("nerf-volume-renderer")({"radius": 1.0, "num_samples_per_ray": 64}, geometry=geo, material=mat, background=_SolidBackground())
    for m in (geo, mat, ren):
        m.cuda().train()
    ren.update_step(0, 0)           # the occupancy grid starts empty: its first update marks the cells the density blob fills
    ys, xs = torch.meshgrid(torch.linspace(-0.4, 0.4, 16), torch.linspace(-0.4, 0.4, 16), indexing="ij")
    rays_d = torch.nn.functional.normalize(torch.stack([xs, ys, -torch.ones_like(xs)], -1), dim=-1).view(1, 16, 16, 3).cuda()
    rays_o = torch.tensor([0.0, 0.0, 2.0]).expand(1, 16, 16, 3).contiguous().cuda()
    out = ren(rays_o=rays_o, rays_d=rays_d, light_positions=torch.zeros(1, 3, device="cuda"))
    assert "normal" in out
    normal = out["normal"]
    assert normal.shape == (out["weights"].shape[0], 3) and normal.shape[0] > 16 and normal.requires_grad
    loss_orient = (out["weights"].detach() * (normal * out["t_dirs"]).sum(-1, keepdim=True).clamp_min(0.0) ** 2).sum() / (out["opacity"] > 0).sum()
    assert torch.isfinite(loss_orient) and loss_orient.item() > 0
    grid = geo.encoding.encoding.encoding.params
    grid.grad = None
    loss_orient.backward()
    assert grid.grad is not None and torch.isfinite(grid.grad).all() and float(grid.grad.abs().max()) > 0
    assert float(geo.density_network.layers[0].weight.grad.abs().max()) > 0
