"""The level limit of the hash grid (asd_grid_meta.n_masked_levels) in asd_hashgrid_*, asd_field_density / _fwd / _bwd, and the coarse-to-fine
`implicit-sdf` route built on it (ProgressiveBandHashGrid + finite_difference_normal_eps "progressive").

Oracle: field_progressive_util.py (float64 restatement, encode times the reference's 0/1 mask); tolerance MARGIN x E32 as in
test_gpu_field_analytic.py.  Exact statements (masked columns, masked table ranges, masked dW1 columns) are compared with == 0.
n = 257 (one block plus one row), n_dev = 200 of 257 where the entry takes it; metas "A" (small tables, heavy collisions: the fine levels
go through the transposed-lane atomics) and "B" (the shipped grid: the fine levels go through the paged scatter).
Level counts 4, 5, 6 straddle ASD_FIELD_NAGG = 5: the last run-aggregated level, the first paged level and one beyond.

Measured on an MI355X (the tests print every figure): over the 187 compared outputs and gradients the largest kernel error / E32 is 1.49
(fd/d_grid, meta A, 4 levels); the forward outputs sit at 0.86 .. 1.37; limited and all-levels-with-zeroed-W1 forwards are bit-identical.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import field_progressive_util as U

pytestmark = pytest.mark.gpu

MARGIN = 4.0
HASH_LEVELS = (0, 1, 4, 5, 6, 16)


def _dev(a):
    return torch.as_tensor(np.asarray(a)).cuda()


def _params(c, zero_cols_from=None):
    ps = [_dev(getattr(c.P, k)) for k in U.PARAMS]
    if zero_cols_from is not None:
        ps[1][:, zero_cols_from:] = 0.0
        ps[3][:, zero_cols_from:] = 0.0
    return ps


def _check(name, got, ref, e32, rows=None):
    err = U.rel_err(got, ref, rows)
    print(f"    {name:<20s} kernel error {err:.3e}   E32 {e32:.3e}   ratio {err / max(e32, 1e-300):.2f}")
    return err <= MARGIN * e32, f"{name}: error {err:.3e} > {MARGIN} x E32 {e32:.3e}"


def _unit(pts):
    return ((pts + U.RADIUS) / (2 * U.RADIUS)).astype(np.float32)


# ---- asd_hashgrid_fwd / _bwd ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("meta_name", ["A", "B"])
def test_hashgrid_fwd_is_the_oracle_encode_times_the_mask(oracle, meta_name):
    from scaledreamer_amd import ops

    _, P, pts, _ = U.draw(meta_name, U.N)
    x = _unit(pts)
    full = oracle.hashgrid_fwd(oracle.grid_meta(*U.METAS[meta_name]), P.grid, x)
    for a in HASH_LEVELS:
        got = ops.hashgrid_fwd(U.limited_meta(meta_name, a), _dev(P.grid), _dev(x)).cpu().numpy()
        want = full * U.column_mask(a).numpy().astype(np.float32)
        np.testing.assert_array_equal(got[:, : 2 * a], want[:, : 2 * a], err_msg=f"a = {a}")
        assert not got[:, 2 * a:].any() and not np.signbit(got[:, 2 * a:]).any(), f"a = {a}: masked columns must be +0.0"


@pytest.mark.parametrize("meta_name", ["A", "B"])
def test_hashgrid_bwd_ignores_masked_dout(oracle, meta_name):
    from scaledreamer_amd import ops

    _, P, pts, _ = U.draw(meta_name, U.N)
    x = _unit(pts)
    om = oracle.grid_meta(*U.METAS[meta_name])
    dout = np.random.default_rng(11).normal(size=(U.N, 32)).astype(np.float32)      # dense: masked columns carry values too
    for a in HASH_LEVELS:
        m = U.limited_meta(meta_name, a)
        g = ops.hashgrid_bwd(m, _dev(x), _dev(dout)).cpu().numpy()
        first_masked = 2 * int(m.offset[a]) if a < 16 else g.size
        assert not g[first_masked:].any(), f"a = {a}: dparams beyond offset[{a}] touched"
        want = oracle.hashgrid_bwd(om, x, dout * U.column_mask(a).numpy().astype(np.float32))
        np.testing.assert_allclose(g, want, rtol=1e-4, atol=1e-5, err_msg=f"a = {a}")      # the tolerance of test_hashgrid_fwd_bwd


def test_limit_above_n_levels_is_an_argument_error():
    from scaledreamer_amd import _lib, ops

    m = _lib.make_grid_meta(*U.METAS["A"])
    m.n_masked_levels = 17
    with pytest.raises(_lib.AsdError, match="error 1: .*n_masked_levels"):
        ops.hashgrid_fwd(m, torch.zeros(m.n_params, device="cuda"), torch.zeros(4, 3, device="cuda"))
    c = U.case("A", 4, with_bwd=False)
    with pytest.raises(_lib.AsdError, match="error 1: .*n_masked_levels"):
        ops.field_fwd(m, U.field_cfg(c.eps), *_params(c), _dev(c.pts), True)


# ---- asd_field_fwd / asd_field_density -----------------------------------------------------------------------------------------------------
def _forward(c, C=3, meta=None, params=None, n_dev=None):
    from scaledreamer_amd import ops

    meta = U.limited_meta(c.meta_name, c.a) if meta is None else meta
    return ops.field_fwd(meta, U.field_cfg(c.eps, C), *(params or _params(c)), _dev(c.pts), True, want_fd_grad=True, n_dev=n_dev)


@pytest.mark.parametrize("a", U.FWD_LEVELS)
@pytest.mark.parametrize("meta_name", ["A", "B"])
def test_field_forward_matches_the_float64_oracle(meta_name, a):
    from scaledreamer_amd import ops

    c = U.case(meta_name, a, with_bwd=False)
    assert 1.0 - c.keep.mean() <= U.MAX_LEFT_OUT
    e32 = U.E32[f"{meta_name}/{a}"]
    sdf, feats, normal, fd_grad, enc = _forward(c)
    got = {"sdf": sdf, "features": feats, "fd_grad": fd_grad, "normal": normal}
    for k, v in got.items():
        assert torch.isfinite(v).all(), k
    assert not enc[:, 2 * a:].any() and not torch.signbit(enc[:, 2 * a:]).any(), "masked columns of enc_save must be +0.0"
    fails = []
    for k in U.OUTPUTS:
        if a == 0 and k == "features":
            assert not feats.any()          # relu(0) . W2 = 0 exactly
            continue
        ok, msg = _check(k, got[k], getattr(c.ref, k), e32[k], c.keep)
        if not ok:
            fails.append(msg)
    assert not fails, fails
    ps = _params(c)
    dens = ops.field_density(U.limited_meta(meta_name, a), U.field_cfg(c.eps), *ps[:3], _dev(c.pts))
    assert torch.equal(dens, sdf), "asd_field_density is the centre evaluation of asd_field_fwd"
    if a == 0:      # nothing active: the sdf is the bias, to the rounding of a float32 sqrt and subtraction
        bias = torch.as_tensor(c.pts).double().norm(dim=-1) - U.CFG["bias_value"]
        assert float((sdf.cpu().double() - bias).abs().max()) <= 4 * 2.0 ** -24 * 2.0


@pytest.mark.parametrize("a", U.FWD_LEVELS)
@pytest.mark.parametrize("meta_name", ["A", "B"])
def test_limited_forward_is_the_all_levels_forward_with_zeroed_w1_columns(meta_name, a):
    """Both runs execute the same fmaf chains; the masked terms are exact zeros in the one (enc = +0) and in the other (w1 = +0), and
    x + (+-0) = x for every x the chain can hold, so the outputs are bit-identical.  (Holds as long as the 32-term sums keep their order: the
    limit only skips gathers, it does not shorten the MLP's loops.)"""
    c = U.case(meta_name, a, with_bwd=False)
    lim = _forward(c)
    full = _forward(c, meta=U.limited_meta(meta_name, 16), params=_params(c, zero_cols_from=2 * a))
    for name, x, y in zip(("sdf", "features", "normal", "fd_grad"), lim, full):
        assert torch.equal(x, y), name
    assert torch.equal(lim[4][:, : 2 * a], full[4][:, : 2 * a])


# ---- asd_field_bwd ------------------------------------------------------------------------------------------------------------------------------
def _backward(c, route):
    """the route's cotangents, zero at the left-out samples (the oracle's loss runs over the kept samples only) -> gradients by PARAMS name"""
    from scaledreamer_amd import ops

    C, on, live = U.ROUTES[route]
    n_dev = torch.tensor(live, dtype=torch.int32, device="cuda") if route == "ndev" else None
    meta = U.limited_meta(c.meta_name, c.a)
    ps = _params(c)
    sdf, feats, normal, fd_grad, enc = _forward(c, C, meta, ps, n_dev)
    keep = _dev(c.keep.astype(np.float32))
    cot = {k: (_dev(getattr(c.cot, k)) * (keep if k == "sdf" else keep[:, None])).contiguous() if k in on else None for k in U.OUTPUTS}
    d_grid = torch.zeros_like(ps[0])
    dws = ops.field_bwd(meta, U.field_cfg(c.eps, C), *ps, _dev(c.pts), enc, sdf, cot["sdf"], cot["features"], cot["normal"], d_grid,
                        n_dev=n_dev, d_fd_grad=cot["fd_grad"])
    return dict(zip(U.PARAMS, (d_grid,) + tuple(dws)))


def _assert_exact_zeros(got, meta, a):
    first_masked = 2 * int(meta.offset[a]) if a < 16 else got["grid"].numel()
    assert not got["grid"][first_masked:].any(), f"d_grid beyond offset[{a}] must be exactly 0"
    for k in ("w1d", "w1f"):
        if got[k] is not None:
            assert not got[k][:, 2 * a:].any(), f"columns >= {2 * a} of d_{k} must be exactly 0"


def _check_route(c, route, got):
    e32 = U.E32[f"{c.meta_name}/{c.a}"]
    fails = []
    for k in U.PARAMS:
        ref = c.dref[route][k]
        if got[k] is None or float(ref.abs().max()) == 0.0:      # C = 0: no feature network
            assert got[k] is None or not got[k].any(), k
            continue
        assert torch.isfinite(got[k]).all(), k
        ok, msg = _check(f"{route}/d_{k}", got[k].reshape(ref.shape), ref, e32[f"{route}/d_{k}"])
        if not ok:
            fails.append(msg)
    assert not fails, fails


@pytest.mark.parametrize("route", list(U.ROUTES))
@pytest.mark.parametrize("a", U.GRAD_LEVELS)
@pytest.mark.parametrize("meta_name", ["A", "B"])
def test_field_backward_matches_the_float64_oracle(meta_name, a, route):
    c = U.case(meta_name, a)
    got = _backward(c, route)
    _assert_exact_zeros(got, U.limited_meta(meta_name, a), a)
    _check_route(c, route, got)


@pytest.mark.parametrize("route", list(U.ROUTES))
@pytest.mark.parametrize("a", [0, 1])
@pytest.mark.parametrize("meta_name", ["A", "B"])
def test_field_backward_exact_zeros_with_one_or_no_level(meta_name, a, route):
    c = U.case(meta_name, a, with_bwd=False)
    got = _backward(c, route)
    _assert_exact_zeros(got, U.limited_meta(meta_name, a), a)
    if a == 0:      # every pre-activation is 0: no hidden unit passes gradient
        for k, v in got.items():
            assert v is None or not v.any(), f"d_{k} must be exactly 0 with no active level"


_CHILD = """
import sys, numpy as np, torch
sys.path.insert(0, {tests!r})
import test_gpu_field_progressive as T, field_progressive_util as U
c = U.case("A", 6)
got = T._backward(c, "fd")
T._assert_exact_zeros(got, U.limited_meta("A", 6), 6)
T._check_route(c, "fd", got)
print("child ok")
"""


def test_field_backward_with_the_paged_scatter_switched_off():
    """ASD_FIELD_PAGED is read once per process: a fresh child runs (A, a = 6, FD rows) with ASD_FIELD_PAGED=0"""
    env = dict(os.environ, ASD_FIELD_PAGED="0")
    r = subprocess.run([sys.executable, "-c", _CHILD.format(tests=os.path.dirname(os.path.abspath(__file__)))], env=env, capture_output=True,
                       text=True, timeout=300, cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    print(r.stdout[-3000:], r.stderr[-3000:])
    assert r.returncode == 0 and "child ok" in r.stdout


@pytest.mark.parametrize("a", [6])
def test_field_backward_paged_and_unpaged_grid_b(a):
    """meta B's levels >= 5 go through the paged scatter; the masked ones emit no items: covered by the exact zeros above.  Here: the
    gradient of the active paged level (5) is not empty, so the pass did run for a = 6 and was skipped for a <= 5."""
    c = U.case("B", a)
    got = _backward(c, "fd")
    m = U.limited_meta("B", a)
    lvl5 = got["grid"][2 * int(m.offset[5]): 2 * int(m.offset[6])]
    assert lvl5.any()


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------------------
def test_analytic_and_envmap_entries_refuse_a_limited_meta():
    from scaledreamer_amd import _lib, ops

    c = U.case("A", 4, with_bwd=False)
    meta = U.limited_meta("A", 4)
    ps = _params(c)
    with pytest.raises(_lib.AsdError, match="error 3: .*level limit"):
        ops.field_analytic_fwd(meta, U.field_cfg(c.eps), *ps, _dev(c.pts))
    sdf, feats, normal, fd_grad, enc = _forward(c)
    with pytest.raises(_lib.AsdError, match="error 3: .*level limit"):
        ops.field_analytic_bwd(meta, U.field_cfg(c.eps), *ps, _dev(c.pts), enc, sdf, torch.ones_like(sdf), None, None, torch.zeros_like(ps[0]))
    bg = _lib.make_grid_meta(4, 2, 19, 4, 4.0)
    bg.n_masked_levels = 1
    grid = torch.zeros(bg.n_params, device="cuda")
    w0, w1, w2 = torch.zeros(16, 8, device="cuda"), torch.zeros(16, 16, device="cuda"), torch.zeros(3, 16, device="cuda")
    dirs = torch.nn.functional.normalize(torch.randn(8, 3, device="cuda"), dim=-1)
    with pytest.raises(_lib.AsdError, match="error 3: .*level limit"):
        ops.envmap_fwd(bg, grid, w0, w1, w2, dirs)
    with pytest.raises(_lib.AsdError, match="error 3: .*level limit"):
        ops.envmap_bwd(bg, grid, w0, w1, w2, dirs, torch.ones(8, 3, device="cuda"))


# ---- implicit-sdf with the progressive config ---------------------------------------------------------------------------------------------------
PROG = {"otype": "ProgressiveBandHashGrid", "n_levels": 16, "n_features_per_level": 2, "log2_hashmap_size": 19, "base_resolution": 16,
        "per_level_scale": 1.447269237440378, "start_level": 4, "start_step": 0, "update_steps": 2}


def _sdf_geometry(**extra):
    import scaledreamer_amd.plugins  # noqa: F401
    from scaledreamer_amd.registry import find

    torch.manual_seed(3)
    cfg = {"radius": 1.0, "pos_encoding_config": dict(PROG), "finite_difference_normal_eps": "progressive", "sdf_bias": "sphere",
           "sdf_bias_params": 0.5, **extra}
    geo = find("implicit-sdf")(cfg).cuda().train()
    with torch.no_grad():
        geo.encoding.encoding.encoding.params.uniform_(-0.5, 0.5)        # tcnn's 1e-4 would leave the masked levels invisible
    return geo


def test_implicit_sdf_fused_route_equals_the_composed_route():
    """The geometry's two routes on the same points, 6 levels.  sdf and features: the bound test_gpu_neus_golden.py holds between its two
    routes (rtol 2e-5 / atol 1e-5).  sdf_grad is a difference quotient of two such values: its bound is theirs times 2 / eps.  The normal is
    sdf_grad over its length: twice sdf_grad's bound over the shortest length."""
    geo = _sdf_geometry()
    assert geo.fused
    geo.do_update_step(0, 4)          # 4 + 4 // 2 = 6 levels
    assert geo.encoding.encoding.current_level == 6 and geo._meta.n_masked_levels == 10
    eps = 2.0 / (16 * 1.447269237440378 ** 5)
    assert geo._fcfg.fd_eps == pytest.approx(eps, rel=1e-6)
    pts = _dev(U.draw("B", U.N)[2]).view(1, U.N, 3)
    fused = geo(pts, output_normal=True)
    composed = geo._forward_composed(pts, True)
    for k in ("sdf", "features"):
        torch.testing.assert_close(fused[k], composed[k], rtol=2e-5, atol=1e-5, msg=lambda m, k=k: f"{k}: {m}")
    d_val = 2e-5 * float(composed["sdf"].detach().abs().max()) + 1e-5
    d_grad = 2 * d_val / eps
    err = float((fused["sdf_grad"] - composed["sdf_grad"]).detach().abs().max())
    print(f"    sdf_grad: |fused - composed| = {err:.3e}, bound {d_grad:.3e}")
    assert err <= d_grad
    shortest = float(composed["sdf_grad"].detach().norm(dim=-1).min())
    err_n = float((fused["normal"] - composed["normal"]).detach().abs().max())
    print(f"    normal: |fused - composed| = {err_n:.3e}, bound {2 * d_grad / shortest:.3e}")
    assert err_n <= 2 * d_grad / shortest
    grid = geo.encoding.encoding.encoding.params
    for out in (fused, composed):
        grid.grad = None
        (out["sdf"].sum() + out["features"].sum() + (out["sdf_grad"] ** 2).sum()).backward()
        assert grid.grad[: 2 * int(geo._meta.offset[6])].any() and not grid.grad[2 * int(geo._meta.offset[6]):].any()


def test_training_smoke_levels_advance_and_masked_levels_get_no_gradient():
    import scaledreamer_amd.plugins  # noqa: F401
    from scaledreamer_amd.registry import find

    geo = _sdf_geometry()
    mat = find("no-material")({"n_output_dims": 3, "color_activation": "sigmoid"})

    class _Solid(torch.nn.Module):
        def forward(self, dirs, **kwargs):
            return torch.full_like(dirs, 0.5)

    ren = find("neus-volume-renderer")({"radius": 1.0, "num_samples_per_ray": 64}, geometry=geo, material=mat, background=_Solid())
    for m in (mat, ren):
        m.cuda().train()
    opt = torch.optim.Adam(geo.parameters(), lr=1e-3)
    ys, xs = torch.meshgrid(torch.linspace(-0.4, 0.4, 8), torch.linspace(-0.4, 0.4, 8), indexing="ij")
    rays_d = torch.nn.functional.normalize(torch.stack([xs, ys, -torch.ones_like(xs)], -1), dim=-1).view(1, 8, 8, 3).cuda()
    rays_o = torch.tensor([0.0, 0.0, 2.0]).expand(1, 8, 8, 3).contiguous().cuda()
    grid = geo.encoding.encoding.encoding.params
    levels = []
    for step in range(5):
        geo.do_update_step(0, step)
        ren.update_step(0, step)
        level = geo.encoding.encoding.current_level
        levels.append(level)
        assert level == 4 + step // 2 and geo._meta.n_masked_levels == 16 - level
        want_eps = 2.0 / (16 * 1.447269237440378 ** (level - 1))
        assert geo.finite_difference_normal_eps == pytest.approx(want_eps, rel=1e-12) and geo._fcfg.fd_eps == pytest.approx(want_eps, rel=1e-6)
        out = ren(rays_o=rays_o, rays_d=rays_d, light_positions=torch.zeros(1, 3, device="cuda"))
        loss = ((out["comp_rgb"] - 0.25) ** 2).mean() + 0.1 * ((out["sdf_grad"].norm(dim=-1) - 1.0) ** 2).mean()
        assert torch.isfinite(loss)
        opt.zero_grad(set_to_none=True)
        loss.backward()
        assert grid.grad is not None and torch.isfinite(grid.grad).all()
        assert grid.grad[: 2 * int(geo._meta.offset[level])].any()
        assert not grid.grad[2 * int(geo._meta.offset[level]):].any(), f"step {step}: a still-masked level received gradient"
        opt.step()
    assert levels == [4, 4, 5, 5, 6]


# ---- goldens made by the reference's own classes (tests/golden/make_goldens_progressive.py) -------------------------------------------------
def test_encoding_module_matches_the_reference_band_encodings():
    import os

    from golden_util import GOLDEN_DIR, grid_params
    from scaledreamer_amd.networks import get_encoding

    g = dict(np.load(os.path.join(GOLDEN_DIR, "progressive_band.npz")))
    band = {**PROG, "start_level": int(g["start_level"]), "start_step": int(g["start_step"]), "update_steps": int(g["update_steps"])}
    x = _dev(g["x"])
    table = torch.from_numpy(grid_params(int(g["seed"]), 12_599_920, float(g["grid_amp"])))
    for a, step in ((0, None), (4, 100), (6, 200), (16, 700)):
        enc = get_encoding(3, band).cuda()
        with torch.no_grad():
            enc.encoding.encoding.params.copy_(table)
            if step is not None:
                enc.do_update_step(0, step)
            got = enc(x).cpu().numpy()
        np.testing.assert_array_equal(got, g["enc_before_update"] if step is None else g[f"enc_{a}"], err_msg=f"{a} levels")


def _neus_d_system(g):
    import json

    import scaledreamer_amd.plugins  # noqa: F401
    from scaledreamer_amd.registry import find
    from test_gpu_neus_golden import BG_ENC

    band = {**PROG, "start_level": int(g["start_level"]), "start_step": int(g["start_step"]), "update_steps": int(g["update_steps"])}
    geo = find("implicit-sdf")({"radius": 1.0, "normal_type": "finite_difference", "finite_difference_normal_eps": "progressive",
                                "pos_encoding_config": band, "sdf_bias": "sphere", "sdf_bias_params": 0.5})
    mat = find("no-material")({"n_output_dims": 3, "color_activation": "sigmoid"})
    bg = find("neural-environment-map-background")({"color_activation": "sigmoid", "random_aug": True, "random_aug_prob": 0.5,
                                                    "dir_encoding_config": BG_ENC})
    ren = find("neus-volume-renderer")({"radius": 1.0, **json.loads(str(g["ren_cfg"]))}, geometry=geo, material=mat, background=bg)
    t = lambda k: torch.from_numpy(g[k])
    geo.load_state_dict({"encoding.encoding.encoding.params": t("grid"), "sdf_network.layers.0.weight": t("w1s"), "sdf_network.layers.2.weight": t("w2s"),
                         "feature_network.layers.0.weight": t("w1f"), "feature_network.layers.2.weight": t("w2f")}, strict=False)
    bg.load_state_dict({"encoding.encoding.encoding.params": t("bgrid"), "network.layers.0.weight": t("bw0"), "network.layers.2.weight": t("bw1"),
                        "network.layers.4.weight": t("bw2")}, strict=False)
    for m in (geo, mat, bg, ren):
        m.cuda().train()
    ren.load_state_dict({"estimator.occs": t("occs"), "estimator.binaries": t("binaries"), "variance._inv_std": t("inv_std_param")}, strict=False)
    step = int(g["step"])
    geo.do_update_step(0, step)
    assert geo.encoding.encoding.current_level == int(g["active_levels"]) == 6 and geo.finite_difference_normal_eps == float(g["fd_eps"])
    assert geo.fused
    ren.cfg.grid_prune, saved = False, ren.cfg.grid_prune          # cos_anneal_ratio of the fixture's step without an occupancy update
    ren.update_step(0, step)
    ren.cfg.grid_prune = saved
    jit = t("jitter").cuda()
    ren.jitter_fn = lambda n, device: jit
    bg.rand_fn = lambda: 0.9
    return geo, mat, bg, ren


_GOLDEN_D = {}


def _golden_d():
    from golden_util import load_renderer_golden

    if not _GOLDEN_D:          # (loaded once: the 12.6 M-entry table comes from its seed rule)
        _GOLDEN_D.update(load_renderer_golden("neus_d_8x8x64_progressive"))
    return _GOLDEN_D


def test_eval_image_is_the_same_on_the_fused_and_the_composed_route(monkeypatch):
    """test_gpu_neus_golden.py::test_eval_image_is_the_same_on_both_routes with the progressive grid and eps: same keys, rtol 2e-5 / atol 1e-5"""
    g = _golden_d()
    dev = lambda k: torch.from_numpy(g[k]).cuda()
    outs = {}
    for route in ("1", "0"):
        monkeypatch.setenv("ASD_NEUS", route)
        geo, mat, bg, ren = _neus_d_system(g)
        ren.eval(); geo.eval(); bg.eval()
        with torch.no_grad():
            outs[route] = ren(rays_o=dev("rays_o"), rays_d=dev("rays_d"), light_positions=dev("light_positions"))
    assert set(outs["0"]) == set(outs["1"])
    for k in outs["0"]:
        torch.testing.assert_close(outs["1"][k], outs["0"][k], rtol=2e-5, atol=1e-5, msg=k)


@pytest.mark.parametrize("route", ["1", "0"], ids=["fused", "composed"])
def test_neus_route_matches_the_reference_with_six_levels(route, monkeypatch):
    """neus_d_8x8x64_progressive.npz: the reference's ImplicitSDF (progressive grid and eps, sphere bias 0.5) + NeuSVolumeRenderer at a step
    with 6 active levels; outputs, kept samples and gradients matched as test_gpu_neus_golden.py matches its fixtures."""
    from test_gpu_neus_golden import reference_loss

    monkeypatch.setenv("ASD_NEUS", route)
    g = _golden_d()
    geo, mat, bg, ren = _neus_d_system(g)
    t = lambda k: torch.from_numpy(g[k])
    dev = lambda k: t(k).cuda()
    out = ren(rays_o=dev("rays_o"), rays_d=dev("rays_d"), light_positions=dev("light_positions"), elevation=None, azimuth=None)
    assert set(out.keys()) == {k[4:] for k in g if k.startswith("out_")}
    cpu = {k: v.detach().cpu().numpy() for k, v in out.items()}
    np.testing.assert_array_equal(cpu["ray_indices"], g["out_ray_indices"])
    for k in ["t_points", "t_intervals", "points", "t_dirs"]:
        np.testing.assert_array_equal(cpu[k], g["out_" + k], err_msg=k)
    for k in ["sdf", "features", "weights", "comp_rgb", "comp_rgb_fg", "comp_rgb_bg", "opacity", "depth", "inv_std"]:
        np.testing.assert_allclose(cpu[k], g["out_" + k], rtol=2e-5, atol=1e-5, err_msg=k)
    np.testing.assert_allclose(cpu["normal"], g["out_normal"], rtol=0, atol=2e-3)
    np.testing.assert_allclose(cpu["sdf_grad"], g["out_sdf_grad"], rtol=0, atol=2e-3)
    loss, loss_eikonal = reference_loss(out, g)
    assert abs(loss.item() - float(g["loss"])) < 2e-4 * max(1.0, abs(float(g["loss"])))
    assert abs(loss_eikonal.item() - float(g["loss_eikonal"])) < 2e-4 * max(1.0, abs(float(g["loss_eikonal"])))
    loss.backward()
    got = {"w1s": geo.sdf_network.layers[0].weight, "w2s": geo.sdf_network.layers[2].weight, "w1f": geo.feature_network.layers[0].weight,
           "w2f": geo.feature_network.layers[2].weight, "bw0": bg.network.layers[0].weight, "bw1": bg.network.layers[2].weight,
           "bw2": bg.network.layers[4].weight, "inv_std_param": ren.variance._inv_std}
    for k, p in got.items():
        ref = g["g_" + k]
        scale = max(float(np.abs(ref).max()), 1e-6)
        np.testing.assert_allclose(p.grad.cpu().numpy() / scale, ref / scale, rtol=0, atol=3e-3, err_msg=k)
    for k in ("w1s", "w1f"):
        assert not got[k].grad[:, 12:].any(), f"columns >= 12 of d_{k} must be exactly 0"
    gg = geo.encoding.encoding.encoding.params.grad.cpu().numpy()
    idx, val = g["g_grid_idx"], g["g_grid_val"]
    np.testing.assert_allclose(gg[idx] / np.abs(val).max(), val / np.abs(val).max(), rtol=0, atol=3e-3)
    assert abs(np.linalg.norm(gg.astype(np.float64)) / float(g["g_grid_l2"]) - 1) < 3e-3
    assert not gg[2 * int(geo._meta.offset[6]):].any()
