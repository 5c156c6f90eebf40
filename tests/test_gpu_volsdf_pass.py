"""The pass-level entries of the importance-sampled VolSDF renderer (include/asd_hip.h: asd_volsdf_*) and the renderer route built on them
(ASD_VOLSDF=1): sampling entries against the oracle and today's torch expressions bit for bit, the compositing pass against a float64
restatement with the composed path's own error as the yardstick, the renderer against the reference's golden and against the composed route
at the bench shape, the fallbacks, guard bands and run-to-run identity."""
import ctypes as C
import math
import os
import random

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
P0 = 0.340119            # the shipped learned_variance_init: a = exp(3.40119) = 30.0


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _load(name):
    return np.load(os.path.join(HERE, "golden", name + ".npz"))


# ---- 1. sampling entries ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stratified", [True, False])
def test_sampling_entries_match_oracle_and_torch_bit_for_bit(stratified):
    from oracle import oracle as O
    from scaledreamer_amd import ops

    rng = np.random.default_rng(5)                     # seeds and shapes of test_importance_resample_cdf_merge_match_oracle
    n_rays, e_in, n_out = 777, 129, 64
    near, far = 0.1, 4.0
    vals = np.sort(rng.uniform(0.1, 4.0, (n_rays, e_in)).astype(np.float32), axis=1)
    sig = (rng.uniform(0, 1, (n_rays, e_in - 1)) ** 6 * 60).astype(np.float32)
    sig[:5] = 0.0
    cdf_o = O.transmittance_cdf(vals, sig)
    jit = rng.uniform(0, 1, n_rays).astype(np.float32) if stratified else None
    s_o = O.importance_resample(vals, cdf_o, n_out, jit)
    s, t = ops.volsdf_edges(_dev(vals), _dev(cdf_o), n_out, None if jit is None else _dev(jit), near, far)
    np.testing.assert_array_equal(s.cpu().numpy(), s_o)
    np.testing.assert_array_equal(t.cpu().numpy(), s_o * np.float32(far) + (np.float32(1) - s_o) * np.float32(near))
    _, t_only = ops.volsdf_edges(_dev(vals), _dev(cdf_o), n_out, None if jit is None else _dev(jit), near, far, want_s=False)
    assert _ is None and torch.equal(t_only, t)

    # asd_volsdf_samples against the torch expressions of the composed _render, on the same device tensors
    ro = _dev(rng.normal(size=(n_rays, 3)).astype(np.float32))
    rd = F.normalize(_dev(rng.normal(size=(n_rays, 3)).astype(np.float32)), dim=-1).contiguous()
    edges = _dev(vals)
    S = e_in - 1
    points, t_dirs, t_mid, t_len, ray_idx = ops.volsdf_samples(ro, rd, edges)
    t0, t1 = edges[:, :-1], edges[:, 1:]
    ray_indices = torch.arange(n_rays, device="cuda").repeat_interleave(S)
    t0f, t1f = t0.reshape(-1).contiguous(), t1.reshape(-1).contiguous()
    want_mid, want_len = ((t0f + t1f) * 0.5)[:, None], (t1f - t0f)[:, None]
    want_dirs = rd[ray_indices]
    want_pos = ro[ray_indices] + want_dirs * want_mid
    for got, want in ((points, want_pos), (t_dirs, want_dirs), (t_mid, want_mid), (t_len, want_len), (ray_idx, ray_indices)):
        assert got.shape == want.shape and got.dtype == want.dtype
        assert torch.equal(got, want)
    mid = ro[:, None, :] + rd[:, None, :] * ((t0 + t1) * 0.5)[..., None]           # the proposal mid-points of _intervals
    assert torch.equal(ops.volsdf_samples(ro, rd, edges, everything=False), mid.reshape(-1, 3))

    # asd_volsdf_proposal_cdf against the oracle's density + cdf
    sdf = rng.uniform(-0.5, 1.0, (n_rays, S)).astype(np.float32)
    sdf[:5] = np.abs(sdf[:5]) + 0.3
    sdf[5, :7] = 0.0
    p = torch.tensor(P0, device="cuda")
    a = float(torch.exp(p * 10.0))
    cdf = ops.volsdf_proposal_cdf(_dev(sdf), edges, p).cpu().numpy()
    np.testing.assert_allclose(cdf, O.transmittance_cdf(vals, O.volsdf_density(sdf, a)), rtol=0, atol=3e-7)
    assert (cdf[:, -1] == 1.0).all() and (cdf[:, 0] == 0.0).all()


# ---- 2. the compositing pass against float64 ----------------------------------------------------------------------------------------------
def _sampler_like_edges(n_rays, rng):
    """[n_rays, 194] edges built like the real sampler's: 129 jittered uniform edges on [0.1, 4.0] merged with 65 edges inside [1.27, 2.05]"""
    jit = rng.uniform(0, 1, (n_rays, 1))
    coarse = 0.1 + 3.9 * (np.arange(129)[None, :] + jit) / 129.0
    fine = rng.uniform(1.27, 2.05, (n_rays, 65))
    return np.sort(np.concatenate([coarse, fine], axis=1), axis=1).astype(np.float32)


def _composite_case(S, with_normal, seed=7):
    rng = np.random.default_rng(seed + S)
    n_rays = 777
    full = _sampler_like_edges(n_rays, rng)
    start = (full.shape[1] - (S + 1)) // 2                       # a window of S + 1 consecutive edges (the fine region sits in the middle)
    edges = np.ascontiguousarray(full[:, start:start + S + 1])
    assert float(np.abs(np.diff(edges, axis=1)).max()) * math.exp(10 * P0) < 1.0       # alpha < 1: the regime the shipped configs run in
    sdf = rng.uniform(-0.5, 1.0, (n_rays * S, 1)).astype(np.float32)
    sdf[:50 * S] = np.abs(sdf[:50 * S]) + 0.3                    # empty rays: opacity ~ 1e-4
    feats = rng.normal(size=(n_rays * S, 3)).astype(np.float32)
    nrm = rng.normal(size=(n_rays * S, 3))
    nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32)
    bg = rng.uniform(0, 1, (n_rays, 3)).astype(np.float32)
    ups = {"weights": (n_rays * S,), "opacity": (n_rays,), "depth": (n_rays,), "rgb_fg": (n_rays, 3), "z_var": (n_rays,), "comp_rgb": (n_rays, 3)}
    if with_normal:
        ups["comp_normal"] = (n_rays, 3)
    ups = {k: rng.normal(size=sh).astype(np.float32) for k, sh in ups.items()}
    return dict(n_rays=n_rays, S=S, edges=edges, sdf=sdf, feats=feats, normal=nrm if with_normal else None, bg=bg, ups=ups)


def _chain(c, color_act, trainable, route):
    """the chain density -> alpha -> running product -> the accumulations -> comp_normal, and its gradients under the case's upstream gradients.
    route "ref": float64 torch, written out from the formulas; "composed": the ASD_VOLSDF=0 code (torch get_alpha + nerfacc_api.composite mode 2 + the
    second normal pass); "fused": asd_volsdf_composite_fwd / _bwd through the renderer's autograd node."""
    from scaledreamer_amd import volsdf_renderer as VR

    dt_ = torch.float64 if route == "ref" else torch.float32
    n_rays, S = c["n_rays"], c["S"]
    leaf = lambda a: _dev(a).to(dt_).requires_grad_(True)
    sdf, feats, bg = leaf(c["sdf"]), leaf(c["feats"]), leaf(c["bg"])
    edges = _dev(c["edges"]).to(dt_)
    normal = None if c["normal"] is None else _dev(c["normal"]).to(dt_)
    var = VR.LearnedVariance(P0, requires_grad=trainable).cuda().to(dt_)
    p = var._inv_std
    t0, t1 = edges[:, :-1].reshape(-1).contiguous(), edges[:, 1:].reshape(-1).contiguous()
    if route == "fused":
        w, op, dp, fg, zv, comp, cn = VR._VolSDFCompositeFn.apply(sdf, feats, bg, p, normal, edges, color_act)
    elif route == "composed":
        alpha = ((t1 - t0)[:, None].abs() * VR.volsdf_density(sdf, var(sdf)))[:, 0]
        rgb = torch.sigmoid(feats) if color_act == 1 else feats
        w, op, dp, fg, zv, comp, cn = VR.GenerativeSpaceVolSDFVolumeRenderer._composite(alpha, rgb, bg, t0, t1, normal, n_rays, S)
    else:
        a = torch.exp(p * 10.0).clamp(1.0e-6, 1.0e6).clamp(0.0, 80.0)
        sigma = a * (0.5 + 0.5 * sdf.sign() * torch.expm1(-sdf.abs() * a))
        alpha = ((t1 - t0)[:, None].abs() * sigma).reshape(n_rays, S)
        T = torch.cumprod(torch.cat([torch.ones_like(alpha[:, :1]), 1.0 - alpha[:, :-1]], dim=1), dim=1)
        wr = T * alpha
        tm = ((t0 + t1) * 0.5).reshape(n_rays, S)
        col = (torch.sigmoid(feats) if color_act == 1 else feats).reshape(n_rays, S, 3)
        op, dp = wr.sum(1), (wr * tm).sum(1)
        fg = (wr[..., None] * col).sum(1)
        zv = (wr * (tm - dp[:, None]) ** 2).sum(1)
        comp = fg + bg * (1.0 - op[:, None])
        cn = None
        if normal is not None:
            acc = (wr.detach()[..., None] * normal.reshape(n_rays, S, 3)).sum(1)
            cn = (acc / acc.norm(dim=-1, keepdim=True).clamp_min(1e-12) + 1.0) * 0.5 * op[:, None]
        w = wr.reshape(-1)
    outs = {"weights": w, "opacity": op, "depth": dp, "rgb_fg": fg, "z_var": zv, "comp_rgb": comp}
    if cn is not None:
        outs["comp_normal"] = cn
    loss = sum((outs[k] * _dev(c["ups"][k]).to(dt_)).sum() for k in outs)
    loss.backward()
    res = {k: v.detach().double() for k, v in outs.items()}
    res.update(d_sdf=sdf.grad.double(), d_features=feats.grad.double(), d_bg=bg.grad.double())
    if trainable:
        res["d_p"] = p.grad.double().reshape(1)
    else:
        assert p.grad is None
    return res


@pytest.mark.parametrize("trainable", [True, False], ids=["variance-trainable", "variance-frozen"])
@pytest.mark.parametrize("with_normal", [True, False], ids=["normal", "no-normal"])
@pytest.mark.parametrize("color_act", [0, 1], ids=["colours", "sigmoid"])
@pytest.mark.parametrize("S", [1, 64, 65, 193])
def test_compositing_pass_against_float64(S, color_act, with_normal, trainable):
    """Bound per output and gradient: e_fused <= 4 e_composed + 2e-6 max|ref|, e_* the largest error against float64 — the composed route's own
    error measured on the same inputs is the yardstick (two fp32 orderings of this chain differ from float64 by 3e-7 .. 6e-6 of max|ref| and from
    each other by a factor ~1; 4x leaves room for the device's expf / expm1f, the floor covers an output where the composed route lands within an ulp)."""
    c = _composite_case(S, with_normal)
    ref = _chain(c, color_act, trainable, "ref")
    composed = _chain(c, color_act, trainable, "composed")
    fused = _chain(c, color_act, trainable, "fused")
    assert set(fused) == set(ref) == set(composed)
    bad = []
    for k in ref:
        assert fused[k].shape == ref[k].shape and torch.isfinite(fused[k]).all(), k
        scale = float(ref[k].abs().max())
        e_f, e_c = float((fused[k] - ref[k]).abs().max()), float((composed[k] - ref[k]).abs().max())
        bound = 4.0 * e_c + 2e-6 * scale
        print(f"S={S:<3d} act={color_act} normal={int(with_normal)} trainable={int(trainable)} {k:<11s} max|ref|={scale:.3e} e_fused={e_f:.3e} "
              f"e_composed={e_c:.3e} bound={bound:.3e}")
        if not e_f <= bound:
            bad.append(k)
    assert not bad, bad


def _both_forward_kernels(S, color_act):
    """(asd_volsdf_composite_fwd, asd_neus_composite_fwd with use_volsdf) on five dense rays of _composite_case: two empty ones and three
    that meet the surface; five rays are two blocks, the second with a single ray"""
    from scaledreamer_amd import ops

    c = _composite_case(S, True)
    rays, n = slice(48, 53), 5
    per_ray = lambda a: _dev(a.reshape(c["n_rays"], S, -1)[rays].reshape(n * S, -1))
    sdf, feats, nrm = per_ray(c["sdf"]).reshape(-1), per_ray(c["feats"]), per_ray(c["normal"])
    edges, bg, p = _dev(c["edges"][rays]), _dev(c["bg"][rays]), torch.tensor(P0, device="cuda")
    dense = ops.volsdf_composite_fwd(sdf, feats, nrm, edges, p, bg, color_act)
    offset = torch.arange(n, device="cuda", dtype=torch.int32) * S
    count = torch.full((n,), S, device="cuda", dtype=torch.int32)
    t0, t1 = edges[:, :-1].reshape(-1).contiguous(), edges[:, 1:].reshape(-1).contiguous()
    packed = ops.neus_composite_fwd(sdf, nrm, nrm, t0, t1, feats, color_act, p, 1.0, True, bg, offset, count, want_comp_normal=True)     # (VolSDF reads no directions)
    return dense, packed


@pytest.mark.parametrize("color_act", [0, 1], ids=["colours", "sigmoid"])
@pytest.mark.parametrize("S", [1, 64, 65, 193])
def test_dense_and_packed_forward_kernels_agree_bit_for_bit(S, color_act):
    """The VolSDF branch of asd_neus_composite_fwd and asd_volsdf_composite_fwd are the same operations in the same order (the variance, the
    density, the transmittance step, the accumulations and the normal image are one definition each, csrc/ray_composite.h): on dense rays every
    output they share is equal in every bit.  S: one lane, a full trip, a trip and one lane, a ragged fourth trip."""
    dense, packed = _both_forward_kernels(S, color_act)
    assert float(dense["weights"].abs().max()) > 0.0
    for k in ("weights", "opacity", "depth", "rgb_fg", "comp_rgb", "comp_normal"):
        assert packed[k].shape == dense[k].shape, k
        assert torch.equal(packed[k].view(torch.int32), dense[k].view(torch.int32)), k


# ---- 3. the renderer against the reference's golden ---------------------------------------------------------------------------------------
_ENC = {"otype": "HashGrid", "n_levels": 16, "n_features_per_level": 2, "log2_hashmap_size": 19, "base_resolution": 16, "per_level_scale": 1.447269237440378}
_HYPER = {"c_dim": 1024, "out_dims": {"sdf_weights": [64, 1], "feature_weights": [64, 3]}, "spectral_norm": False, "n_neurons": 64, "n_hidden_layers": 1}


def _hyper_ingp_renderer(n_fine, n_prop, trainable=False, material=None, **ren_kw):
    import scaledreamer_amd.plugins  # noqa: F401
    from scaledreamer_amd.registry import find

    geo = find("Hyper-iNGP")({"radius": 2.0, "normal_type": "finite_difference", "finite_difference_normal_eps": 0.01, "sdf_bias": "sphere",
                              "sdf_bias_params": 0.5, "shape_init": "sphere", "shape_init_params": 0.5, "hypernet_config": _HYPER,
                              "pos_encoding_config": _ENC}).cuda()
    mat = find("no-material")(material or {"n_output_dims": 3, "color_activation": "sigmoid", "requires_normal": True}).cuda()
    bg = find("multiprompt-neural-hashgrid-environment-map-background")(
        {"color_activation": "sigmoid", "random_aug": True, "random_aug_prob": 0.2, "pos_encoding_config": dict(_ENC, per_level_scale=1.0)}).cuda()
    ren = find("generative-space-volsdf-volume-renderer")(
        dict({"radius": 2.0, "use_volsdf": True, "trainable_variance": trainable, "learned_variance_init": P0, "estimator": "importance",
              "num_samples_per_ray": n_fine, "num_samples_per_ray_importance": n_prop, "near_plane": 0.1, "far_plane": 4.0, "train_chunk_size": 0}, **ren_kw),
        geometry=geo, material=mat, background=bg).cuda()
    geo.do_update_step(0, 0)
    assert geo._fcfg is not None
    return ren, geo, mat, bg


def _count_pass_level_calls(monkeypatch):
    from scaledreamer_amd import ops

    calls = {"n": 0}
    real = ops.volsdf_composite_fwd

    def counted(*a, **kw):
        calls["n"] += 1
        return real(*a, **kw)

    monkeypatch.setattr(ops, "volsdf_composite_fwd", counted)
    return calls


@pytest.mark.parametrize("route", ["1", "0"], ids=["pass-level", "composed"])
def test_hyper_ingp_volsdf_renderer_matches_reference_golden_on_both_routes(route, monkeypatch):
    from test_goldens_amortized_cpu import amortized_loss, amortized_problem, check_amortized_against_golden

    monkeypatch.setenv("ASD_VOLSDF", route)
    calls = _count_pass_level_calls(monkeypatch)
    g = _load("amortized_hyper_ingp_2x4x4")
    P = amortized_problem(g)
    ren, geo, mat, bg = _hyper_ingp_renderer(int(g["n_fine"]), int(g["n_prop"]))
    with torch.no_grad():
        geo.encoding.encoding.encoding.params.copy_(P["grid"].detach())
        bg.encoding.encoding.encoding.params.copy_(P["bgrid"].detach())
        for tag, net in (("geo_hyper", geo.hypernet), ("bg_hyper", bg.hypernet)):
            for k, p in net.named_parameters():
                p.copy_(P[tag][k].detach())
    jit = [_dev(g["jitter0"]), _dev(g["jitter1"])]
    ren.estimator.jitter_fn = lambda n, device: jit.pop(0)
    real = random.random
    random.random = lambda: 0.9
    try:
        ren.train(); geo.train(); bg.train(); mat.train()
        out = ren(rays_o=_dev(g["rays_o"]), rays_d=_dev(g["rays_d"]), light_positions=_dev(g["light_positions"]), text_embed=_dev(g["text_embed"]))
    finally:
        random.random = real
    assert calls["n"] == (1 if route == "1" else 0)
    loss, loss_eik = amortized_loss(out, g)
    loss.backward()
    Pg = {"grid": geo.encoding.encoding.encoding.params, "bgrid": bg.encoding.encoding.encoding.params,
          "geo_hyper": dict(geo.hypernet.named_parameters()), "bg_hyper": dict(bg.hypernet.named_parameters())}
    check_amortized_against_golden(out, Pg, g, loss, loss_eik, tol=2.0)
    assert abs(float(out["inv_std"]) - 30.0) < 1e-2


# ---- 4. pass-level against composed at the bench shape ------------------------------------------------------------------------------------
def _camera_rays(V, H, W, seed):
    """pinhole rays from a camera on the sphere of radius 1.25 looking at the origin, [V, H, W, 3]"""
    g = torch.Generator().manual_seed(seed)
    eye = F.normalize(torch.randn(V, 3, generator=g), dim=-1) * 1.25
    fwd = F.normalize(-eye, dim=-1)
    right = F.normalize(torch.cross(fwd, torch.tensor([[0.0, 0.0, 1.0]]).expand(V, -1), dim=-1), dim=-1)
    up = torch.cross(right, fwd, dim=-1)
    ys, xs = torch.meshgrid((torch.arange(H) + 0.5) / H - 0.5, (torch.arange(W) + 0.5) / W - 0.5, indexing="ij")
    d = fwd[:, None, None, :] + 0.9 * xs[None, :, :, None] * right[:, None, None, :] - 0.9 * ys[None, :, :, None] * up[:, None, None, :]
    return eye[:, None, None, :].expand(V, H, W, 3).contiguous().cuda(), F.normalize(d, dim=-1).contiguous().cuda()


_IMAGE_KEYS = ("comp_rgb", "comp_rgb_fg", "comp_rgb_bg", "opacity", "depth", "z_variance", "comp_normal")
_EXACT_KEYS = ("t_points", "t_intervals", "t_dirs", "ray_indices", "points")
_rel = lambda a, b: float((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-20))


@pytest.mark.parametrize("trainable", [True, False], ids=["variance-trainable", "variance-frozen"])
def test_pass_level_route_matches_composed_route_at_the_bench_shape(trainable, monkeypatch):
    """Hyper-iNGP, no-material, hypernetwork background, 1 x 64 x 64 rays, 128 + 64 samples, the same injected jitter on both routes.  Tolerances:
    those of _fused_vs_composed in test_gpu_amortized.py (2e-5 of the maximum for plain outputs, 2e-3 for normal / sdf_grad and for gradients
    that pass the finite differences and the atomic scatter)."""
    torch.manual_seed(11)
    ren, geo, mat, bg = _hyper_ingp_renderer(64, 128, trainable=trainable, eval_chunk_size=100000)
    V, H, W = 1, 64, 64
    rays_o, rays_d = _camera_rays(V, H, W, 3)
    gen = torch.Generator().manual_seed(4)
    text = torch.randn(V, 1024, generator=gen).cuda()
    light = torch.randn(V, 3, generator=gen).cuda()
    jitters = [torch.rand(V * H * W, generator=gen).cuda() for _ in range(2)]
    params = {"grid": geo.encoding.encoding.encoding.params, "bgrid": bg.encoding.encoding.encoding.params,
              **{"geo_hyper." + k: p for k, p in geo.hypernet.named_parameters()}, **{"bg_hyper." + k: p for k, p in bg.hypernet.named_parameters()}}
    if trainable:
        params["_inv_std"] = ren.variance._inv_std
    ups = {}
    calls = _count_pass_level_calls(monkeypatch)

    def run(route, train):
        monkeypatch.setenv("ASD_VOLSDF", route)
        for p in params.values():
            p.grad = None
        jit = list(jitters)
        ren.estimator.jitter_fn = lambda n, device: jit.pop(0)
        real = random.random
        random.random = lambda: 0.9
        try:
            if train:
                ren.train(); geo.train(); bg.train(); mat.train()
                out = ren(rays_o=rays_o, rays_d=rays_d, light_positions=light, text_embed=text)
            else:
                ren.eval(); bg.eval(); mat.eval()
                with torch.no_grad():
                    return ren(rays_o=rays_o, rays_d=rays_d, light_positions=light, text_embed=text), None
        finally:
            random.random = real
        loss = 0.0
        for k in _IMAGE_KEYS + ("weights", "sdf", "sdf_grad", "features", "normal"):
            if k not in ups:
                ups[k] = torch.randn(out[k].shape, generator=gen).cuda() * (1.0 if k in _IMAGE_KEYS else 1e-2)
            loss = loss + (out[k] * ups[k]).sum()
        loss.backward()
        return {k: v.detach() for k, v in out.items()}, {k: p.grad.clone() for k, p in params.items() if p.grad is not None}

    n0 = calls["n"]
    o1, g1 = run("1", True)
    assert calls["n"] == n0 + 1
    o0, g0 = run("0", True)
    assert calls["n"] == n0 + 1
    assert set(o1) == set(o0) and "t_light" not in o1
    for k in o0:
        assert o1[k].shape == o0[k].shape and o1[k].dtype == o0[k].dtype, k
    assert o0["points"].shape == (V * H * W * 193, 3)
    for k in _EXACT_KEYS:
        assert torch.equal(o1[k], o0[k]), k
    for k in o0:
        if k in _EXACT_KEYS:
            continue
        tol = 2e-3 if k in ("normal", "shading_normal", "sdf_grad") else 2e-5
        r = _rel(o1[k], o0[k])
        print(f"train output {k:<14s} pass-level vs composed: {r:.2e} of the maximum (bound {tol:.0e})")
        assert r < tol, k
    assert set(g1) == set(g0) and len(g0) >= 4 + int(trainable)
    for k in g0:
        r = _rel(g1[k], g0[k])
        print(f"gradient {k:<28s} pass-level vs composed: {r:.2e} of the maximum (bound 2e-3)")
        assert r < 2e-3, k
    # evaluation: no jitter, the field in chunks of 100 000 of the 790 528 samples
    e1, _ = run("1", False)
    assert calls["n"] == n0 + 2
    e0, _ = run("0", False)
    assert calls["n"] == n0 + 2
    assert set(e1) == set(e0) == set(_IMAGE_KEYS)
    for k in _IMAGE_KEYS:
        assert e1[k].shape == e0[k].shape and e1[k].dtype == e0[k].dtype, k
        r = _rel(e1[k], e0[k])
        print(f"eval output {k:<14s} pass-level vs composed: {r:.2e} of the maximum (bound 2e-5)")
        assert r < 2e-5, k


# ---- 5. fallbacks -------------------------------------------------------------------------------------------------------------------------
def test_ineligible_configurations_take_the_composed_route_unchanged(monkeypatch):
    calls = _count_pass_level_calls(monkeypatch)
    V, H, W = 1, 8, 8
    rays_o, rays_d = _camera_rays(V, H, W, 5)
    gen = torch.Generator().manual_seed(6)
    text, light = torch.randn(V, 1024, generator=gen).cuda(), torch.randn(V, 3, generator=gen).cuda()
    jitters = [torch.rand(V * H * W, generator=gen).cuda() for _ in range(2)]

    def render(ren, ro, rd):
        jit = list(jitters)
        ren.estimator.jitter_fn = lambda n, device: jit.pop(0).to(device)
        real = random.random
        random.random = lambda: 0.9
        try:
            ren.train()
            with torch.no_grad():
                return ren(rays_o=ro, rays_d=rd, light_positions=light.to(ro.device), text_embed=text.to(ro.device))
        finally:
            random.random = real

    # a colour MLP behind the features: the material's own forward has to run
    torch.manual_seed(2)
    mlp = {"n_output_dims": 3, "color_activation": "sigmoid", "input_feature_dims": 3,
           "mlp_network_config": {"otype": "VanillaMLP", "activation": "ReLU", "n_neurons": 16, "n_hidden_layers": 1}}
    ren = _hyper_ingp_renderer(16, 32, material=mlp)[0]
    assert not ren.material.elementwise
    monkeypatch.setenv("ASD_VOLSDF", "1")
    a = render(ren, rays_o, rays_d)
    monkeypatch.setenv("ASD_VOLSDF", "0")
    b = render(ren, rays_o, rays_d)
    assert calls["n"] == 0 and set(a) == set(b)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    # the pass-level route itself, for the record: an eligible material on the same rays does take it
    monkeypatch.setenv("ASD_VOLSDF", "1")
    ren2 = _hyper_ingp_renderer(16, 32)[0]
    render(ren2, rays_o, rays_d)
    assert calls["n"] == 1
    # CPU rays: whatever the composed route answers today (the HIP path has no CPU fallback), unchanged by the switch
    def outcome(ro, rd):
        try:
            return ("ok", render(ren2, ro, rd))
        except Exception as e:          # noqa: BLE001 - the point is that both settings end the same way
            return ("raised", type(e), str(e))

    monkeypatch.setenv("ASD_VOLSDF", "0")
    want = outcome(rays_o.cpu(), rays_d.cpu())
    monkeypatch.setenv("ASD_VOLSDF", "1")
    got = outcome(rays_o.cpu(), rays_d.cpu())
    assert calls["n"] == 1 and got[0] == want[0]
    if want[0] == "raised":
        assert got[1:] == want[1:]
    else:
        assert set(got[1]) == set(want[1]) and all(torch.equal(got[1][k], want[1][k]) for k in want[1])
    # use_volsdf=False raises what it raises on the composed route
    ren3 = _hyper_ingp_renderer(16, 32, use_volsdf=False)[0]
    for route in ("1", "0"):
        monkeypatch.setenv("ASD_VOLSDF", route)
        with pytest.raises(ValueError, match="only VolSDF supports importance sampling"):
            render(ren3, rays_o, rays_d)
    assert calls["n"] == 1


# ---- 6. memory safety and run-to-run identity ---------------------------------------------------------------------------------------------
GUARD = 1 << 16


def _guarded(nbytes: int):
    buf = torch.full((nbytes + 2 * GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    return buf, buf[GUARD:GUARD + nbytes]


def _intact(buf, nbytes):
    return bool((buf[:GUARD] == 0xA5).all()) and bool((buf[GUARD + nbytes:] == 0xA5).all())


@pytest.mark.parametrize("S", [193, 1])
def test_entries_stay_inside_their_outputs_and_repeat_bit_for_bit(S):
    from scaledreamer_amd import _lib

    L, n_rays = _lib.lib(), 777                     # (not a multiple of the four rays a block holds)
    c = _composite_case(S, True)
    n = n_rays * S
    rng = np.random.default_rng(3)
    ro, rd = _dev(rng.normal(size=(n_rays, 3)).astype(np.float32)), _dev(rng.normal(size=(n_rays, 3)).astype(np.float32))
    edges, sdf, feats, nrm, bg = _dev(c["edges"]), _dev(c["sdf"]), _dev(c["feats"]), _dev(c["normal"]), _dev(c["bg"])
    ups = {k: _dev(v) for k, v in c["ups"].items()}
    p = torch.tensor(P0, device="cuda")
    jit = _dev(rng.uniform(0, 1, n_rays).astype(np.float32))
    i32, f32, ptr, st = _lib.i32, _lib.f32, _lib.ptr, _lib.stream()
    bufs = {}

    def out(name, elems, width=4):
        bufs[name] = (*_guarded(elems * width), elems * width)
        return C.c_void_p(bufs[name][1].data_ptr())

    def view(name, dtype=torch.float32):
        return bufs[name][1].view(dtype).clone()

    def check_all(entry):
        torch.cuda.synchronize()
        for name, (buf, _, nbytes) in bufs.items():
            assert _intact(buf, nbytes), f"{entry} wrote outside `{name}`"

    def run_all():
        bufs.clear()
        unit = torch.tensor([0.0, 1.0], device="cuda").repeat(n_rays, 1)
        _lib.check(L.asd_volsdf_edges(ptr(unit), ptr(unit), i32(n_rays), i32(2), i32(S), ptr(jit), f32(0.1), f32(4.0), out("s_edges", n_rays * (S + 1)),
                                      out("t_edges", n_rays * (S + 1)), st))
        check_all("asd_volsdf_edges")
        _lib.check(L.asd_volsdf_samples(ptr(ro), ptr(rd), ptr(edges), i32(n_rays), i32(S), out("points", n * 3), out("t_dirs", n * 3), out("t_mid", n),
                                        out("t_len", n), out("ray_idx", n, 8), st))
        check_all("asd_volsdf_samples")
        _lib.check(L.asd_volsdf_proposal_cdf(ptr(sdf), ptr(edges), ptr(p), i32(n_rays), i32(S), out("cdf", n_rays * (S + 1)), st))
        check_all("asd_volsdf_proposal_cdf")
        _lib.check(L.asd_volsdf_composite_fwd(ptr(sdf), ptr(feats), i32(1), ptr(nrm), ptr(edges), ptr(p), ptr(bg), i32(n_rays), i32(S), out("weights", n),
                                              out("opacity", n_rays), out("depth", n_rays), out("rgb_fg", n_rays * 3), out("z_var", n_rays),
                                              out("comp_rgb", n_rays * 3), out("comp_normal", n_rays * 3), st))
        check_all("asd_volsdf_composite_fwd")
        w, op, dp = (C.c_void_p(bufs[k][1].data_ptr()) for k in ("weights", "opacity", "depth"))
        _lib.check(L.asd_volsdf_composite_bwd(ptr(sdf), ptr(feats), i32(1), ptr(nrm), ptr(edges), ptr(p), ptr(bg), i32(n_rays), i32(S), w, op, dp,
                                              ptr(ups["comp_rgb"]), ptr(ups["rgb_fg"]), ptr(ups["opacity"]), ptr(ups["depth"]), ptr(ups["z_var"]),
                                              ptr(ups["weights"]), ptr(ups["comp_normal"]), out("d_sdf", n), out("d_features", n * 3), out("d_bg", n_rays * 3),
                                              out("d_p", 1), out("dp_partial", n_rays), st))
        check_all("asd_volsdf_composite_bwd")
        return {k: view(k, torch.int64 if k == "ray_idx" else torch.float32) for k in bufs}

    first, second = run_all(), run_all()
    for k in first:
        assert not (first[k].view(torch.uint8) == 0xA5).all(), f"`{k}` was never written"
        if first[k].dtype == torch.float32:
            assert torch.isfinite(first[k]).all(), k
        assert torch.equal(first[k], second[k]), f"`{k}` differs between two runs on the same inputs"
    assert (first["ray_idx"].view(n_rays, S) == torch.arange(n_rays, device="cuda")[:, None]).all()
