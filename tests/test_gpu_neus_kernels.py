"""The NeuS entries (include/asd_hip.h: asd_neus_*) on the device: the compositing pass and its backward against float64 tensor-op autograd
written here, the pruning pass against the step alpha plus the float64 visibility rule, guard bands and run-to-run identity."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

P0 = 0.3                                     # learned_variance_init: a = exp(3) = 20.09
COUNTS = [0, 1, 2, 63, 64, 65, 130]          # empty, one lane, two, one short of a trip, a trip, one over, two trips and a bit


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _case(counts=COUNTS, seed=0, special=True):
    """packed rays: per ray increasing t, an sdf that crosses the surface, unit normals and directions.  With `special`, three built samples:
    the middle sample of the 65-ray has an sdf so negative that both logistic cdfs underflow (NeuS alpha clips to exactly 1, in fp32 and in
    float64); one sample of the 63-ray has t_end < t_start (next cdf above prev: the ratio is negative, alpha clips to 0); one sample of the
    130-ray has sdf == 0."""
    rng = np.random.default_rng(seed)
    counts = np.asarray(counts, np.int32)
    offset = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.int32)
    n, nr = int(counts.sum()), len(counts)
    t0, t1, sdf, dirs = np.zeros(n, np.float32), np.zeros(n, np.float32), np.zeros(n, np.float32), np.zeros((n, 3), np.float32)
    for r, (b, c) in enumerate(zip(offset, counts)):
        if c == 0:
            continue
        step = 1.6 / max(int(c), 8)
        t0[b:b + c] = 0.4 + step * (np.arange(c) + rng.uniform(0, 1))
        t1[b:b + c] = t0[b:b + c] + step * rng.uniform(0.5, 1.0, c)
        sdf[b:b + c] = np.linspace(0.5, -0.3, c) + rng.normal(0, 0.03, c)
        d = rng.normal(size=3)
        dirs[b:b + c] = d / np.linalg.norm(d)
    normal = rng.normal(size=(n, 3))
    normal = (normal / np.linalg.norm(normal, axis=1, keepdims=True)).astype(np.float32)
    if special:
        at = {int(c): int(b) for b, c in zip(offset, counts)}
        sdf[at[65] + 32] = -50.0
        i = at[63] + 40
        t1[i] = t0[i] - 0.05
        normal[i] = -0.8 * dirs[i] + 0.6 * np.cross(dirs[i], [0.0, 0.0, 1.0]) / np.linalg.norm(np.cross(dirs[i], [0.0, 0.0, 1.0]))
        sdf[i] = 0.01
        sdf[at[130] + 70] = 0.0
    feats = rng.normal(size=(n, 3)).astype(np.float32)
    bg = rng.uniform(0, 1, (nr, 3)).astype(np.float32)
    ups = {k: rng.normal(size=sh).astype(np.float32) for k, sh in
           {"weights": (n,), "opacity": (nr,), "depth": (nr,), "rgb_fg": (nr, 3), "comp_rgb": (nr, 3)}.items()}
    return dict(n=n, n_rays=nr, counts=counts, offset=offset, t0=t0, t1=t1, sdf=sdf, dirs=dirs, normal=normal, feats=feats, bg=bg, ups=ups)


def _alpha_ops(sdf, normal, dirs, dt, a, k, use_volsdf):
    """get_alpha (neus_volume_renderer.py:93-117) in the dtype of its arguments; sdf, dt [n]"""
    if use_volsdf:
        a = a.clamp(0.0, 80.0)
        return dt.abs() * (a * (0.5 + 0.5 * sdf.sign() * torch.expm1(-sdf.abs() / (1 / a))))
    true_cos = (dirs * normal).sum(-1)
    iter_cos = -(F.relu(-true_cos * 0.5 + 0.5) * (1.0 - k) + F.relu(-true_cos) * k)
    prev = torch.sigmoid((sdf - iter_cos * dt * 0.5) * a)
    nxt = torch.sigmoid((sdf + iter_cos * dt * 0.5) * a)
    return ((prev - nxt + 1e-5) / (prev + 1e-5)).clip(0.0, 1.0)


def _chain(c, use_volsdf, k, color_act, trainable, route):
    """route "ref": float64 tensor ops + autograd; "composed": the same tensor ops in fp32 on the same device; "fused": asd_neus_composite_fwd /
    _bwd through the renderer's autograd node"""
    from scaledreamer_amd.neus_renderer import _NeuSCompositeFn
    from scaledreamer_amd.volsdf_renderer import LearnedVariance

    dt_ = torch.float64 if route == "ref" else torch.float32
    leaf = lambda a: _dev(a).to(dt_).requires_grad_(True)
    sdf, normal, feats, bg = leaf(c["sdf"]), leaf(c["normal"]), leaf(c["feats"]), leaf(c["bg"])
    dirs, t0, t1 = _dev(c["dirs"]).to(dt_), _dev(c["t0"]).to(dt_), _dev(c["t1"]).to(dt_)
    var = LearnedVariance(P0, requires_grad=trainable).cuda().to(dt_)
    p = var._inv_std
    if route == "fused":
        w, op, dp, fg, comp, _ = _NeuSCompositeFn.apply(sdf, normal, feats, bg, p, dirs, t0, t1, _dev(c["offset"]), _dev(c["counts"]), color_act,
                                                        float(k), bool(use_volsdf), False)
    else:
        a = torch.exp(p * 10.0).clamp(1.0e-6, 1.0e6)
        alpha = _alpha_ops(sdf, normal, dirs, t1 - t0, a, k, use_volsdf)
        col = torch.sigmoid(feats) if color_act == 1 else feats
        tm = (t0 + t1) / 2.0
        ws, ops_, dps, fgs = [], [], [], []
        for b, cnt in zip(c["offset"], c["counts"]):
            al = alpha[b:b + cnt]
            T = torch.cumprod(torch.cat([torch.ones_like(al[:1]), 1.0 - al[:-1]]), dim=0) if cnt > 0 else al
            wr = T * al
            ws.append(wr)
            ops_.append(wr.sum())
            dps.append((wr * tm[b:b + cnt]).sum())
            fgs.append((wr[:, None] * col[b:b + cnt]).sum(0))
        w, op, dp, fg = torch.cat(ws), torch.stack(ops_), torch.stack(dps), torch.stack(fgs)
        comp = fg + bg * (1.0 - op[:, None])
    outs = {"weights": w, "opacity": op, "depth": dp, "rgb_fg": fg, "comp_rgb": comp}
    loss = sum((outs[name] * _dev(c["ups"][name]).to(dt_)).sum() for name in outs)
    loss.backward()
    res = {name: v.detach().double() for name, v in outs.items()}
    zero = lambda t: torch.zeros_like(t).double() if t.grad is None else t.grad.double()
    res.update(d_sdf=zero(sdf), d_normal=zero(normal), d_features=zero(feats), d_bg=zero(bg))
    if trainable:
        res["d_p"] = p.grad.double().reshape(1)
    else:
        assert p.grad is None
    return res


MODELS = [(False, 0.0), (False, 0.5), (False, 1.0), (True, 1.0)]      # (use_volsdf, cos_anneal_ratio): VolSDF does not read the ratio


@pytest.mark.parametrize("trainable", [True, False], ids=["variance-trainable", "variance-frozen"])
@pytest.mark.parametrize("color_act", [0, 1], ids=["colours", "sigmoid"])
@pytest.mark.parametrize("use_volsdf, k", MODELS, ids=["neus-k0", "neus-k0.5", "neus-k1", "volsdf"])
def test_compositing_pass_against_float64(use_volsdf, k, color_act, trainable):
    """Bound per output and gradient: e_fused <= 4 e_composed + 2e-6 max|ref|, e_* the largest error against float64, e_composed that of the
    fp32 tensor-op route on the same device (the bound of tests/test_gpu_volsdf_pass.py)."""
    c = _case()
    ref = _chain(c, use_volsdf, k, color_act, trainable, "ref")
    composed = _chain(c, use_volsdf, k, color_act, trainable, "composed")
    fused = _chain(c, use_volsdf, k, color_act, trainable, "fused")
    assert set(fused) == set(ref) == set(composed)
    at = {int(cn): int(b) for b, cn in zip(c["offset"], c["counts"])}
    if not use_volsdf:      # the built samples are what they were built to be
        T65 = ref["weights"][at[65] + 33:at[65] + 65]
        assert float(ref["weights"][at[65] + 32]) > 0 and float(T65.abs().max()) == 0.0, "alpha == 1 must end the ray"
        assert float(ref["weights"][at[63] + 40]) == 0.0 and float(fused["weights"][at[63] + 40]) == 0.0, "alpha clipped to 0"
        assert float(fused["weights"][at[65] + 33:at[65] + 65].abs().max()) == 0.0
    else:
        assert float(fused["d_normal"].abs().max()) == 0.0
    assert float(fused["opacity"][0]) == 0.0 and torch.equal(fused["comp_rgb"][0], _dev(c["bg"])[0].double())     # the empty ray
    bad, lines = [], []
    for name in ref:
        assert fused[name].shape == ref[name].shape and torch.isfinite(fused[name]).all(), name
        scale = float(ref[name].abs().max())
        e_f, e_c = float((fused[name] - ref[name]).abs().max()), float((composed[name] - ref[name]).abs().max())
        bound = 4.0 * e_c + 2e-6 * scale
        lines.append(f"volsdf={int(use_volsdf)} k={k} act={color_act} trainable={int(trainable)} {name:<11s} max|ref|={scale:.3e} e_fused={e_f:.3e} "
                     f"e_composed={e_c:.3e} bound={bound:.3e}")
        if not e_f <= bound:
            bad.append(name)
    print("\n".join(lines))
    assert not bad, bad


def _threshold_near(vals: np.ndarray, nominal: float) -> float:
    """a threshold close to `nominal` that no value comes within 2e-4 (relative) of: the geometric middle of a wide enough gap"""
    v = np.unique(vals[vals > 0])
    i = int(np.searchsorted(v, nominal))
    for d in range(len(v)):
        for j in (i + d, i - d):
            if 1 <= j < len(v) and v[j] / v[j - 1] > 1.0 + 1e-3:
                return float(np.sqrt(v[j] * v[j - 1]))
    raise AssertionError("no gap")


@pytest.mark.parametrize("use_volsdf", [False, True], ids=["neus", "volsdf"])
def test_prune_count_equals_step_alpha_plus_the_visibility_rule(use_volsdf):
    from scaledreamer_amd import ops

    c = _case(COUNTS + [300, 7, 0, 129], seed=5, special=False)
    sdf, offset, count = _dev(c["sdf"]), _dev(c["offset"]), _dev(c["counts"])
    p = torch.tensor(P0, device="cuda")
    step = 0.02
    alpha = ops.neus_step_alpha(sdf, p, step, use_volsdf)
    a32 = torch.exp(p * 10.0).clamp(1.0e-6, 1.0e6)
    want_alpha = _alpha_ops(sdf.double(), None, None, torch.full_like(sdf, step).double(), a32.double(), 1.0, True) if use_volsdf else None
    if use_volsdf:
        torch.testing.assert_close(alpha.double(), want_alpha, rtol=1e-5, atol=1e-7)
    else:
        s, a = sdf.double(), a32.double()
        prev, nxt = torch.sigmoid((s + step * 0.5) * a), torch.sigmoid((s - step * 0.5) * a)
        torch.testing.assert_close(alpha.double(), ((prev - nxt + 1e-5) / (prev + 1e-5)).clip(0.0, 1.0), rtol=1e-4, atol=1e-6)
    a64 = alpha.double().cpu().numpy()
    T = np.ones_like(a64)
    for b, cnt in zip(c["offset"], c["counts"]):
        if cnt > 0:
            T[b:b + cnt] = np.concatenate([[1.0], np.cumprod(1.0 - a64[b:b + cnt])[:-1]])
    alpha_thre, eps = _threshold_near(a64, 0.01), _threshold_near(T, 1e-4)
    want = (T >= eps) & (a64 >= alpha_thre)
    assert 0 < want.sum() < want.size and (T < eps).any() and (a64 < alpha_thre).any()
    keep, kept = ops.neus_prune(sdf, offset, count, p, step, use_volsdf, eps, alpha_thre)
    np.testing.assert_array_equal(keep.cpu().numpy().astype(bool), want)
    np.testing.assert_array_equal(kept.cpu().numpy(), [int(want[b:b + cnt].sum()) for b, cnt in zip(c["offset"], c["counts"])])
    # n_dev: only the live prefix is written
    n_live = 100
    buf = torch.full_like(sdf, -7.0)
    from scaledreamer_amd import _lib
    _lib.check(_lib.lib().asd_neus_step_alpha(_lib.ptr(sdf), _lib.i32(sdf.numel()), _lib.ptr(torch.tensor([n_live], device="cuda", dtype=torch.int32)),
                                              _lib.ptr(p), _lib.f32(step), _lib.i32(int(use_volsdf)), _lib.ptr(buf), _lib.stream()))
    assert torch.equal(buf[:n_live], alpha[:n_live]) and bool((buf[n_live:] == -7.0).all())


GUARD = 1 << 16


def _guarded(nbytes: int):
    buf = torch.full((nbytes + 2 * GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    return buf, buf[GUARD:GUARD + nbytes]


def _intact(buf, nbytes):
    return bool((buf[:GUARD] == 0xA5).all()) and bool((buf[GUARD + nbytes:] == 0xA5).all())


@pytest.mark.parametrize("use_volsdf", [0, 1], ids=["neus", "volsdf"])
def test_entries_stay_inside_their_outputs_and_repeat_bit_for_bit(use_volsdf):
    from scaledreamer_amd import _lib

    L = _lib.lib()
    counts = np.random.default_rng(9).integers(0, 140, 773)       # (not a multiple of the four rays a block holds)
    counts[-1] = 131                                              # the last ray ends the arrays: a trip that runs over would leave them
    c = _case(counts, seed=2, special=False)
    n, nr = c["n"], c["n_rays"]
    t = {k: _dev(c[k]) for k in ("sdf", "normal", "dirs", "t0", "t1", "feats", "bg", "offset", "counts")}
    ups = {k: _dev(v) for k, v in c["ups"].items()}
    p = torch.tensor(P0, device="cuda")
    i32, f32, ptr, st = _lib.i32, _lib.f32, _lib.ptr, _lib.stream()
    bufs = {}

    def out(name, elems, width=4):
        bufs[name] = (*_guarded(elems * width), elems * width)
        return C.c_void_p(bufs[name][1].data_ptr())

    def check_all(entry):
        torch.cuda.synchronize()
        for name, (buf, _, nbytes) in bufs.items():
            assert _intact(buf, nbytes), f"{entry} wrote outside `{name}`"

    def run_all():
        bufs.clear()
        _lib.check(L.asd_neus_step_alpha(ptr(t["sdf"]), i32(n), None, ptr(p), f32(0.02), i32(use_volsdf), out("alpha", n), st))
        check_all("asd_neus_step_alpha")
        _lib.check(L.asd_neus_prune_count(ptr(t["sdf"]), ptr(t["offset"]), ptr(t["counts"]), i32(nr), ptr(p), f32(0.02), i32(use_volsdf), f32(1e-4),
                                          f32(0.01), out("keep", n, 1), out("kept", nr), st))
        check_all("asd_neus_prune_count")
        common = [ptr(t[k]) for k in ("sdf", "normal", "dirs", "t0", "t1", "feats")] + [i32(1), ptr(p), f32(0.5), i32(use_volsdf), ptr(t["bg"]),
                                                                                           ptr(t["offset"]), ptr(t["counts"]), i32(nr)]
        _lib.check(L.asd_neus_composite_fwd(*common, out("weights", n), out("opacity", nr), out("depth", nr), out("rgb_fg", nr * 3),
                                            out("comp_rgb", nr * 3), out("comp_normal", nr * 3), st))
        check_all("asd_neus_composite_fwd")
        w, op = (C.c_void_p(bufs[k][1].data_ptr()) for k in ("weights", "opacity"))
        _lib.check(L.asd_neus_composite_bwd(*common, w, op, ptr(ups["comp_rgb"]), ptr(ups["rgb_fg"]), ptr(ups["opacity"]), ptr(ups["depth"]),
                                            ptr(ups["weights"]), out("d_sdf", n), out("d_normal", n * 3), out("d_features", n * 3), out("d_bg", nr * 3),
                                            out("d_p", 1), out("dp_partial", nr), st))
        check_all("asd_neus_composite_bwd")
        return {k: bufs[k][1].view(torch.uint8 if k == "keep" else torch.int32 if k == "kept" else torch.float32).clone() for k in bufs}

    first, second = run_all(), run_all()
    for k in first:
        assert not (first[k].view(torch.uint8) == 0xA5).all(), f"`{k}` was never written"
        if first[k].dtype == torch.float32:
            assert torch.isfinite(first[k]).all(), k
        assert torch.equal(first[k], second[k]), f"`{k}` differs between two runs on the same inputs"
    assert float(first["d_p"].abs()) > 0
