"""Oracle of the field kernels under a level limit (asd_grid_meta.n_masked_levels; ProgressiveBandHashGrid, threestudio/models/networks.py:129-167):
field_analytic_util's restated hash-grid encode times the reference's 0/1 column mask -> the SDF head and the feature head -> sphere bias,
at the point and at the three offset points clamped to [-radius, radius]; fd_grad = (s_k - s) / eps, normal = normalize(fd_grad)
(implicit_sdf.py:300-340).  Parameter gradients are autograd's, of sum over the kept samples of <cotangent, output>, with cotangents on
sdf, features, normal and fd_grad.  Float64 is the reference; the same code in float32 on the CPU gives E32 per output and per gradient;
the kernels are held to 4 x E32 (the rule of field_analytic_util.py).

eps is the progressive step of the level count: 2 radius / (base_resolution * per_level_scale ** (a - 1)) (implicit_sdf.py:396-404).

Left out of the gradient comparisons: a sample of which, in the float64 run, a hidden pre-activation of either MLP at any of its four
points lies within 2e-5 of the ReLU kink (the SDF head is evaluated at the four points, the feature head at the centre).  Only for level
counts a > 0 (at a = 0 every pre-activation is exactly 0 and ReLU'(0) = 0 on both sides).  At most 10 % of the samples may be left out:
a condition of the tests, asserted by test_field_progressive_cpu.py.
"""
from __future__ import annotations

import functools
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F

from field_analytic_util import CFGS, METAS, RADIUS, SEEDS, _bias, draw, encode, rel_err  # noqa: F401

CFG = CFGS["none_sphere_sdf"]
N, N_DEV = 257, 200
MAX_LEFT_OUT = 0.10
KINK = 2e-5
OUTPUTS = ("sdf", "features", "fd_grad", "normal")
PARAMS = ("grid", "w1d", "w2d", "w1f", "w2f")
# the routes of asd_field_bwd: (feature dims, cotangents, live rows)
ROUTES = {
    "mfma": (3, ("sdf", "features"), N),                          # no normal gradient, C = 3: MLP half on the matrix pipe, scatter only
    "fd": (3, ("sdf", "features", "normal", "fd_grad"), N),       # finite-difference rows on the VALU form
    "c0": (0, ("sdf", "normal", "fd_grad"), N),                   # n_feature_dims == 0
    # device-side live count, rows >= N_DEV are dead.  As the render pass calls it: no normal gradient (asd_field_bwd with n_dev AND
    # finite-difference rows reads the dead samples' rows of its workspace, which nothing writes: not a supported combination, before
    # or after the level limit)
    "ndev": (3, ("sdf", "features"), N_DEV),
}
GRAD_LEVELS = (4, 5, 6, 16)          # 4, 5, 6 straddle ASD_FIELD_NAGG = 5
FWD_LEVELS = (0, 4, 5, 6, 16)


def progressive_eps(meta_name: str, a: int) -> float:
    _, _, _, base, pls = METAS[meta_name]
    return 2 * RADIUS / (base * pls ** (a - 1))


def column_mask(a: int, n_levels: int = 16, dtype=torch.float64):
    m = torch.zeros(2 * n_levels, dtype=dtype)
    m[: 2 * a] = 1.0
    return m


def cotangents(meta_name: str, n: int):
    """draw()'s cotangents (sigma -> sdf, features, normal) and a seeded one for fd_grad"""
    _, _, _, cot = draw(meta_name, n)
    rng = np.random.default_rng(SEEDS[meta_name] + 13 * n)
    return SimpleNamespace(sdf=cot.sigma, features=cot.features, normal=cot.normal, fd_grad=rng.standard_normal((n, 3)).astype(np.float32))


def run(meta, P, pts, a: int, eps: float, dtype, cot=None, keep=None):
    """one evaluation in `dtype` with `a` active levels -> outputs (detached), the four points' pre-activations, and with `cot` the parameter
    gradients of every route of ROUTES"""
    t = {k: torch.tensor(getattr(P, k), dtype=dtype, requires_grad=True) for k in PARAMS}
    p = torch.tensor(pts, dtype=dtype)
    mask = column_mask(a, int(meta.n_levels), dtype)
    table = t["grid"].view(-1, 2)

    def heads(q):
        enc = encode(meta, table, (q + RADIUS) / (2 * RADIUS))[0] * mask
        a_d, a_f = enc @ t["w1d"].T, enc @ t["w1f"].T
        return (torch.relu(a_d) @ t["w2d"].T)[:, 0] + _bias(CFG, q), a_d, a_f

    s, a_d, a_f = heads(p)
    feats = torch.relu(a_f) @ t["w2f"].T
    pre = [a_d.detach(), a_f.detach()]
    sk = []
    for k in range(3):
        off = torch.zeros(3, dtype=dtype)
        off[k] = eps
        s_k, ad_k, af_k = heads(torch.clamp(p + off, -RADIUS, RADIUS))
        sk.append(s_k)
        pre.append(ad_k.detach())
    fd_grad = (torch.stack(sk, -1) - s[:, None]) / eps
    normal = F.normalize(fd_grad, dim=-1)
    vals = {"sdf": s, "features": feats, "fd_grad": fd_grad, "normal": normal}
    out = SimpleNamespace(**{k: v.detach() for k, v in vals.items()}, pre=torch.cat(pre, -1))
    if cot is not None:
        out.dparams = {}
        for route, (C, on, live) in ROUTES.items():
            k = torch.as_tensor(keep, dtype=dtype).clone()
            k[live:] = 0.0
            loss = sum(((torch.tensor(getattr(cot, name), dtype=dtype) * vals[name]).reshape(len(pts), -1).sum(-1) * k).sum() for name in on)
            gs = torch.autograd.grad(loss, [t[k_] for k_ in PARAMS], allow_unused=True, retain_graph=True)
            out.dparams[route] = {k_: (torch.zeros_like(t[k_]) if g is None else g).detach() for k_, g in zip(PARAMS, gs)}
    return out


def left_out(ref, a: int) -> np.ndarray:
    if a == 0:
        return np.zeros(ref.pre.shape[0], dtype=bool)
    return (ref.pre.abs() < KINK).any(-1).numpy()


@functools.lru_cache(maxsize=None)
def case(meta_name: str, a: int, with_bwd: bool = True):
    """the shared reference of one (meta, level count): float64 outputs, per-route parameter gradients, the kept mask and E32 of every
    output and gradient.  Computed once per process; callers must not write into it."""
    meta, P, pts, _ = draw(meta_name, N)
    cot = cotangents(meta_name, N)
    eps = progressive_eps(meta_name, a)
    ref = run(meta, P, pts, a, eps, torch.float64)
    keep = ~left_out(ref, a)
    f32 = run(meta, P, pts, a, eps, torch.float32)
    e32 = {k: rel_err(getattr(f32, k), getattr(ref, k), keep) for k in OUTPUTS}
    dref = {}
    if with_bwd:
        dref = run(meta, P, pts, a, eps, torch.float64, cot, keep).dparams
        d32 = run(meta, P, pts, a, eps, torch.float32, cot, keep).dparams
        for route in ROUTES:
            for k in PARAMS:
                if float(dref[route][k].abs().max()) > 0:
                    e32[f"{route}/d_{k}"] = rel_err(d32[route][k], dref[route][k])
    return SimpleNamespace(meta_name=meta_name, a=a, P=P, pts=pts, cot=cot, eps=eps, ref=ref, keep=keep, e32=e32, dref=dref, n=N)


def field_cfg(eps: float, n_feature_dims: int = 3):
    from scaledreamer_amd import _lib

    f = _lib.FieldCfg()
    for d in range(3):
        f.bbox_min[d], f.bbox_max[d] = -RADIUS, RADIUS
    f.radius, f.bias_mode, f.bias_value = RADIUS, CFG["bias_mode"], CFG["bias_value"]
    f.blob_scale, f.blob_std, f.activation = CFG["blob_scale"], CFG["blob_std"], CFG["activation"]
    f.fd_eps, f.n_hidden, f.n_feature_dims, f.field_mode = eps, 64, n_feature_dims, CFG["field_mode"]
    return f


def limited_meta(meta_name: str, a: int):
    from scaledreamer_amd import _lib

    m = _lib.make_grid_meta(*METAS[meta_name])
    m.n_masked_levels = int(m.n_levels) - a
    return m


# samples left out by the kink rule, of N = 257 (test_field_progressive_cpu.py asserts them and the 10 % cap)
LEFT_OUT = {"A/4": 13, "A/5": 17, "A/6": 16, "A/16": 8, "B/4": 22, "B/5": 16, "B/6": 11, "B/16": 11}

# E32 as measured with this file on the CPU: max-norm error of the float32 run against the float64 run, relative to the float64
# quantity's max magnitude; outputs over the kept samples, "<route>/d_<parameter>" = parameter gradients of the route's loss.
# test_field_progressive_cpu.py recomputes them from the seeds.  The GPU tests hold the kernels to 4 x these.
E32 = {
    "A/0": {
        "sdf": 8.806e-08, "features": 0.000e+00, "fd_grad": 2.539e-07, "normal": 4.901e-07,
    },
    "A/1": {
        "sdf": 9.988e-08, "features": 3.006e-07, "fd_grad": 2.920e-07, "normal": 5.681e-07,
    },
    "A/4": {
        "sdf": 1.456e-07, "features": 5.842e-07, "fd_grad": 5.901e-07, "normal": 2.164e-06, "mfma/d_grid": 2.598e-07,
        "mfma/d_w1d": 3.852e-07, "mfma/d_w2d": 2.218e-07, "mfma/d_w1f": 4.446e-07, "mfma/d_w2f": 4.459e-07, "fd/d_grid": 7.425e-07,
        "fd/d_w1d": 8.060e-07, "fd/d_w2d": 1.165e-06, "fd/d_w1f": 4.446e-07, "fd/d_w2f": 4.459e-07, "c0/d_grid": 8.303e-07,
        "c0/d_w1d": 8.060e-07, "c0/d_w2d": 1.165e-06, "ndev/d_grid": 2.966e-07, "ndev/d_w1d": 3.788e-07, "ndev/d_w2d": 2.911e-07,
        "ndev/d_w1f": 5.418e-07, "ndev/d_w2f": 5.372e-07,
    },
    "A/5": {
        "sdf": 1.419e-07, "features": 7.253e-07, "fd_grad": 8.222e-07, "normal": 2.439e-06, "mfma/d_grid": 3.630e-07,
        "mfma/d_w1d": 5.994e-07, "mfma/d_w2d": 2.818e-07, "mfma/d_w1f": 5.745e-07, "mfma/d_w2f": 3.869e-07, "fd/d_grid": 8.562e-07,
        "fd/d_w1d": 1.232e-06, "fd/d_w2d": 9.751e-07, "fd/d_w1f": 5.745e-07, "fd/d_w2f": 3.869e-07, "c0/d_grid": 8.855e-07,
        "c0/d_w1d": 1.232e-06, "c0/d_w2d": 9.751e-07, "ndev/d_grid": 5.288e-07, "ndev/d_w1d": 6.570e-07, "ndev/d_w2d": 3.414e-07,
        "ndev/d_w1f": 7.209e-07, "ndev/d_w2f": 7.817e-07,
    },
    "A/6": {
        "sdf": 1.688e-07, "features": 8.525e-07, "fd_grad": 1.020e-06, "normal": 3.290e-06, "mfma/d_grid": 4.042e-07,
        "mfma/d_w1d": 6.746e-07, "mfma/d_w2d": 3.190e-07, "mfma/d_w1f": 7.241e-07, "mfma/d_w2f": 6.167e-07, "fd/d_grid": 3.242e-06,
        "fd/d_w1d": 1.191e-06, "fd/d_w2d": 2.002e-06, "fd/d_w1f": 7.241e-07, "fd/d_w2f": 6.167e-07, "c0/d_grid": 3.080e-06,
        "c0/d_w1d": 1.191e-06, "c0/d_w2d": 2.002e-06, "ndev/d_grid": 5.841e-07, "ndev/d_w1d": 7.357e-07, "ndev/d_w2d": 5.196e-07,
        "ndev/d_w1f": 1.015e-06, "ndev/d_w2f": 4.855e-07,
    },
    "A/16": {
        "sdf": 2.098e-06, "features": 5.906e-06, "fd_grad": 1.328e-05, "normal": 5.107e-05, "mfma/d_grid": 1.001e-05,
        "mfma/d_w1d": 5.725e-06, "mfma/d_w2d": 4.852e-06, "mfma/d_w1f": 8.660e-06, "mfma/d_w2f": 5.153e-06, "fd/d_grid": 1.486e-05,
        "fd/d_w1d": 9.402e-06, "fd/d_w2d": 1.334e-05, "fd/d_w1f": 8.660e-06, "fd/d_w2f": 5.153e-06, "c0/d_grid": 1.487e-05,
        "c0/d_w1d": 9.402e-06, "c0/d_w2d": 1.334e-05, "ndev/d_grid": 5.857e-06, "ndev/d_w1d": 8.491e-06, "ndev/d_w2d": 4.425e-06,
        "ndev/d_w1f": 9.848e-06, "ndev/d_w2f": 5.916e-06,
    },
    "B/0": {
        "sdf": 9.621e-08, "features": 0.000e+00, "fd_grad": 8.751e-07, "normal": 1.308e-06,
    },
    "B/1": {
        "sdf": 2.006e-07, "features": 1.461e-06, "fd_grad": 1.045e-06, "normal": 3.127e-06,
    },
    "B/4": {
        "sdf": 4.686e-07, "features": 2.677e-06, "fd_grad": 3.925e-06, "normal": 1.173e-05, "mfma/d_grid": 2.522e-06,
        "mfma/d_w1d": 3.782e-06, "mfma/d_w2d": 5.393e-06, "mfma/d_w1f": 1.938e-06, "mfma/d_w2f": 2.630e-06, "fd/d_grid": 7.485e-06,
        "fd/d_w1d": 4.058e-06, "fd/d_w2d": 5.570e-06, "fd/d_w1f": 1.938e-06, "fd/d_w2f": 2.630e-06, "c0/d_grid": 7.426e-06,
        "c0/d_w1d": 4.058e-06, "c0/d_w2d": 5.570e-06, "ndev/d_grid": 2.522e-06, "ndev/d_w1d": 3.572e-06, "ndev/d_w2d": 3.820e-06,
        "ndev/d_w1f": 2.278e-06, "ndev/d_w2f": 3.116e-06,
    },
    "B/5": {
        "sdf": 1.032e-06, "features": 3.789e-06, "fd_grad": 6.175e-06, "normal": 3.308e-05, "mfma/d_grid": 3.769e-06,
        "mfma/d_w1d": 1.908e-06, "mfma/d_w2d": 4.015e-06, "mfma/d_w1f": 6.095e-06, "mfma/d_w2f": 3.317e-06, "fd/d_grid": 1.038e-04,
        "fd/d_w1d": 3.192e-05, "fd/d_w2d": 1.996e-05, "fd/d_w1f": 6.095e-06, "fd/d_w2f": 3.317e-06, "c0/d_grid": 1.038e-04,
        "c0/d_w1d": 3.192e-05, "c0/d_w2d": 1.996e-05, "ndev/d_grid": 3.829e-06, "ndev/d_w1d": 2.930e-06, "ndev/d_w2d": 4.170e-06,
        "ndev/d_w1f": 2.595e-06, "ndev/d_w2f": 3.116e-06,
    },
    "B/6": {
        "sdf": 1.047e-06, "features": 3.460e-06, "fd_grad": 6.700e-06, "normal": 3.146e-05, "mfma/d_grid": 7.338e-06,
        "mfma/d_w1d": 3.490e-06, "mfma/d_w2d": 4.751e-06, "mfma/d_w1f": 5.906e-06, "mfma/d_w2f": 3.729e-06, "fd/d_grid": 1.176e-05,
        "fd/d_w1d": 9.645e-06, "fd/d_w2d": 9.912e-06, "fd/d_w1f": 5.906e-06, "fd/d_w2f": 3.729e-06, "c0/d_grid": 1.180e-05,
        "c0/d_w1d": 9.645e-06, "c0/d_w2d": 9.912e-06, "ndev/d_grid": 7.338e-06, "ndev/d_w1d": 4.674e-06, "ndev/d_w2d": 3.141e-06,
        "ndev/d_w1f": 3.794e-06, "ndev/d_w2f": 2.959e-06,
    },
    "B/16": {
        "sdf": 2.893e-05, "features": 1.184e-04, "fd_grad": 3.100e-04, "normal": 1.891e-03, "mfma/d_grid": 2.378e-04,
        "mfma/d_w1d": 2.329e-04, "mfma/d_w2d": 1.304e-04, "mfma/d_w1f": 1.959e-04, "mfma/d_w2f": 8.758e-05, "fd/d_grid": 3.720e-04,
        "fd/d_w1d": 3.416e-04, "fd/d_w2d": 2.785e-04, "fd/d_w1f": 1.959e-04, "fd/d_w2f": 8.758e-05, "c0/d_grid": 3.719e-04,
        "c0/d_w1d": 3.416e-04, "c0/d_w2d": 2.785e-04, "ndev/d_grid": 1.784e-04, "ndev/d_w1d": 1.586e-04, "ndev/d_w2d": 8.028e-05,
        "ndev/d_w1f": 2.078e-04, "ndev/d_w2f": 9.810e-05,
    },
}
