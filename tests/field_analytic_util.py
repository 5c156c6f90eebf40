"""Oracle of the analytic-normal field kernels (csrc/field_analytic.hip): a torch restatement of
hash-grid encode -> two VanillaMLPs -> density bias -> activation, written from the formulas of tcnn's grid encoding and
threestudio's ImplicitVolume, not from the kernels.  It is differentiable, so autograd.grad(..., create_graph=True) yields the position
gradient and the normal exactly as the reference forms them (implicit_volume.py:181-190), and a second backward yields every parameter
gradient.  Run in float64 it is the reference; run in float32 on the CPU it measures E32, the error a float32 evaluation of the same
mathematics has against float64 (max-norm, relative to the float64 output's max magnitude).  The kernels must be within 4 x E32.

Everything is a fixed seeded draw; a case (meta, cfg, n) is computed once per process and shared (case()).
"""
from __future__ import annotations

import functools
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F

BIAS_CONST, BIAS_MAGIC3D, BIAS_DREAMFUSION, BIAS_SPHERE = 0, 1, 2, 3
ACT_SOFTPLUS, ACT_EXP, ACT_TRUNC_EXP, ACT_NONE = 0, 1, 2, 3
RADIUS = 1.0

# meta: (n_levels, n_features, log2_hashmap_size, base_resolution, per_level_scale)
METAS = {
    "A": (16, 2, 12, 4, 1.3),                       # small tables, dense and hashed levels, many collisions; largest scale ~ 204
    "B": (16, 2, 19, 16, 1.447269237440378),        # the shipped configuration
}
# cfg: activation, bias_mode, bias_value, blob_scale, blob_std, field_mode (0 density, 1 SDF)
CFGS = {
    "softplus_magic3d": dict(activation=ACT_SOFTPLUS, bias_mode=BIAS_MAGIC3D, bias_value=0.0, blob_scale=10.0, blob_std=0.5, field_mode=0),
    "exp_const": dict(activation=ACT_EXP, bias_mode=BIAS_CONST, bias_value=0.5, blob_scale=10.0, blob_std=0.5, field_mode=0),
    "none_sphere_sdf": dict(activation=ACT_NONE, bias_mode=BIAS_SPHERE, bias_value=0.5, blob_scale=10.0, blob_std=0.5, field_mode=1),
    # blob_scale 20: raw = mlp + 20 exp(-2 r^2) is above 15 for r < 0.38, a few of every hundred points
    "truncexp_dreamfusion": dict(activation=ACT_TRUNC_EXP, bias_mode=BIAS_DREAMFUSION, bias_value=0.0, blob_scale=20.0, blob_std=0.5, field_mode=0),
    # the finite-difference property test: its bound is stated in units of sigma's own rounding (2^-23 |sigma|), so the constant is chosen
    # to dominate sigma; what else a float32 evaluation rounds (the MLP's sums of ~0.3, positions to 2^-16 of a cell at scale 204) stays below it
    "none_const": dict(activation=ACT_NONE, bias_mode=BIAS_CONST, bias_value=4.0, blob_scale=10.0, blob_std=0.5, field_mode=0),
}
SEEDS = {"A": 1101, "B": 2202}
OUTPUTS = ("sigma", "features", "grad", "normal")
PARAMS = ("grid", "w1d", "w2d", "w1f", "w2f")
MAX_LEFT_OUT = 0.10


class _TruncExp(torch.autograd.Function):
    """threestudio/utils/ops.py:41-54: forward exp(x), backward g * exp(clamp(x, max=15)) (differentiable again under create_graph)"""

    @staticmethod
    def forward(ctx, x):
        ctx.save_for_backward(x)
        return torch.exp(x)

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        return g * torch.exp(torch.clamp(x, max=15))


def make_meta(name):
    from scaledreamer_amd import _lib

    return _lib.make_grid_meta(*METAS[name])


def draw(meta_name: str, n: int):
    """tables U(-0.5, 0.5), W1 ~ N(0, 1/sqrt(32)), W2 ~ N(0, 1/8), points uniform in [-0.95 r, 0.95 r]^3 with |p| >= 0.05; float32 values"""
    meta = make_meta(meta_name)
    rng = np.random.default_rng(SEEDS[meta_name])
    f = np.float32
    P = SimpleNamespace(
        grid=rng.uniform(-0.5, 0.5, meta.n_params).astype(f),
        w1d=(rng.standard_normal((64, 32)) / np.sqrt(32.0)).astype(f), w2d=(rng.standard_normal((1, 64)) / 8.0).astype(f),
        w1f=(rng.standard_normal((64, 32)) / np.sqrt(32.0)).astype(f), w2f=(rng.standard_normal((3, 64)) / 8.0).astype(f))
    prng = np.random.default_rng(SEEDS[meta_name] + 7 * n)
    pts = prng.uniform(-0.95 * RADIUS, 0.95 * RADIUS, (4 * n + 16, 3))
    pts = pts[np.linalg.norm(pts, axis=1) >= 0.05][:n].astype(f)
    assert pts.shape == (n, 3)
    cot = SimpleNamespace(sigma=prng.standard_normal(n).astype(f), features=prng.standard_normal((n, 3)).astype(f),
                          normal=prng.standard_normal((n, 3)).astype(f))
    return meta, P, pts, cot


def _levels(meta):
    L = int(meta.n_levels)
    return [(float(meta.scale[l]), int(meta.resolution[l]), int(meta.offset[l]), int(meta.size[l]), bool(meta.dense[l])) for l in range(L)]


def grid_index(res, size, dense, cx, cy, cz):
    """the table index of integer corner (cx, cy, cz): direct while the level's res^3 fits its table (one wrap), else tcnn's spatial hash"""
    if dense:
        di = cx + cy * res + cz * res * res
        return torch.where(di >= size, di - size, di)
    m = 0xFFFFFFFF
    return (((cx * 1) & m) ^ ((cy * 2654435761) & m) ^ ((cz * 805459861) & m)) & (size - 1)


def encode(meta, table, u):
    """table [entries, 2], u [n, 3] in the unit cube -> ([n, 2 L], positions [n, L, 3]); one gather for all levels and corners"""
    u = torch.clamp(u, 0.0, 1.0)
    idx, wts, poss = [], [], []
    for s, res, off, size, dense in _levels(meta):
        pos = s * u + 0.5
        fl = torch.floor(pos)
        w = pos - fl
        c = fl.detach().to(torch.int64)
        for corner in range(8):
            d = [(corner >> k) & 1 for k in range(3)]
            idx.append(off + grid_index(res, size, dense, c[:, 0] + d[0], c[:, 1] + d[1], c[:, 2] + d[2]))
            ax = [w[:, k] if d[k] else 1.0 - w[:, k] for k in range(3)]
            wts.append(ax[0] * ax[1] * ax[2])
        poss.append(pos)
    L = int(meta.n_levels)
    idx = torch.stack(idx, 1).view(-1, L, 8)
    wts = torch.stack(wts, 1).view(-1, L, 8)
    vals = table[idx]                                            # [n, L, 8, 2]
    return (wts[..., None] * vals).sum(2).reshape(-1, 2 * L), torch.stack(poss, 1)


def _bias(cfg, p):
    r2 = (p * p).sum(-1)
    if cfg["bias_mode"] == BIAS_MAGIC3D:
        return cfg["blob_scale"] * (1 - torch.sqrt(r2) / cfg["blob_std"])
    if cfg["bias_mode"] == BIAS_DREAMFUSION:
        return cfg["blob_scale"] * torch.exp(-0.5 * r2 / cfg["blob_std"] ** 2)
    if cfg["bias_mode"] == BIAS_SPHERE:
        return torch.sqrt(r2) - cfg["bias_value"]
    return torch.full_like(r2, cfg["bias_value"])


def _act(cfg, raw):
    a = cfg["activation"]
    if a == ACT_SOFTPLUS:
        return F.softplus(raw)
    if a == ACT_EXP:
        return torch.exp(raw)
    if a == ACT_TRUNC_EXP:
        return _TruncExp.apply(raw)
    return raw


def run(meta, cfg, P, pts, dtype, keep=None, cot=None, cot_on=("sigma", "features", "normal")):
    """One evaluation in `dtype`.  -> namespace with sigma, features, grad, normal (detached), the quantities the left-out rule reads
    (pos, a_d, a_f), and, with `cot`, the parameter gradients of loss = sum over kept samples of <cotangent, output>."""
    t = {k: torch.tensor(getattr(P, k), dtype=dtype, requires_grad=True) for k in PARAMS}
    p = torch.tensor(pts, dtype=dtype, requires_grad=True)
    u = (p - (-RADIUS)) / (RADIUS - (-RADIUS))
    enc, pos = encode(meta, t["grid"].view(-1, 2), u)
    a_d = enc @ t["w1d"].T
    raw = (torch.relu(a_d) @ t["w2d"].T)[:, 0] + _bias(cfg, p)
    sigma = _act(cfg, raw)
    a_f = enc @ t["w1f"].T
    feats = torch.relu(a_f) @ t["w2f"].T
    (grad,) = torch.autograd.grad(sigma, p, grad_outputs=torch.ones_like(sigma), create_graph=True)
    normal = (1.0 if cfg["field_mode"] == 1 else -1.0) * F.normalize(grad, dim=-1)
    out = SimpleNamespace(sigma=sigma.detach(), features=feats.detach(), grad=grad.detach(), normal=normal.detach(), raw=raw.detach(),
                          pos=pos.detach(), a_d=a_d.detach(), a_f=a_f.detach())
    if cot is not None:
        k = torch.ones(len(pts), dtype=dtype) if keep is None else torch.as_tensor(keep, dtype=dtype)
        loss = 0.0
        for name, val in (("sigma", sigma), ("features", feats), ("normal", normal)):
            if name in cot_on:
                c = torch.tensor(getattr(cot, name), dtype=dtype)
                loss = loss + ((c * val).reshape(len(pts), -1).sum(-1) * k).sum()
        gs = torch.autograd.grad(loss, [t[k_] for k_ in PARAMS], allow_unused=True)
        out.dparams = {k_: (torch.zeros_like(t[k_]) if g is None else g).detach() for k_, g in zip(PARAMS, gs)}
    return out


def left_out(meta, ref) -> np.ndarray:
    """True where a sample sits on a discontinuity of the derivative: a level's position within max(8 s 2^-24, 1e-4) of a cell face, or a
    hidden pre-activation of either MLP within 2e-5 of its ReLU kink (read from the float64 run)"""
    out = torch.zeros(ref.pos.shape[0], dtype=torch.bool)
    for l, (s, *_rest) in enumerate(_levels(meta)):
        d = (ref.pos[:, l] - torch.round(ref.pos[:, l])).abs()
        out |= (d < max(8 * s * 2.0 ** -24, 1e-4)).any(-1)
    out |= (ref.a_d.abs() < 2e-5).any(-1) | (ref.a_f.abs() < 2e-5).any(-1)
    return out.numpy()


def rel_err(x, ref, rows=None) -> float:
    """max-norm error relative to the reference's max magnitude (over `rows` where given)"""
    x, ref = torch.as_tensor(x).double().cpu(), torch.as_tensor(ref).double().cpu()
    if rows is not None:
        x, ref = x[rows], ref[rows]
    return float((x - ref).abs().max() / ref.abs().max().clamp_min(1e-300))


COT_SETS = {"all": ("sigma", "features", "normal"), "normal": ("normal",), "sigma": ("sigma",)}


@functools.lru_cache(maxsize=None)
def case(meta_name: str, cfg_name: str, n: int, with_bwd: bool = True):
    """the shared reference of one configuration: float64 outputs and parameter gradients (per cotangent set), the kept mask, and E32 of
    every output and gradient.  Computed once; callers must not write into it."""
    meta, P, pts, cot = draw(meta_name, n)
    cfg = CFGS[cfg_name]
    ref = run(meta, cfg, P, pts, torch.float64)
    keep = ~left_out(meta, ref)
    f32 = run(meta, cfg, P, pts, torch.float32)
    e32 = {k: rel_err(getattr(f32, k), getattr(ref, k), keep) for k in OUTPUTS}
    dref = {}
    if with_bwd:
        for cs, on in COT_SETS.items():
            d64 = run(meta, cfg, P, pts, torch.float64, keep, cot, on).dparams
            d32 = run(meta, cfg, P, pts, torch.float32, keep, cot, on).dparams
            dref[cs] = d64
            for k in PARAMS:
                if float(d64[k].abs().max()) > 0:
                    e32[f"{cs}/d_{k}"] = rel_err(d32[k], d64[k])
    return SimpleNamespace(meta=meta, cfg=cfg, P=P, pts=pts, cot=cot, ref=ref, keep=keep, e32=e32, dref=dref, n=n)


def field_cfg(cfg: dict):
    from scaledreamer_amd import _lib

    f = _lib.FieldCfg()
    for d in range(3):
        f.bbox_min[d], f.bbox_max[d] = -RADIUS, RADIUS
    f.radius, f.bias_mode, f.bias_value = RADIUS, cfg["bias_mode"], cfg["bias_value"]
    f.blob_scale, f.blob_std, f.activation = cfg["blob_scale"], cfg["blob_std"], cfg["activation"]
    f.fd_eps, f.n_hidden, f.n_feature_dims, f.field_mode = 0.01, 64, 3, cfg["field_mode"]
    return f


# E32 as measured with this file on the CPU (max-norm error of the float32 run against the float64 run, relative to the float64 output's max
# magnitude; outputs over the kept samples; "<cotangents>/d_<parameter>" = parameter gradients of the loss over the kept samples).
# test_field_analytic_cpu.py recomputes them from the seeds.  The GPU tests hold the kernels to 4 x these.
E32 = {
    "A/softplus_magic3d/257": {  # left out: 5 of 257
        "sigma": 1.601e-07, "features": 5.906e-06, "grad": 3.375e-06, "normal": 2.446e-05,
        "all/d_grid": 1.878e-05, "all/d_w1d": 1.340e-05, "all/d_w2d": 9.622e-06, "all/d_w1f": 7.400e-06,
        "all/d_w2f": 5.316e-06, "normal/d_grid": 1.920e-05, "normal/d_w1d": 1.308e-05, "normal/d_w2d": 9.637e-06,
        "sigma/d_grid": 6.894e-06, "sigma/d_w1d": 8.009e-06, "sigma/d_w2d": 8.521e-06,
    },
    "A/exp_const/257": {  # left out: 5 of 257
        "sigma": 2.182e-06, "features": 5.906e-06, "grad": 9.296e-06, "normal": 3.459e-05,
        "all/d_grid": 1.925e-05, "all/d_w1d": 1.764e-05, "all/d_w2d": 2.939e-05, "all/d_w1f": 7.400e-06,
        "all/d_w2f": 5.316e-06, "normal/d_grid": 1.920e-05, "normal/d_w1d": 1.764e-05, "normal/d_w2d": 3.131e-05,
        "sigma/d_grid": 4.359e-06, "sigma/d_w1d": 5.755e-06, "sigma/d_w2d": 4.088e-06,
    },
    "A/none_sphere_sdf/257": {  # left out: 5 of 257
        "sigma": 2.098e-06, "features": 5.906e-06, "grad": 1.089e-05, "normal": 2.836e-05,
        "all/d_grid": 2.926e-05, "all/d_w1d": 3.248e-05, "all/d_w2d": 2.550e-05, "all/d_w1f": 7.400e-06,
        "all/d_w2f": 5.316e-06, "normal/d_grid": 2.940e-05, "normal/d_w1d": 3.358e-05, "normal/d_w2d": 2.450e-05,
        "sigma/d_grid": 5.019e-06, "sigma/d_w1d": 6.587e-06, "sigma/d_w2d": 4.843e-06,
    },
    "A/truncexp_dreamfusion/257": {  # left out: 5 of 257
        "sigma": 4.867e-07, "features": 5.906e-06, "grad": 3.505e-06, "normal": 2.745e-05,
        "all/d_grid": 6.506e-06, "all/d_w1d": 9.684e-06, "all/d_w2d": 9.800e-06, "all/d_w1f": 7.400e-06,
        "all/d_w2f": 5.316e-06, "normal/d_grid": 2.395e-05, "normal/d_w1d": 3.003e-05, "normal/d_w2d": 3.522e-05,
        "sigma/d_grid": 6.505e-06, "sigma/d_w1d": 9.683e-06, "sigma/d_w2d": 9.830e-06,
    },
    "A/softplus_magic3d/1": {  # left out: 0 of 1
        "sigma": 1.322e-07, "features": 1.973e-06, "grad": 1.123e-06, "normal": 4.491e-07,
        "all/d_grid": 7.222e-06, "all/d_w1d": 7.455e-06, "all/d_w2d": 1.020e-05, "all/d_w1f": 6.998e-06,
        "all/d_w2f": 3.801e-06, "normal/d_grid": 6.218e-06, "normal/d_w1d": 7.449e-06, "normal/d_w2d": 1.017e-05,
        "sigma/d_grid": 3.270e-06, "sigma/d_w1d": 7.016e-06, "sigma/d_w2d": 5.335e-06,
    },
    "B/softplus_magic3d/257": {  # left out: 11 of 257
        "sigma": 3.203e-06, "features": 1.184e-04, "grad": 3.489e-04, "normal": 5.805e-04,
        "all/d_grid": 8.566e-04, "all/d_w1d": 3.566e-04, "all/d_w2d": 3.322e-04, "all/d_w1f": 1.590e-04,
        "all/d_w2f": 8.965e-05, "normal/d_grid": 8.578e-04, "normal/d_w1d": 3.549e-04, "normal/d_w2d": 3.311e-04,
        "sigma/d_grid": 8.334e-05, "sigma/d_w1d": 6.557e-05, "sigma/d_w2d": 6.911e-05,
    },
}
