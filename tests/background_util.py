"""Float64 restatement of the two parameter-light backgrounds (`textured-background`, `solid-color-background`), the directions at which the
equirect mapping has an edge, and the tolerance builders of tests/test_gpu_background.py.

The restatement is written from the mapping itself (clamped bilinear lookup, no F.grid_sample), so tests/test_background_cpu.py can hold it
against the goldens the reference's own classes produced; the GPU tests then use it, evaluated in float64 on the same fp32 inputs, as the
reference for shapes the goldens do not cover.
"""
from __future__ import annotations

import math

import torch

# ±z (the poles: atan2(0, 0) = 0, v = 0.5), ±x, ±y, the azimuth seam from both sides (the sign of a zero y decides the row), (0, 0, 0)
SPECIAL_DIRS = [
    (0.0, 0.0, 1.0), (0.0, 0.0, -1.0), (1.0, 0.0, 0.0), (-1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, -1.0, 0.0),
    (-1.0, 0.0, 0.0), (-1.0, -0.0, 0.0), (-1.0, 1e-9, 0.0), (-1.0, -1e-9, 0.0), (0.0, 0.0, 0.0),
]


def special_dirs() -> torch.Tensor:
    return torch.tensor(SPECIAL_DIRS, dtype=torch.float32)


def random_dirs(n: int, seed: int) -> torch.Tensor:
    g = torch.Generator().manual_seed(seed)
    return torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=-1)


def contended_dirs(n: int, seed: int) -> torch.Tensor:
    """one camera's small solid angle: thousands of rays on one texel of a 64 x 64 texture"""
    g = torch.Generator().manual_seed(seed)
    d = torch.tensor([1.0, 0.3, 0.2]) + 0.4 * (torch.rand(n, 3, generator=g) - 0.5)
    return torch.nn.functional.normalize(d, dim=-1)


def with_special(dirs: torch.Tensor) -> torch.Tensor:
    return torch.cat([special_dirs(), dirs], 0)


def sample_point(dirs: torch.Tensor, H: int, W: int):
    """(ix, iy) in texels, float64: u (polar angle) runs along the WIDTH, v (azimuth) along the HEIGHT; u, v lie in [0, 1], so the
    reflection of grid_sample(padding_mode="reflection", align_corners=False) never acts and its clip is this clamp"""
    d = dirs.double()
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    u = torch.atan2(torch.sqrt(x * x + y * y), z) / math.pi
    v = torch.atan2(y, x) / (2.0 * math.pi) + 0.5
    return (u * W - 0.5).clamp(0.0, W - 1.0), (v * H - 0.5).clamp(0.0, H - 1.0)


def _act(name):
    return {"sigmoid": torch.sigmoid, "none": lambda t: t, "tanh": torch.tanh}[name]


def texture_sample(texture: torch.Tensor, dirs: torch.Tensor) -> torch.Tensor:
    """texture [C,H,W] -> the pre-activation bilinear sample [n,C], float64 (differentiable with respect to the texture)"""
    tex = texture.double()
    C, H, W = tex.shape
    ix, iy = sample_point(dirs, H, W)
    x0, y0 = ix.floor().long(), iy.floor().long()
    x1, y1 = (x0 + 1).clamp(max=W - 1), (y0 + 1).clamp(max=H - 1)
    wx, wy = ix - x0, iy - y0
    s = (tex[:, y0, x0] * ((1 - wx) * (1 - wy)) + tex[:, y0, x1] * (wx * (1 - wy)) + tex[:, y1, x0] * ((1 - wx) * wy) + tex[:, y1, x1] * (wx * wy))
    return s.T


def texture_color(texture: torch.Tensor, dirs: torch.Tensor, activation: str = "sigmoid") -> torch.Tensor:
    return _act(activation)(texture_sample(texture, dirs))


def texture_grad(texture: torch.Tensor, dirs: torch.Tensor, d_color: torch.Tensor, activation: str = "sigmoid") -> torch.Tensor:
    """d_texture [C,H,W] of sum(color * d_color), float64"""
    t = texture.double().detach().requires_grad_(True)
    return torch.autograd.grad(texture_color(t, dirs, activation), t, d_color.double())[0]


def solid_color(colors: torch.Tensor, rays_per_view: int) -> torch.Tensor:
    """colors [V,C] -> [V * R, C]"""
    return colors.repeat_interleave(rays_per_view, dim=0)


def solid_grad(d_out: torch.Tensor, n_views: int) -> torch.Tensor:
    return d_out.double().view(n_views, -1, d_out.shape[-1]).sum(1)


def forward_tolerance(texture: torch.Tensor, activation: str) -> float:
    """8 * 2^-23 * max(H, W) * D * A' + 2^-22: fp32 rounding of (ix, iy) is an absolute error of a few 2^-23 max(H, W) in the bilinear
    weights; D = the largest difference of horizontally or vertically adjacent texels; A' = max |act'| (0.25 sigmoid, 1 none)"""
    tex = texture.double()
    C, H, W = tex.shape
    D = 0.0
    if W > 1:
        D = max(D, float((tex[:, :, 1:] - tex[:, :, :-1]).abs().max()))
    if H > 1:
        D = max(D, float((tex[:, 1:, :] - tex[:, :-1, :]).abs().max()))
    A = {"sigmoid": 0.25, "none": 1.0}[activation]
    return 8.0 * 2.0 ** -23 * max(H, W) * D * A + 2.0 ** -22


def backward_unit(texture: torch.Tensor, dirs: torch.Tensor, d_color: torch.Tensor, activation: str):
    """-> (unit [C,H,W], n_t [H,W]).  Per texel t: G_t = sum |d_color_r act'_r| and n_t = the count over the rays whose float64 sample
    point lies within 1.001 texels of t on both axes; unit = 2^-23 (max(H, W) + n_t) G_t per channel."""
    tex = texture.double()
    C, H, W = tex.shape
    ix, iy = sample_point(dirs, H, W)
    s = texture_sample(tex, dirs)
    if activation == "sigmoid":
        a = torch.sigmoid(s)
        dact = a * (1 - a)
    elif activation == "none":
        dact = torch.ones_like(s)
    else:
        raise ValueError(activation)
    mag = (d_color.double() * dact).abs()                       # [n, C]
    G = torch.zeros(H * W, C, dtype=torch.float64)
    n_t = torch.zeros(H * W, dtype=torch.float64)
    fx, fy = ix.floor().long(), iy.floor().long()
    for dy in (-1, 0, 1, 2):
        for dx in (-1, 0, 1, 2):
            tx, ty = fx + dx, fy + dy
            ok = (tx >= 0) & (tx < W) & (ty >= 0) & (ty < H) & ((ix - tx).abs() <= 1.001) & ((iy - ty).abs() <= 1.001)
            idx = (ty * W + tx)[ok]
            G.index_add_(0, idx, mag[ok])
            n_t.index_add_(0, idx, torch.ones(idx.shape[0], dtype=torch.float64))
    n_t = n_t.view(H, W)
    unit = 2.0 ** -23 * (max(H, W) + n_t)[None] * G.T.reshape(C, H, W)
    return unit, n_t
