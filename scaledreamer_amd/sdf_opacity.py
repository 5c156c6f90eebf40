"""The opacity model of the two SDF renderers (threestudio/models/renderers/neus_volume_renderer.py:19-37, 93-117, 154-164) as tensor ops:
the learned variance, the VolSDF density, and alpha along a ray in its NeuS (logistic cdf) and VolSDF (|dt| sigma) forms.  These are the
composed routes of neus_renderer.py and volsdf_renderer.py; the fused routes evaluate the same model in csrc/ray_composite.h and csrc/neus.hip.
"""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn as nn
import torch.nn.functional as F


def volsdf_density(sdf: torch.Tensor, inv_std: torch.Tensor) -> torch.Tensor:
    """neus_volume_renderer.py:19-23"""
    inv_std = inv_std.clamp(0.0, 80.0)
    beta = 1 / inv_std
    return inv_std * (0.5 + 0.5 * sdf.sign() * torch.expm1(-sdf.abs() / beta))


class LearnedVariance(nn.Module):
    def __init__(self, init_val, requires_grad=True):
        super().__init__()
        self.register_parameter("_inv_std", nn.Parameter(torch.tensor(init_val), requires_grad=requires_grad))

    @property
    def inv_std(self):
        return torch.exp(self._inv_std * 10.0)

    def forward(self, x):
        return torch.ones_like(x) * self.inv_std.clamp(1.0e-6, 1.0e6)


def step_alpha(sdf: torch.Tensor, inv_std: torch.Tensor, step: float, use_volsdf: bool) -> torch.Tensor:
    """alpha_fn / occ_eval_fn (neus_volume_renderer.py:154-164, 366-376) as tensor ops"""
    if use_volsdf:
        return step * volsdf_density(sdf, inv_std)
    prev_cdf = torch.sigmoid((sdf + step * 0.5) * inv_std)
    next_cdf = torch.sigmoid((sdf - step * 0.5) * inv_std)
    return ((prev_cdf - next_cdf + 1e-5) / (prev_cdf + 1e-5)).clip(0.0, 1.0)


def get_alpha(sdf, normal, dirs, dists, inv_std, cos_anneal_ratio: float, use_volsdf: bool) -> torch.Tensor:
    """neus_volume_renderer.py:93-117 as tensor ops; sdf, dists [n, 1], normal, dirs [n, 3], inv_std broadcastable to sdf.
    VolSDF: alpha = |dt| * sigma(sdf); NeuS: the discrete opacity of the logistic cdf along the ray with the annealed cosine"""
    if use_volsdf:
        return torch.abs(dists.detach()) * volsdf_density(sdf, inv_std)
    true_cos = (dirs * normal).sum(-1, keepdim=True)
    iter_cos = -(F.relu(-true_cos * 0.5 + 0.5) * (1.0 - cos_anneal_ratio) + F.relu(-true_cos) * cos_anneal_ratio)   # always non-positive
    estimated_next_sdf = sdf + iter_cos * dists * 0.5
    estimated_prev_sdf = sdf - iter_cos * dists * 0.5
    prev_cdf = torch.sigmoid(estimated_prev_sdf * inv_std)
    next_cdf = torch.sigmoid(estimated_next_sdf * inv_std)
    return ((prev_cdf - next_cdf + 1e-5) / (prev_cdf + 1e-5)).clip(0.0, 1.0)


def kernel_color_act(material) -> Optional[int]:
    """the color_act of asd_neus_composite_* / asd_volsdf_composite_* when the material is colour = activation(features) with an activation
    the kernels carry, else None"""
    if not getattr(material, "elementwise", False) or getattr(material.cfg, "n_output_dims", None) != 3:
        return None
    name = getattr(material.cfg, "color_activation", None)
    name = "none" if name is None else str(name).lower()
    return {"none": 0, "sigmoid": 1}.get(name)
