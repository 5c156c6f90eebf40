"""The reference's backgrounds on the HIP path: `neural-environment-map-background`
(threestudio/models/background/neural_environment_map_background.py:15-67), `solid-color-background` (solid_color_background.py:13-51)
and `textured-background` (textured_background.py:13-54)."""
from __future__ import annotations

import math
import random
from dataclasses import dataclass, field
from typing import Optional, Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib, ops
from .base import BaseModule
from .networks import VanillaMLP, get_activation, get_encoding, get_mlp
from .registry import register


class BaseBackground(BaseModule):
    @dataclass
    class Config(BaseModule.Config):
        pass

    cfg: Config

    def configure(self):
        pass

    def forward(self, dirs: torch.Tensor) -> torch.Tensor:
        raise NotImplementedError


class _EnvMapFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, dirs, grid, w0, w1, w2, meta):
        color = ops.envmap_fwd(meta, grid, w0, w1, w2, dirs)
        ctx.save_for_backward(dirs, grid, w0, w1, w2)
        ctx.meta = meta
        return color

    @staticmethod
    def backward(ctx, d_color):
        dirs, grid, w0, w1, w2 = ctx.saved_tensors
        dgrid, dw0, dw1, dw2 = ops.envmap_bwd(ctx.meta, grid, w0, w1, w2, dirs, d_color.contiguous())
        return None, dgrid, dw0, dw1, dw2, None


@register("neural-environment-map-background")
class NeuralEnvironmentMapBackground(BaseBackground):
    @dataclass
    class Config(BaseBackground.Config):
        n_output_dims: int = 3
        color_activation: str = "sigmoid"
        dir_encoding_config: dict = field(default_factory=lambda: {"otype": "SphericalHarmonics", "degree": 3})
        mlp_network_config: dict = field(
            default_factory=lambda: {"otype": "VanillaMLP", "activation": "ReLU", "n_neurons": 16, "n_hidden_layers": 2}
        )
        random_aug: bool = False
        random_aug_prob: float = 0.5
        eval_color: Optional[Tuple[float, float, float]] = None

    cfg: Config

    def configure(self) -> None:
        self.encoding = get_encoding(3, self.cfg.dir_encoding_config)
        self.network = get_mlp(self.encoding.n_output_dims, self.cfg.n_output_dims, self.cfg.mlp_network_config)
        m = self.cfg.mlp_network_config
        self._meta = getattr(self.encoding.encoding.encoding, "meta", None)   # None: parameter-free encodings (SphericalHarmonics)
        self._fused = (
            self._meta is not None and self._meta.n_levels == 4 and not self.encoding.include_xyz and isinstance(self.network, VanillaMLP)
            and m.get("n_neurons") == 16 and m.get("n_hidden_layers") == 2 and self.cfg.n_output_dims == 3
            and self.cfg.color_activation == "sigmoid" and m.get("output_activation", "none") in (None, "none")
        )
        # injectable RNG hooks: tests replace these to pin "identical inputs"
        self.rand_fn = random.random
        self.rand_color_fn = lambda b, c: torch.rand(b, 1, 1, c)

    def forward(self, dirs: torch.Tensor) -> torch.Tensor:
        if not self.training and self.cfg.eval_color is not None:
            return torch.ones(*dirs.shape[:-1], self.cfg.n_output_dims).to(dirs) * torch.as_tensor(self.cfg.eval_color).to(dirs)
        if self._fused and dirs.is_cuda:
            flat = dirs.reshape(-1, 3).contiguous().float()
            grid = self.encoding.encoding.encoding.params
            w0, w1, w2 = (self.network.layers[i].weight for i in (0, 2, 4))
            if torch.is_grad_enabled() and grid.requires_grad:
                color = _EnvMapFn.apply(flat, grid, w0, w1, w2, self._meta)
            else:
                color = ops.envmap_fwd(self._meta, grid.detach(), w0.detach(), w1.detach(), w2.detach(), flat)
            color = color.view(*dirs.shape[:-1], 3)
        else:
            d01 = (dirs + 1.0) / 2.0
            color = self.network(self.encoding(d01.view(-1, 3))).view(*dirs.shape[:-1], self.cfg.n_output_dims)
            color = get_activation(self.cfg.color_activation)(color)
        if self.training and self.cfg.random_aug and self.rand_fn() < self.cfg.random_aug_prob:
            # random solid colour; `color * 0 +` keeps every parameter in the autograd graph (DDP)
            rc = self.rand_color_fn(dirs.shape[0], self.cfg.n_output_dims)      # host RNG, as in the reference (its draw order is the contract)
            if dirs.is_cuda and not rc.is_cuda:
                # through pinned memory, asynchronously: a pageable .to(device) blocks the host until the stream reaches the copy —
                # every second step (random_aug_prob = 0.5) the host lost the lead it has over the GPU
                rc = rc.pin_memory().to(dirs.device, non_blocking=True)
            color = color * 0 + rc.to(dirs).expand(*dirs.shape[:-1], -1)
        return color


def _upload_colors(rc: torch.Tensor, dirs: torch.Tensor) -> torch.Tensor:
    """the host-drawn random colours on the device of `dirs`: through pinned memory, asynchronously (see NeuralEnvironmentMapBackground)"""
    if dirs.is_cuda and not rc.is_cuda:
        rc = rc.pin_memory().to(dirs.device, non_blocking=True)
    return rc.to(dirs)


class _SolidFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, colors, rays_per_view):
        ctx.n_views = colors.shape[0]
        return ops.bg_solid_fwd(colors, rays_per_view)

    @staticmethod
    def backward(ctx, d_out):
        return ops.bg_solid_bwd(d_out.contiguous(), ctx.n_views), None


@register("solid-color-background")
class SolidColorBackground(BaseBackground):
    @dataclass
    class Config(BaseBackground.Config):
        n_output_dims: int = 3
        color: Tuple = (1.0, 1.0, 1.0)
        learned: bool = False
        random_aug: bool = False
        random_aug_prob: float = 0.5

    cfg: Config

    def configure(self) -> None:
        color = torch.as_tensor(self.cfg.color, dtype=torch.float32)
        if self.cfg.learned:
            self.env_color = nn.Parameter(color)
        else:
            self.register_buffer("env_color", color)
        # injectable RNG hooks, as NeuralEnvironmentMapBackground's: tests replace these to pin "identical inputs"
        self.rand_fn = random.random
        self.rand_color_fn = lambda b, c: torch.rand(b, 1, 1, c)

    def forward(self, dirs: torch.Tensor) -> torch.Tensor:
        C = self.cfg.n_output_dims
        aug = self.training and self.cfg.random_aug and self.rand_fn() < self.cfg.random_aug_prob
        rc = self.rand_color_fn(dirs.shape[0], C) if aug else None      # host RNG, in the reference's draw order
        if not dirs.is_cuda:
            color = torch.ones(*dirs.shape[:-1], C).to(dirs) * self.env_color.to(dirs)
            if aug:
                color = color * 0 + rc.to(dirs).expand(*dirs.shape[:-1], -1)
            return color
        colors = self.env_color.float().expand(C).reshape(1, C)         # (a one-value colour broadcasts over the channels, as `ones * env_color`)
        n = math.prod(dirs.shape[:-1])
        if aug:
            # `color * 0 +`: the learned colour stays in the graph and receives a zero gradient
            colors = colors * 0 + _upload_colors(rc, dirs).float().reshape(dirs.shape[0], C)
        rays = n // colors.shape[0]
        if torch.is_grad_enabled() and colors.requires_grad:
            color = _SolidFn.apply(colors.contiguous(), rays)
        else:
            color = ops.bg_solid_fwd(colors.detach(), rays)
        return color.view(*dirs.shape[:-1], C).to(dirs.dtype)


class _TextureFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, dirs, texture, act):
        ctx.save_for_backward(dirs, texture)
        ctx.act = act
        return ops.bg_texture_fwd(texture, dirs, act)

    @staticmethod
    def backward(ctx, d_color):
        dirs, texture = ctx.saved_tensors
        return None, ops.bg_texture_bwd(texture, dirs, d_color.contiguous(), ctx.act), None


@register("textured-background")
class TexturedBackground(BaseBackground):
    @dataclass
    class Config(BaseBackground.Config):
        n_output_dims: int = 3
        height: int = 64
        width: int = 64
        color_activation: str = "sigmoid"

    cfg: Config

    # activations the kernels apply themselves; any other name runs them with "none" and composes get_activation on top
    _FUSED_ACTS = {"sigmoid": _lib.ASD_BG_ACT_SIGMOID, "none": _lib.ASD_BG_ACT_NONE, None: _lib.ASD_BG_ACT_NONE}

    def configure(self) -> None:
        self.texture = nn.Parameter(torch.randn((1, self.cfg.n_output_dims, self.cfg.height, self.cfg.width)))

    @staticmethod
    def spherical_xyz_to_uv(dirs: torch.Tensor) -> torch.Tensor:
        x, y, z = dirs[..., 0], dirs[..., 1], dirs[..., 2]
        xy = (x**2 + y**2) ** 0.5
        u = torch.atan2(xy, z) / torch.pi
        v = torch.atan2(y, x) / (torch.pi * 2) + 0.5
        return torch.stack([u, v], -1)

    def forward(self, dirs: torch.Tensor) -> torch.Tensor:
        C = self.cfg.n_output_dims
        name = self.cfg.color_activation
        name = name.lower() if isinstance(name, str) else name
        if not dirs.is_cuda:
            uv = 2 * self.spherical_xyz_to_uv(dirs.reshape(-1, dirs.shape[-1])) - 1
            color = F.grid_sample(self.texture.to(dirs.dtype), uv.reshape(1, -1, 1, 2), mode="bilinear", padding_mode="reflection", align_corners=False)
            color = color.reshape(C, -1).T.reshape(*dirs.shape[:-1], C)
            return get_activation(name)(color)
        act = self._FUSED_ACTS.get(name)
        flat = dirs.reshape(-1, 3).contiguous().float()
        if torch.is_grad_enabled() and self.texture.requires_grad:
            color = _TextureFn.apply(flat, self.texture, _lib.ASD_BG_ACT_NONE if act is None else act)
        else:
            color = ops.bg_texture_fwd(self.texture.detach(), flat, _lib.ASD_BG_ACT_NONE if act is None else act)
        if act is None:
            color = get_activation(name)(color)
        return color.view(*dirs.shape[:-1], C).to(dirs.dtype)
