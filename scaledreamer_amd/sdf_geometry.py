"""`implicit-sdf` geometry (threestudio/models/geometry/implicit_sdf.py:17-413) on the HIP path.

Module / parameter layout is the reference's (encoding / sdf_network / feature_network as nn.Modules with fp32 nn.Parameters, so a
reference checkpoint loads).  Two routes, as `implicit-volume` (geometry.py):
  fused      asd_field_fwd / asd_field_bwd / asd_field_density in ASD_FIELD_SDF mode (hash grid -> two 32 -> 64 -> 1 | 3 heads -> const or
             sphere bias -> forward-difference sdf_grad and normal in one kernel each way) — the same entries the hypernetwork geometry calls
  composed   tensor ops over the HIP hash-grid encoding: ellipsoid bias, finite_difference_laplacian, pred, a deformation network
Coarse-to-fine (Neuralangelo, implicit_sdf.py:380-413): with pos_encoding_config.otype "ProgressiveBandHashGrid" the encoding switches its
levels on by schedule (networks.ProgressiveBandHashGrid writes the level limit into the grid meta both routes read, the kernels skip the
masked levels), and finite_difference_normal_eps "progressive" shrinks the finite-difference step with the finest active level: update_step
writes it into the field cfg, so the route stays fused.
Not carried, each raising NotImplementedError with its reason: finite_difference_normal_eps "progressive" on any other encoding (the
reference asserts ProgressiveBandHashGrid there), shape_init "mesh:..." (needs trimesh and pysdf), normal_type "analytic" (the derivative of the hash grid w.r.t. the position exists for
`implicit-volume` only: asd_field_analytic_fwd / _bwd take ASD_FIELD_SDF cfgs, but this geometry is not wired to them).
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Any, Dict, Optional, Tuple, Union

import torch
import torch.nn.functional as F

from . import _lib, dist, ops
from .geometry import BaseImplicitGeometry, _SdfFieldFn, contract_to_unisphere, make_field_cfg, sdf_bias_mode, shifted_sdf
from .networks import VanillaMLP, get_encoding, get_mlp
from .registry import info, register, warn


@register("implicit-sdf")
class ImplicitSDF(BaseImplicitGeometry):
    @dataclass
    class Config(BaseImplicitGeometry.Config):
        n_input_dims: int = 3
        n_feature_dims: int = 3
        pos_encoding_config: dict = field(
            default_factory=lambda: {
                "otype": "HashGrid", "n_levels": 16, "n_features_per_level": 2, "log2_hashmap_size": 19,
                "base_resolution": 16, "per_level_scale": 1.447269237440378,
            }
        )
        mlp_network_config: dict = field(
            default_factory=lambda: {
                "otype": "VanillaMLP", "activation": "ReLU", "output_activation": "none", "n_neurons": 64,
                "n_hidden_layers": 1,
            }
        )
        normal_type: Optional[str] = "finite_difference"  # in ['pred', 'finite_difference', 'finite_difference_laplacian']
        finite_difference_normal_eps: Union[float, str] = 0.01
        shape_init: Optional[str] = None
        shape_init_params: Optional[Any] = None
        shape_init_mesh_up: str = "+z"
        shape_init_mesh_front: str = "+x"
        force_shape_init: bool = False
        sdf_bias: Union[float, str] = 0.0
        sdf_bias_params: Optional[Any] = None
        isosurface_remove_outliers: bool = False     # no need to remove outliers for an SDF

    cfg: Config
    SHAPE_INIT_STEPS = 1000

    def configure(self) -> None:
        super().configure()
        c = self.cfg
        if c.finite_difference_normal_eps == "progressive" and c.pos_encoding_config.get("otype", "HashGrid") != "ProgressiveBandHashGrid":
            raise NotImplementedError('finite_difference_normal_eps "progressive" only works with pos_encoding_config.otype '
                                      '"ProgressiveBandHashGrid" (the reference asserts it)')
        if isinstance(c.shape_init, str) and c.shape_init.startswith("mesh:"):
            raise NotImplementedError('shape_init "mesh:..." needs trimesh and pysdf, which this port does not use')
        if c.normal_type == "analytic":
            raise NotImplementedError('normal_type "analytic" needs the derivative of the hash grid w.r.t. the position, which only '
                                      '`implicit-volume` is wired to (asd_field_analytic_fwd); "finite_difference" is the fused route here')
        self.encoding = get_encoding(c.n_input_dims, c.pos_encoding_config)
        self.sdf_network = get_mlp(self.encoding.n_output_dims, 1, c.mlp_network_config)
        if c.n_feature_dims > 0:
            self.feature_network = get_mlp(self.encoding.n_output_dims, c.n_feature_dims, c.mlp_network_config)
        if c.normal_type == "pred":
            self.normal_network = get_mlp(self.encoding.n_output_dims, 3, c.mlp_network_config)
        if c.isosurface_deformable_grid:
            assert c.isosurface_method == "mt", "isosurface_deformable_grid only works with mt"
            self.deformation_network = get_mlp(self.encoding.n_output_dims, 3, c.mlp_network_config)
        self.finite_difference_normal_eps: Optional[float] = None
        self._meta = self.encoding.encoding.encoding.meta
        self._fcfg = self._make_field_cfg()

    # ---- fused-kernel eligibility (the conditions of ImplicitVolume._make_field_cfg) ----------------------------------------------
    def _make_field_cfg(self) -> Optional[_lib.FieldCfg]:
        c = self.cfg
        bias = sdf_bias_mode(c)
        if bias is None:
            return None
        mlp = c.mlp_network_config
        ok = (
            self._meta.n_levels == 16 and self.encoding.n_output_dims == 32 and not self.encoding.include_xyz
            and isinstance(self.sdf_network, VanillaMLP) and mlp.get("n_neurons") == 64 and mlp.get("n_hidden_layers") == 1
            and mlp.get("output_activation", "none") in (None, "none") and c.n_feature_dims in (0, 3)
            and c.normal_type in (None, "finite_difference") and c.n_input_dims == 3
            and (isinstance(c.finite_difference_normal_eps, float) or c.finite_difference_normal_eps == "progressive")
        )
        if not ok:
            return None
        # "progressive": update_step writes the step of the finest active level before anything asks for a normal (0.01, the config's
        # default, stands in until then)
        eps = float(c.finite_difference_normal_eps) if isinstance(c.finite_difference_normal_eps, float) else 0.01
        return make_field_cfg(c.radius, *bias, eps, c.n_feature_dims, _lib.ASD_FIELD_SDF)

    @property
    def fused(self) -> bool:
        return self._fcfg is not None

    def _weights(self):
        w1s, w2s = self.sdf_network.layers[0].weight, self.sdf_network.layers[2].weight
        if self.cfg.n_feature_dims > 0:
            return w1s, w2s, self.feature_network.layers[0].weight, self.feature_network.layers[2].weight
        return w1s, w2s, w1s, w2s  # dummies, never dereferenced when n_feature_dims == 0

    def _grid(self):
        return self.encoding.encoding.encoding.params

    def _wants_grad(self) -> bool:
        return torch.is_grad_enabled() and any(p.requires_grad for p in (self._grid(), *self._weights()))

    # ---- shape initialisation (implicit_sdf.py:91-222) ------------------------------------------------------------------------------
    def initialize_shape(self) -> None:
        c = self.cfg
        if c.shape_init is None and not c.force_shape_init:
            return
        if c.weights is not None and not c.force_shape_init:      # do not initialize shape if weights are provided
            return
        if c.sdf_bias != 0.0:
            warn("shape_init and sdf_bias are both specified, which may lead to unexpected results.")
        assert isinstance(c.shape_init, str)
        if c.shape_init == "ellipsoid":
            assert hasattr(c.shape_init_params, "__len__") and len(c.shape_init_params) == 3
            size = torch.as_tensor(list(c.shape_init_params), dtype=torch.float32).to(self._grid().device)
            get_gt_sdf = lambda p: ((p / size) ** 2).sum(dim=-1, keepdim=True).sqrt() - 1.0     # pseudo signed distance of an ellipsoid
        elif c.shape_init == "sphere":
            assert isinstance(c.shape_init_params, float)
            radius = c.shape_init_params
            get_gt_sdf = lambda p: (p ** 2).sum(dim=-1, keepdim=True).sqrt() - radius
        else:
            raise ValueError(f"Unknown shape initialization type: {c.shape_init}")
        optim = torch.optim.Adam(self.parameters(), lr=1e-3)
        dev = self._grid().device
        self.shape_init_losses = []          # device scalars, one per step (tests / tools)
        with torch.enable_grad():
            for _ in range(self.SHAPE_INIT_STEPS):
                points_rand = torch.rand((10000, 3), dtype=torch.float32).to(dev) * 2.0 - 1.0
                loss = F.mse_loss(self.forward_sdf(points_rand), get_gt_sdf(points_rand))
                optim.zero_grad()
                loss.backward()
                optim.step()
                self.shape_init_losses.append(loss.detach())
        if dist.is_distributed():            # explicit broadcast to ensure param consistency across ranks
            dist.broadcast_parameters(self, src=0)

    def get_shifted_sdf(self, points, sdf):
        return shifted_sdf(self.cfg, points, sdf)

    # ---- forward ----------------------------------------------------------------------------------------------------------------------
    def forward(self, points: torch.Tensor, output_normal: bool = False) -> Dict[str, torch.Tensor]:
        if self.fused and points.is_cuda and (self.cfg.normal_type is not None or not output_normal):
            return self._forward_fused(points, output_normal)
        return self._forward_composed(points, output_normal)

    def _forward_fused(self, points, output_normal):
        if output_normal:
            assert self.finite_difference_normal_eps is not None
        shape = points.shape[:-1]
        flat = points.reshape(-1, 3).contiguous().float()
        grid, ws = self._grid(), self._weights()
        if self._wants_grad():
            sdf, feats, normal, sdf_grad = _SdfFieldFn.apply(flat, grid, *ws, self._meta, self._fcfg, bool(output_normal))
        else:
            g, w = grid.detach(), [t.detach() for t in ws]
            if output_normal:
                sdf, feats, normal, sdf_grad, _ = ops.field_fwd(self._meta, self._fcfg, g, *w, flat, True, want_fd_grad=True)
            else:
                (sdf, feats, normal, _), sdf_grad = ops.field_fwd(self._meta, self._fcfg, g, *w, flat, False), None
        out = {"sdf": sdf.view(*shape, 1)}
        if self.cfg.n_feature_dims > 0:
            out["features"] = feats.view(*shape, self.cfg.n_feature_dims)
        if output_normal:
            n = normal.view(*shape, 3)
            out.update({"normal": n, "shading_normal": n, "sdf_grad": sdf_grad.view(*shape, 3)})
        return out

    def _forward_composed(self, points, output_normal):
        c = self.cfg
        points_unscaled = points
        pts = contract_to_unisphere(points, self.bbox, self.unbounded)
        enc = self.encoding(pts.view(-1, c.n_input_dims))
        sdf = self.get_shifted_sdf(points_unscaled, self.sdf_network(enc).view(*pts.shape[:-1], 1))
        out = {"sdf": sdf}
        if c.n_feature_dims > 0:
            out["features"] = self.feature_network(enc).view(*pts.shape[:-1], c.n_feature_dims)
        if output_normal:
            if c.normal_type in ("finite_difference", "finite_difference_laplacian"):
                assert self.finite_difference_normal_eps is not None
                eps = self.finite_difference_normal_eps
                if c.normal_type == "finite_difference_laplacian":
                    offs = torch.as_tensor([[eps, 0.0, 0.0], [-eps, 0.0, 0.0], [0.0, eps, 0.0], [0.0, -eps, 0.0], [0.0, 0.0, eps],
                                            [0.0, 0.0, -eps]]).to(points_unscaled)
                    so = self._forward_sdf_composed((points_unscaled[..., None, :] + offs).clamp(-c.radius, c.radius))
                    sdf_grad = 0.5 * (so[..., 0::2, 0] - so[..., 1::2, 0]) / eps
                else:
                    offs = torch.as_tensor([[eps, 0.0, 0.0], [0.0, eps, 0.0], [0.0, 0.0, eps]]).to(points_unscaled)
                    so = self._forward_sdf_composed((points_unscaled[..., None, :] + offs).clamp(-c.radius, c.radius))
                    sdf_grad = (so[..., 0::1, 0] - sdf) / eps
                normal = F.normalize(sdf_grad, dim=-1)
            elif c.normal_type == "pred":
                normal = F.normalize(self.normal_network(enc).view(*pts.shape[:-1], 3), dim=-1)
                sdf_grad = normal
            else:
                raise AttributeError(f"Unknown normal type {c.normal_type}")
            out.update({"normal": normal, "shading_normal": normal, "sdf_grad": sdf_grad})
        return out

    def _forward_sdf_composed(self, points):
        pts = contract_to_unisphere(points, self.bbox, self.unbounded)
        sdf = self.sdf_network(self.encoding(pts.reshape(-1, self.cfg.n_input_dims))).reshape(*pts.shape[:-1], 1)
        return self.get_shifted_sdf(points, sdf)

    def forward_sdf(self, points: torch.Tensor, n_dev: Optional[torch.Tensor] = None) -> torch.Tensor:
        """sdf [..., 1]: the no-grad sdf-only kernel when no gradient is wanted, the differentiable field entry otherwise.  n_dev
        (extension of the reference signature, no-grad fused route): int32 device scalar, the number of leading points that are valid."""
        if self.fused and points.is_cuda:
            flat = points.reshape(-1, 3).contiguous().float()
            grid, ws = self._grid(), self._weights()
            if self._wants_grad():
                sdf = _SdfFieldFn.apply(flat, grid, *ws, self._meta, self._fcfg, False)[0]
            else:
                sdf = ops.field_density(self._meta, self._fcfg, grid.detach(), ws[0].detach(), ws[1].detach(), flat, n_dev=n_dev)
            return sdf.view(*points.shape[:-1], 1)
        if n_dev is not None:
            raise ValueError("n_dev needs the fused field kernels")
        return self._forward_sdf_composed(points)

    # ---- isosurface / export --------------------------------------------------------------------------------------------------------
    def forward_field(self, points) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
        if not self.cfg.isosurface_deformable_grid:
            return self.forward_sdf(points), None
        pts = contract_to_unisphere(points, self.bbox, self.unbounded)
        enc = self.encoding(pts.reshape(-1, self.cfg.n_input_dims))
        sdf = self.get_shifted_sdf(points, self.sdf_network(enc).reshape(*pts.shape[:-1], 1))
        return sdf, self.deformation_network(enc).reshape(*pts.shape[:-1], 3)

    def forward_level(self, field, threshold):
        return field - threshold

    def export(self, points, **kwargs) -> Dict[str, Any]:
        out: Dict[str, Any] = {}
        if self.cfg.n_feature_dims == 0:
            return out
        if self.fused and points.is_cuda:
            out["features"] = self._forward_fused(points, False)["features"]
            return out
        pts = contract_to_unisphere(points, self.bbox, self.unbounded)
        enc = self.encoding(pts.reshape(-1, self.cfg.n_input_dims))
        out["features"] = self.feature_network(enc).view(*pts.shape[:-1], self.cfg.n_feature_dims)
        return out

    def update_step(self, epoch: int, global_step: int, on_load_weights: bool = False):
        if self.cfg.normal_type in ("finite_difference", "finite_difference_laplacian"):
            if isinstance(self.cfg.finite_difference_normal_eps, float):
                if self.finite_difference_normal_eps != self.cfg.finite_difference_normal_eps:
                    info(f"finite_difference_normal_eps = {self.cfg.finite_difference_normal_eps}")
                self.finite_difference_normal_eps = self.cfg.finite_difference_normal_eps
            elif self.cfg.finite_difference_normal_eps == "progressive":
                # progressive finite-difference eps from Neuralangelo (https://arxiv.org/abs/2306.03092): the cell of the finest active level
                hg = self.cfg.pos_encoding_config
                current_level = min(hg["start_level"] + max(global_step - hg["start_step"], 0) // hg["update_steps"], hg["n_levels"])
                grid_size = 2 * self.cfg.radius / (hg["base_resolution"] * hg["per_level_scale"] ** (current_level - 1))
                if grid_size != self.finite_difference_normal_eps:
                    info(f"Update finite_difference_normal_eps to {grid_size}")
                self.finite_difference_normal_eps = grid_size
                if self._fcfg is not None:
                    self._fcfg.fd_eps = grid_size
            else:
                raise ValueError(f"Unknown finite_difference_normal_eps={self.cfg.finite_difference_normal_eps}")
