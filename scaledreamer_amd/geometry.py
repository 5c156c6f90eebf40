"""`implicit-volume` geometry (threestudio/models/geometry/implicit_volume.py:19-207) on the HIP path.

Module / parameter layout is the reference's (encoding / density_network / feature_network as nn.Modules
with fp32 nn.Parameters — the optimizer addresses them by dotted name, systems/utils.py:19-39); the
arithmetic of forward()/forward_density() runs in the fused HIP field kernels when the configuration is
the one those kernels are built for, otherwise in the composed path (HIP hash grid + torch VanillaMLP).
"""
from __future__ import annotations

from dataclasses import dataclass, field
from functools import partial
from typing import Any, Dict, Optional, Tuple, Union

import torch
import torch.nn.functional as F

from . import _lib, ops
from .base import BaseModule
from .networks import VanillaMLP, get_activation, get_encoding, get_mlp
from .registry import debug, info, register, warn


def scale_tensor(dat, inp_scale, tgt_scale):
    """threestudio/utils/ops.py:27-38"""
    if inp_scale is None:
        inp_scale = (0, 1)
    if tgt_scale is None:
        tgt_scale = (0, 1)
    dat = (dat - inp_scale[0]) / (inp_scale[1] - inp_scale[0])
    return dat * (tgt_scale[1] - tgt_scale[0]) + tgt_scale[0]


def contract_to_unisphere(x, bbox, unbounded: bool = False):
    """threestudio/models/geometry/base.py:20-32"""
    if unbounded:
        x = scale_tensor(x, bbox, (0, 1))
        x = x * 2 - 1
        mag = x.norm(dim=-1, keepdim=True)
        mask = mag.squeeze(-1) > 1
        x[mask] = (2 - 1 / mag[mask]) * (x[mask] / mag[mask])
        return x / 4 + 0.5
    return scale_tensor(x, bbox, (0, 1))


class BaseImplicitGeometry(BaseModule):
    @dataclass
    class Config(BaseModule.Config):
        radius: float = 1.0
        isosurface: bool = True
        isosurface_method: str = "mt"
        isosurface_resolution: int = 128
        isosurface_threshold: Union[float, str] = 0.0
        isosurface_chunk: int = 0
        isosurface_coarse_to_fine: bool = True
        isosurface_deformable_grid: bool = False
        isosurface_remove_outliers: bool = True
        isosurface_outlier_n_faces_threshold: Union[int, float] = 0.01

    cfg: Config

    def configure(self) -> None:
        r = self.cfg.radius
        self.register_buffer("bbox", torch.as_tensor([[-r, -r, -r], [r, r, r]], dtype=torch.float32))
        self.isosurface_helper = None
        self.unbounded = False

    # ---- mesh extraction (geometry/base.py:85-188) ------------------------------------------------
    def _initilize_isosurface_helper(self):
        if not self.cfg.isosurface or self.isosurface_helper is not None:
            return
        import os

        from .isosurface import MarchingTetrahedraGridHelper, MarchingTetrahedraHelper

        method, res = self.cfg.isosurface_method, self.cfg.isosurface_resolution
        if method == "mt":
            path = f"load/tets/{res}_tets.npz"
            if not os.path.exists(path):
                raise FileNotFoundError(f'isosurface_method "mt" needs the tetrahedral grid {path}, which is not there; '
                                        'isosurface_method "mt-grid" runs marching tetrahedra over a regular grid and needs no file')
            self.isosurface_helper = MarchingTetrahedraHelper(res, path).to(self.device)
        elif method == "mt-grid":
            self.isosurface_helper = MarchingTetrahedraGridHelper(res).to(self.device)
        elif method == "mc-cpu":
            raise NotImplementedError('isosurface_method "mc-cpu" needs PyMCubes, which this port does not use; '
                                      '"mt-grid" is the method that needs no file')
        else:
            raise AttributeError(f"Unknown isosurface method {method}")

    def forward_field(self, points):
        raise NotImplementedError

    def forward_level(self, field, threshold):
        raise NotImplementedError

    def _isosurface(self, bbox: torch.Tensor, fine_stage: bool = False):
        helper = self.isosurface_helper
        assert helper is not None
        grid = helper.grid_vertices
        chunk = self.cfg.isosurface_chunk if self.cfg.isosurface_chunk > 0 else grid.shape[0]
        fields, deformations = [], []
        for i in range(0, grid.shape[0], chunk):       # chunk_batch(batch_func, isosurface_chunk, grid_vertices), base.py:120-140
            x = grid[i:i + chunk]
            f, d = self.forward_field(scale_tensor(x.to(bbox.device), helper.points_range, bbox))
            fields.append(f.to(x.device))
            deformations.append(None if d is None else d.to(x.device))
        field = torch.cat(fields, dim=0)
        deformation = None if deformations[0] is None else torch.cat(deformations, dim=0)
        if isinstance(self.cfg.isosurface_threshold, float):
            threshold = self.cfg.isosurface_threshold
        elif self.cfg.isosurface_threshold == "auto":
            eps = 1.0e-5
            threshold = field[field > eps].mean().item()
            info(f"Automatically determined isosurface threshold: {threshold}")
        else:
            raise TypeError(f"Unknown isosurface_threshold {self.cfg.isosurface_threshold}")
        level = self.forward_level(field, threshold)
        mesh = helper(level, deformation=deformation)
        mesh.v_pos = scale_tensor(mesh.v_pos, helper.points_range, bbox)
        mesh.add_extra("bbox", bbox)
        if self.cfg.isosurface_remove_outliers:
            mesh = mesh.remove_outlier(self.cfg.isosurface_outlier_n_faces_threshold)
        return mesh

    def isosurface(self):
        if not self.cfg.isosurface:
            raise NotImplementedError("Isosurface is not enabled in the current configuration")
        self._initilize_isosurface_helper()
        if self.cfg.isosurface_coarse_to_fine:
            debug("First run isosurface to get a tight bounding box ...")
            with torch.no_grad():
                mesh_coarse = self._isosurface(self.bbox)
            if mesh_coarse.v_pos.shape[0] == 0:
                raise ValueError("the coarse isosurface pass found no surface: no grid edge crosses isosurface_threshold "
                                 f"{self.cfg.isosurface_threshold!r}")
            vmin, vmax = mesh_coarse.v_pos.amin(dim=0), mesh_coarse.v_pos.amax(dim=0)
            vmin_ = (vmin - (vmax - vmin) * 0.1).max(self.bbox[0])
            vmax_ = (vmax + (vmax - vmin) * 0.1).min(self.bbox[1])
            debug("Run isosurface again with the tight bounding box ...")
            with torch.no_grad():       # the extracted mesh is not differentiable here (no DMTet stage): no graph over the grid's field values
                return self._isosurface(torch.stack([vmin_, vmax_], dim=0), fine_stage=True)
        with torch.no_grad():
            return self._isosurface(self.bbox)


def make_field_cfg(radius: float, bias_mode: int, bias_value: float, fd_eps: float, n_feature_dims: int, field_mode: int,
                   activation: int = _lib.ASD_ACT_NONE, blob_scale: float = 0.0, blob_std: float = 1.0) -> _lib.FieldCfg:
    """The ONE place an asd_field_cfg is filled, for every geometry on the field kernels (a field added to the struct is set here or is
    zero everywhere).  activation / blob_scale / blob_std are the density case's; an SDF cfg leaves them at their neutral values."""
    f = _lib.FieldCfg()
    for d in range(3):
        f.bbox_min[d], f.bbox_max[d] = -radius, radius
    f.radius, f.bias_mode, f.bias_value = radius, bias_mode, bias_value
    f.blob_scale, f.blob_std, f.activation = blob_scale, blob_std, activation
    f.fd_eps, f.n_hidden, f.n_feature_dims, f.field_mode = fd_eps, 64, n_feature_dims, field_mode
    return f


def sdf_bias_mode(cfg) -> Optional[Tuple[int, float]]:
    """(bias mode, bias value) of sdf_bias / sdf_bias_params as the field kernels apply it; None for a bias they do not (ellipsoid)"""
    if cfg.sdf_bias == "sphere" and isinstance(cfg.sdf_bias_params, float):
        return _lib.ASD_BIAS_SPHERE, float(cfg.sdf_bias_params)
    if isinstance(cfg.sdf_bias, float):
        return _lib.ASD_BIAS_CONST, float(cfg.sdf_bias)
    return None


def shifted_sdf(cfg, points, sdf):
    """get_shifted_sdf of the four SDF geometries (implicit_sdf.py:224, and its copies hyper_iNGP.py:206, stylegan_3dconv_net.py:201,
    triplane_transformer.py:104); the ellipsoid parameters may be any sequence of three"""
    if cfg.sdf_bias == "ellipsoid":
        assert hasattr(cfg.sdf_bias_params, "__len__") and len(cfg.sdf_bias_params) == 3
        size = torch.as_tensor(list(cfg.sdf_bias_params)).to(points)
        bias = ((points / size) ** 2).sum(dim=-1, keepdim=True).sqrt() - 1.0
    elif cfg.sdf_bias == "sphere":
        assert isinstance(cfg.sdf_bias_params, float)
        bias = (points ** 2).sum(dim=-1, keepdim=True).sqrt() - cfg.sdf_bias_params
    elif isinstance(cfg.sdf_bias, float):
        bias = cfg.sdf_bias
    else:
        raise ValueError(f"Unknown sdf bias {cfg.sdf_bias}")
    return sdf + bias


def _contiguous(t):
    return None if t is None else t.contiguous()


class _FieldFn(torch.autograd.Function):
    """sigma, features, normal = field(points) around the ops pair it is handed: (ops.field_fwd, ops.field_bwd) with their want_normal /
    n_dev bound — backward scatters into the table and reduces MLP grads — or (ops.field_analytic_fwd, ops.field_analytic_bwd), where
    normal = -grad sigma / |grad sigma| from the field's own position derivative (normal_type "analytic") and backward is the double
    backward of the reference's autograd.grad(..., create_graph=True)."""

    @staticmethod
    def forward(ctx, points, grid, w1d, w2d, w1f, w2f, geom, fwd, bwd):
        sigma, feats, normal, enc = fwd(geom._meta, geom._fcfg, grid, w1d, w2d, w1f, w2f, points)
        ctx.save_for_backward(points, grid, w1d, w2d, w1f, w2f, enc, sigma)
        ctx.geom, ctx.bwd = geom, bwd
        ctx.set_materialize_grads(False)
        if normal is None:
            normal = sigma.new_zeros(0)
            ctx.mark_non_differentiable(normal)
        return sigma, feats, normal

    @staticmethod
    def backward(ctx, d_sigma, d_feats, d_normal):
        points, grid, w1d, w2d, w1f, w2f, enc, sigma = ctx.saved_tensors
        g = ctx.geom
        d_grid = torch.zeros_like(grid)
        if d_sigma is None and d_feats is None and d_normal is None:
            return None, d_grid, torch.zeros_like(w1d), torch.zeros_like(w2d), torch.zeros_like(w1f), torch.zeros_like(w2f), None, None, None
        dw = ctx.bwd(g._meta, g._fcfg, grid, w1d, w2d, w1f, w2f, points, enc, sigma, _contiguous(d_sigma), _contiguous(d_feats),
                     _contiguous(d_normal), d_grid)
        return None, d_grid, dw[0], dw[1], dw[2], dw[3], None, None, None


class _SdfFieldFn(torch.autograd.Function):
    """(sdf, features, normal, sdf_grad) of ONE field evaluation in ASD_FIELD_SDF mode (fused HIP kernels): `implicit-sdf` with its own heads,
    `Hyper-iNGP` with one prompt's hypernetwork weights."""

    @staticmethod
    def forward(ctx, points, grid, w1d, w2d, w1f, w2f, meta, fcfg, want_normal):
        if want_normal:
            sdf, feats, normal, fdg, enc = ops.field_fwd(meta, fcfg, grid, w1d, w2d, w1f, w2f, points, True, want_fd_grad=True)
        else:
            sdf, feats, normal, enc = ops.field_fwd(meta, fcfg, grid, w1d, w2d, w1f, w2f, points, False)
            normal, fdg = sdf.new_zeros(0), sdf.new_zeros(0)
            ctx.mark_non_differentiable(normal, fdg)
        ctx.save_for_backward(points, grid, w1d, w2d, w1f, w2f, enc, sdf)
        ctx.meta, ctx.fcfg, ctx.want_normal = meta, fcfg, want_normal
        ctx.set_materialize_grads(False)
        return sdf, feats, normal, fdg

    @staticmethod
    def backward(ctx, d_sdf, d_feats, d_normal, d_fdg):
        points, grid, w1d, w2d, w1f, w2f, enc, sdf = ctx.saved_tensors
        d_grid = torch.zeros_like(grid)
        if d_sdf is None and d_feats is None and d_normal is None and d_fdg is None:
            return (None, d_grid, *(torch.zeros_like(w) for w in (w1d, w2d, w1f, w2f)), None, None, None)
        c = _contiguous
        dw = ops.field_bwd(ctx.meta, ctx.fcfg, grid, w1d, w2d, w1f, w2f, points, enc, sdf, c(d_sdf), c(d_feats),
                           c(d_normal) if ctx.want_normal else None, d_grid, d_fd_grad=c(d_fdg) if ctx.want_normal else None)
        return None, d_grid, dw[0], dw[1], dw[2], dw[3], None, None, None


@register("implicit-volume")
class ImplicitVolume(BaseImplicitGeometry):
    @dataclass
    class Config(BaseImplicitGeometry.Config):
        n_input_dims: int = 3
        n_feature_dims: int = 3
        density_activation: Optional[str] = "softplus"
        density_bias: Union[float, str] = "blob_magic3d"
        density_blob_scale: float = 10.0
        density_blob_std: float = 0.5
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
        normal_type: Optional[str] = "finite_difference"
        finite_difference_normal_eps: float = 0.01
        isosurface_threshold: Union[float, str] = 25.0
        anneal_density_blob_std_config: Optional[dict] = None

    cfg: Config

    def configure(self) -> None:
        super().configure()
        self.encoding = get_encoding(self.cfg.n_input_dims, self.cfg.pos_encoding_config)
        self.density_network = get_mlp(self.encoding.n_output_dims, 1, self.cfg.mlp_network_config)
        if self.cfg.n_feature_dims > 0:
            self.feature_network = get_mlp(self.encoding.n_output_dims, self.cfg.n_feature_dims, self.cfg.mlp_network_config)
        if self.cfg.normal_type == "pred":
            self.normal_network = get_mlp(self.encoding.n_output_dims, 3, self.cfg.mlp_network_config)
        self._meta = self.encoding.encoding.encoding.meta
        self._fcfg = self._make_field_cfg()
        if self.cfg.normal_type == "analytic" and self.cfg.pos_encoding_config.get("otype", "HashGrid") == "ProgressiveBandHashGrid":
            raise NotImplementedError('normal_type "analytic" with a ProgressiveBandHashGrid: the analytic field kernels take no level limit '
                                      "(asd_field_analytic_fwd returns ASD_ERR_UNSUPPORTED for a masked grid); use finite-difference normals")
        if self.cfg.normal_type == "analytic" and self._fcfg is None:
            raise NotImplementedError('normal_type "analytic" exists on the fused field kernels only (the composed route\'s encoding has no '
                                      "derivative with respect to the position); this configuration is kept off them by: "
                                      + ", ".join(self._fused_blockers))

    # ---- fused-kernel eligibility ---------------------------------------------------------------
    def _make_field_cfg(self) -> Optional[_lib.FieldCfg]:
        c = self.cfg
        act = {"softplus": _lib.ASD_ACT_SOFTPLUS, "exp": _lib.ASD_ACT_EXP, "trunc_exp": _lib.ASD_ACT_TRUNC_EXP,
               None: _lib.ASD_ACT_NONE, "none": _lib.ASD_ACT_NONE}.get(c.density_activation, -1)
        if isinstance(c.density_bias, str):
            bias = {"blob_magic3d": _lib.ASD_BIAS_BLOB_MAGIC3D, "blob_dreamfusion": _lib.ASD_BIAS_BLOB_DREAMFUSION}.get(c.density_bias, -1)
            bias_value = 0.0
        else:
            bias, bias_value = _lib.ASD_BIAS_CONST, float(c.density_bias)
        mlp = c.mlp_network_config
        # what keeps a configuration off the fused kernels, by name (configure() quotes them when normal_type "analytic" needs the kernels)
        blockers = [why for cond, why in (
            (act >= 0, f"density_activation {c.density_activation!r}"),
            (bias >= 0, f"density_bias {c.density_bias!r}"),
            (self._meta.n_levels == 16 and self.encoding.n_output_dims == 32, "a hash grid other than 16 levels x 2 features"),
            (not self.encoding.include_xyz, "include_xyz"),
            (isinstance(self.density_network, VanillaMLP), "a density network that is not a VanillaMLP"),
            (mlp.get("n_neurons") == 64, f"n_neurons {mlp.get('n_neurons')} (the kernels are built for 64)"),
            (mlp.get("n_hidden_layers") == 1, f"n_hidden_layers {mlp.get('n_hidden_layers')} (the kernels are built for 1)"),
            (mlp.get("output_activation", "none") in (None, "none"), f"output_activation {mlp.get('output_activation')!r}"),
            (c.n_feature_dims in (0, 3), f"n_feature_dims {c.n_feature_dims}"),
            (c.normal_type in (None, "finite_difference", "analytic"), f"normal_type {c.normal_type!r}"),
            (c.n_input_dims == 3, f"n_input_dims {c.n_input_dims}"),
        ) if not cond]
        self._fused_blockers = blockers
        if blockers:
            return None
        return make_field_cfg(c.radius, bias, bias_value, c.finite_difference_normal_eps, c.n_feature_dims, _lib.ASD_FIELD_DENSITY,
                              activation=act, blob_scale=c.density_blob_scale, blob_std=c.density_blob_std)

    @property
    def fused(self) -> bool:
        return self._fcfg is not None

    def _weights(self):
        w1d, w2d = self.density_network.layers[0].weight, self.density_network.layers[2].weight
        if self.cfg.n_feature_dims > 0:
            return w1d, w2d, self.feature_network.layers[0].weight, self.feature_network.layers[2].weight
        return w1d, w2d, w1d, w2d  # dummies, never dereferenced when n_feature_dims == 0

    # ---- reference surface ----------------------------------------------------------------------
    def get_activated_density(self, points, density):
        c = self.cfg
        if c.density_bias == "blob_dreamfusion":
            bias = c.density_blob_scale * torch.exp(-0.5 * (points**2).sum(dim=-1) / c.density_blob_std**2)[..., None]
        elif c.density_bias == "blob_magic3d":
            bias = c.density_blob_scale * (1 - torch.sqrt((points**2).sum(dim=-1)) / c.density_blob_std)[..., None]
        elif isinstance(c.density_bias, float):
            bias = c.density_bias
        else:
            raise ValueError(f"Unknown density bias {c.density_bias}")
        raw = density + bias
        return raw, get_activation(c.density_activation)(raw)

    def forward(self, points: torch.Tensor, output_normal: bool = False, n_dev: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
        """n_dev (extension of the reference signature, fused path only): int32 device scalar — only the first n_dev points are valid,
        the rows behind them are neither read nor written (the renderer's capacity-sized sample buffers, no host read of the count)"""
        if self.fused and points.is_cuda:
            return self._forward_fused(points, output_normal, n_dev)
        if n_dev is not None:
            raise ValueError("n_dev needs the fused field kernels")
        return self._forward_composed(points, output_normal)

    def _forward_fused(self, points, output_normal, n_dev=None):
        if output_normal and self.cfg.normal_type is None:
            raise AttributeError(f"Unknown normal type {self.cfg.normal_type}")
        shape = points.shape[:-1]
        flat = points.reshape(-1, 3).contiguous().float()
        w1d, w2d, w1f, w2f = self._weights()
        grid = self.encoding.encoding.encoding.params
        if output_normal and self.cfg.normal_type == "analytic":
            if n_dev is not None:
                raise ValueError('normal_type "analytic" takes no n_dev: the renderer path with a device-side sample count never asks for normals')
            if torch.is_grad_enabled() and grid.requires_grad:
                sigma, feats, normal = _FieldFn.apply(flat, grid, w1d, w2d, w1f, w2f, self, ops.field_analytic_fwd, ops.field_analytic_bwd)
            else:       # detached, as the reference detaches the normal when grad was disabled (implicit_volume.py:189-190)
                sigma, feats, normal, _ = ops.field_analytic_fwd(self._meta, self._fcfg, grid.detach(), w1d.detach(), w2d.detach(),
                                                                 w1f.detach(), w2f.detach(), flat)
        elif torch.is_grad_enabled() and grid.requires_grad:
            fwd, bwd = partial(ops.field_fwd, want_normal=bool(output_normal), n_dev=n_dev), partial(ops.field_bwd, n_dev=n_dev)
            sigma, feats, normal = _FieldFn.apply(flat, grid, w1d, w2d, w1f, w2f, self, fwd, bwd)
        else:
            sigma, feats, normal, _ = ops.field_fwd(self._meta, self._fcfg, grid.detach(), w1d.detach(), w2d.detach(),
                                                    w1f.detach(), w2f.detach(), flat, bool(output_normal), n_dev=n_dev)
        out = {"density": sigma.view(*shape, 1)}
        if self.cfg.n_feature_dims > 0:
            out["features"] = feats.view(*shape, self.cfg.n_feature_dims)
        if output_normal:
            n = normal.view(*shape, 3)
            out.update({"normal": n, "shading_normal": n})
        return out

    def _forward_composed(self, points, output_normal):
        c = self.cfg
        points_unscaled = points
        pts = contract_to_unisphere(points, self.bbox, self.unbounded)
        enc = self.encoding(pts.view(-1, c.n_input_dims))
        density = self.density_network(enc).view(*pts.shape[:-1], 1)
        _, density = self.get_activated_density(points_unscaled, density)
        out = {"density": density}
        if c.n_feature_dims > 0:
            out["features"] = self.feature_network(enc).view(*pts.shape[:-1], c.n_feature_dims)
        if output_normal:
            if c.normal_type in ("finite_difference", "finite_difference_laplacian"):
                eps = c.finite_difference_normal_eps
                if c.normal_type == "finite_difference_laplacian":
                    offs = torch.as_tensor([[eps, 0, 0], [-eps, 0, 0], [0, eps, 0], [0, -eps, 0], [0, 0, eps], [0, 0, -eps]]).to(points_unscaled)
                    po = (points_unscaled[..., None, :] + offs).clamp(-c.radius, c.radius)
                    do = self.forward_density(po)
                    normal = -0.5 * (do[..., 0::2, 0] - do[..., 1::2, 0]) / eps
                else:
                    offs = torch.as_tensor([[eps, 0.0, 0.0], [0.0, eps, 0.0], [0.0, 0.0, eps]]).to(points_unscaled)
                    po = (points_unscaled[..., None, :] + offs).clamp(-c.radius, c.radius)
                    do = self.forward_density(po)
                    normal = -(do[..., 0::1, 0] - density) / eps
                normal = F.normalize(normal, dim=-1)
            elif c.normal_type == "pred":
                normal = F.normalize(self.normal_network(enc).view(*pts.shape[:-1], 3), dim=-1)
            else:
                raise AttributeError(f"Unknown normal type {c.normal_type}")
            out.update({"normal": normal, "shading_normal": normal})
        return out

    def forward_density(self, points: torch.Tensor, n_dev: Optional[torch.Tensor] = None) -> torch.Tensor:
        """n_dev (extension of the reference signature): int32 device scalar, the number of leading points that are valid — the
        renderer passes capacity-sized candidate buffers and the marcher's device-side count instead of reading the count back."""
        if self.fused and points.is_cuda and not (torch.is_grad_enabled() and self.encoding.encoding.encoding.params.requires_grad):
            w1d, w2d, _, _ = self._weights()
            grid = self.encoding.encoding.encoding.params
            flat = points.reshape(-1, 3).contiguous().float()
            s = ops.field_density(self._meta, self._fcfg, grid.detach(), w1d.detach(), w2d.detach(), flat, n_dev=n_dev)
            return s.view(*points.shape[:-1], 1)
        if self.fused and points.is_cuda:
            return self._forward_fused(points, False)["density"]
        pts = contract_to_unisphere(points, self.bbox, self.unbounded)
        density = self.density_network(self.encoding(pts.reshape(-1, self.cfg.n_input_dims))).reshape(*pts.shape[:-1], 1)
        return self.get_activated_density(points, density)[1]

    def forward_field(self, points):
        if self.cfg.isosurface_deformable_grid:
            warn(f"{self.__class__.__name__} does not support isosurface_deformable_grid. Ignoring.")
        return self.forward_density(points), None

    def forward_level(self, field, threshold):
        return -(field - threshold)

    def export(self, points, **kwargs) -> Dict[str, Any]:
        out: Dict[str, Any] = {}
        if self.cfg.n_feature_dims == 0:
            return out
        out["features"] = self.forward(points)["features"]
        return out
