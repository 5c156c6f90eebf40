"""`neus-volume-renderer` (threestudio/models/renderers/neus_volume_renderer.py:40-391) on the HIP path: the single-prompt SDF route,
with `implicit-sdf` as its geometry.

Same Config, forward signature and output dictionary as the reference class.  Occupancy-grid sampling runs through the marcher of
csrc/render.hip; what is specific to NeuS — the opacity model of the learned variance — runs in csrc/neus.hip:
    sampling     march -> [forward_sdf at the candidates -> asd_neus_prune_count -> scan -> compact]     (the bracket: pruning with alpha_fn)
    forward      field with normals -> material -> background -> ONE asd_neus_composite_fwd inside one autograd node
    update_step  cos_anneal_ratio, and the occupancy update with asd_neus_step_alpha as occ_eval_fn
Two routes (ASD_NEUS, read at every call; "0" = composed, kept as fallback and A/B partner): the composed route forms alpha with tensor ops
(get_alpha / step_alpha of sdf_opacity.py), prunes with asd_prune_count fed -log(1 - alpha) / dt and composites with asd_composite_* mode 1.
This renderer reads the kept count once per pass; the sync-free, capacity-sized form of the NeRF renderer is not carried over.  The sampler
is shared (renderer.OccGridVolumeRenderer), so adopting it takes `count_on_device` in `_sample` and a forward that hands `n_dev` to the field and
defers the per-sample entries (renderer.defer_per_sample); asd_neus_composite_* is per ray already.
"""
from __future__ import annotations

import os
from dataclasses import dataclass
from typing import Dict, Optional

import torch
import torch.nn.functional as F

from . import nerfacc_api, ops
from .registry import register
from .renderer import OccGridVolumeRenderer, VolumeRenderer, background_colour, chunk_batch, image_outputs, per_sample_entries
from .sdf_opacity import LearnedVariance, get_alpha, kernel_color_act, step_alpha


class _NeuSCompositeFn(torch.autograd.Function):
    """The compositing pass of the NeuS renderer as one node: asd_neus_composite_fwd / _bwd (get_alpha -> weights -> every per-ray image).
    Gradients for sdf, normal, features, bg and the raw variance parameter; directions and interval ends take none."""

    @staticmethod
    def forward(ctx, sdf, normal, features, bg, inv_std_param, dirs, t0, t1, offset, count, color_act, cos_anneal_ratio, use_volsdf, want_cn):
        c = lambda t: t.detach().contiguous().float()
        ctx.sdf_shape = sdf.shape
        sdf, normal, features, bg, dirs, t0, t1 = c(sdf).reshape(-1), c(normal), c(features), c(bg), c(dirs), c(t0), c(t1)
        out = ops.neus_composite_fwd(sdf, normal, dirs, t0, t1, features, color_act, inv_std_param, cos_anneal_ratio, use_volsdf, bg, offset, count,
                                     want_comp_normal=want_cn)
        ctx.save_for_backward(sdf, normal, features, bg, inv_std_param, dirs, t0, t1, offset, count, out["weights"], out["opacity"])
        ctx.args = (color_act, cos_anneal_ratio, use_volsdf)
        ctx.set_materialize_grads(False)
        cn = out["comp_normal"] if want_cn else sdf.new_zeros(0)
        ctx.mark_non_differentiable(cn)
        return out["weights"], out["opacity"], out["depth"], out["rgb_fg"], out["comp_rgb"], cn

    @staticmethod
    def backward(ctx, d_w, d_op, d_dp, d_fg, d_comp, _d_cn):
        sdf, normal, features, bg, p, dirs, t0, t1, offset, count, w, op = ctx.saved_tensors
        color_act, k, use_volsdf = ctx.args
        d_sdf, d_normal, d_feat, d_bg, d_p = ops.neus_composite_bwd(
            sdf, normal, dirs, t0, t1, features, color_act, p, k, use_volsdf, bg, offset, count, dict(weights=w, opacity=op), d_comp_rgb=d_comp,
            d_rgb_fg=d_fg, d_opacity=d_op, d_depth=d_dp, d_weights=d_w, want_normal=ctx.needs_input_grad[1], want_bg=ctx.needs_input_grad[3],
            want_inv_std=ctx.needs_input_grad[4])
        return (d_sdf.view(ctx.sdf_shape), d_normal, d_feat, d_bg, d_p) + (None,) * 9


@register("neus-volume-renderer")
class NeuSVolumeRenderer(OccGridVolumeRenderer):
    @dataclass
    class Config(VolumeRenderer.Config):
        num_samples_per_ray: int = 512
        randomized: bool = True
        eval_chunk_size: int = 160000
        learned_variance_init: float = 0.3
        cos_anneal_end_steps: int = 0
        use_volsdf: bool = False
        near_plane: float = 0.0
        far_plane: float = 1e10
        estimator: str = "occgrid"  # in ['occgrid', 'importance']
        grid_prune: bool = True
        prune_alpha_threshold: bool = True
        num_samples_per_ray_importance: int = 64

    cfg: Config

    def configure(self, geometry, material, background) -> None:
        self.variance = LearnedVariance(self.cfg.learned_variance_init)
        self.cos_anneal_ratio = 1.0
        super().configure(geometry, material, background)

    @staticmethod
    def _refused_estimator(name: str) -> str:
        if name == "importance":
            return ("estimator 'importance': importance-sampled VolSDF rendering is the amortized renderer "
                    "(generative-space-volsdf-volume-renderer); the single-prompt NeuS renderer here uses 'occgrid'")
        return "unknown estimator, should be in ['occgrid', 'importance']"

    # ---- routes -----------------------------------------------------------------------------------------------------------------------
    @staticmethod
    def _fused_route(t: torch.Tensor) -> bool:
        return os.environ.get("ASD_NEUS", "1") != "0" and t.is_cuda

    def _color_act(self) -> Optional[int]:
        return kernel_color_act(self.material)

    def get_alpha(self, sdf, normal, dirs, dists):
        return get_alpha(sdf, normal, dirs, dists, self.variance(sdf), self.cos_anneal_ratio, self.cfg.use_volsdf)

    # ---- sampling ---------------------------------------------------------------------------------------------------------------------
    def _sample(self, rays_o_flatten, rays_d_flatten):
        """(ray_indices int64, t_starts, t_ends, points, dirs, offset int32, count int32) of the kept samples: the three branches of the
        reference (:168-194) — no grid pruning, pruning by the grid alone, pruning by the grid and alpha_fn.  One host read per pass (the kept
        count), not two, where the sdf kernel takes the candidate count on the device — on either route (the composed one forms its alphas
        over the whole buffer; the pruning pass only ever looks at [offset, offset + count) of each ray)."""
        _, capacity = self._candidates(rays_o_flatten)
        prune_fn = None
        if self.cfg.grid_prune and self.cfg.prune_alpha_threshold:
            def prune_fn(pts, t0, t1, ray_idx, offset, count, n_dev):
                early_stop_eps, alpha_thre = 1e-4, self.estimator.alpha_threshold(0.01)
                sdf = self._candidate_values(self.geometry.forward_sdf, pts, n_dev if capacity is not None else None)
                if self._fused_route(rays_o_flatten):
                    return ops.neus_prune(sdf, offset, count, self.variance._inv_std.detach(), self.render_step_size, self.cfg.use_volsdf,
                                          early_stop_eps, alpha_thre)
                alpha = step_alpha(sdf, self.variance(sdf), self.render_step_size, self.cfg.use_volsdf)
                # (a VolSDF alpha above 1 has no density: it ends the ray here, while the running product of the fused kernel — nerfacc's —
                # changes sign behind it; step * inv_std <= 1 keeps the two routes on the same samples)
                sigma = -torch.log1p(-alpha.clamp(max=1.0)) / (t1 - t0)
                return ops.prune(sigma.contiguous(), t0, t1, offset, count, early_stop_eps, alpha_thre)
        return self._sample_packed(rays_o_flatten, rays_d_flatten, capacity, prune_fn)[:7]

    # ---- forward ----------------------------------------------------------------------------------------------------------------------
    def forward(self, rays_o: torch.Tensor, rays_d: torch.Tensor, light_positions: torch.Tensor, bg_color: Optional[torch.Tensor] = None,
                **kwargs) -> Dict[str, torch.Tensor]:
        bhw = batch_size, height, width = rays_o.shape[:3]
        rays_o_flatten = rays_o.reshape(-1, 3).contiguous().float()
        rays_d_flatten = rays_d.reshape(-1, 3).contiguous().float()
        light_positions_flatten = light_positions.reshape(-1, 1, 1, 3).expand(-1, height, width, -1).reshape(-1, 3)
        n_rays = rays_o_flatten.shape[0]
        with torch.no_grad():
            ray_indices, t_starts_, t_ends_, positions, t_dirs, offset, count = self._sample(rays_o_flatten, rays_d_flatten)
        if ray_indices.nelement() == 0:
            ray_indices, t_starts_, t_ends_, positions, t_dirs, offset, count = self._dummy_sample(
                ray_indices, t_starts_, t_ends_, rays_o_flatten, rays_d_flatten)
        self._last_n = int(ray_indices.shape[0])
        t_light_positions = light_positions_flatten[ray_indices]

        fused = self._fused_route(rays_o_flatten)
        color_act = self._color_act() if fused else None
        rgb_fg_all = None
        if self.training:
            geo_out = self.geometry(positions, output_normal=True)
            if color_act is None:
                rgb_fg_all = self.material(viewdirs=t_dirs, positions=positions, light_positions=t_light_positions, **geo_out, **kwargs)
            comp_rgb_bg = self.background(dirs=rays_d)
        else:
            geo_out = chunk_batch(self.geometry, self.cfg.eval_chunk_size, positions, output_normal=True)
            if color_act is None:
                rgb_fg_all = chunk_batch(self.material, self.cfg.eval_chunk_size, viewdirs=t_dirs, positions=positions,
                                         light_positions=t_light_positions, **geo_out)
            comp_rgb_bg = chunk_batch(self.background, self.cfg.eval_chunk_size, dirs=rays_d)
        bg_color = background_colour(bg_color, comp_rgb_bg, *bhw, per_view=False)

        want_cn = not self.training and "normal" in geo_out
        if fused:
            colours, act = (geo_out["features"], color_act) if color_act is not None else (rgb_fg_all, 0)
            weights_, opacity_, depth_, comp_rgb_fg, comp_rgb, comp_normal = _NeuSCompositeFn.apply(
                geo_out["sdf"], geo_out["normal"], colours, bg_color.float(), self.variance._inv_std, t_dirs, t_starts_, t_ends_, offset, count,
                act, float(self.cos_anneal_ratio), bool(self.cfg.use_volsdf), want_cn)
        else:
            alpha = self.get_alpha(geo_out["sdf"], geo_out["normal"], t_dirs, (t_ends_ - t_starts_)[..., None])
            weights_, opacity_, depth_, comp_rgb_fg, _, comp_rgb = nerfacc_api.composite(
                alpha[..., 0], rgb_fg_all, bg_color.float(), t_starts_, t_ends_, offset, count, 1)
            comp_normal = None
            if want_cn:
                cn = nerfacc_api.accumulate_along_rays(weights_, values=geo_out["normal"], ray_indices=ray_indices, n_rays=n_rays)
                comp_normal = (F.normalize(cn, dim=-1) + 1.0) / 2.0 * opacity_[..., None]

        out = image_outputs(bhw, comp_rgb, comp_rgb_fg, comp_rgb_bg, opacity_, depth_)
        if self.training:
            out.update(per_sample_entries(None, t_starts_, t_ends_, weights_, t_dirs, ray_indices, positions, geo_out))
        elif want_cn:
            out["comp_normal"] = comp_normal.view(batch_size, height, width, 3)
        out["inv_std"] = self.variance.inv_std
        return out

    # ---- maintenance ------------------------------------------------------------------------------------------------------------------
    def _occ_eval_fn(self, x):
        sdf = self.geometry.forward_sdf(x)
        if self._fused_route(sdf):
            return ops.neus_step_alpha(sdf, self.variance._inv_std.detach(), self.render_step_size, self.cfg.use_volsdf)
        return step_alpha(sdf, self.variance(sdf), self.render_step_size, self.cfg.use_volsdf)

    def update_step(self, epoch: int, global_step: int, on_load_weights: bool = False) -> None:
        self.cos_anneal_ratio = 1.0 if self.cfg.cos_anneal_end_steps == 0 else min(1.0, global_step / self.cfg.cos_anneal_end_steps)
        super().update_step(epoch, global_step, on_load_weights)
