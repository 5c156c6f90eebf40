"""`generative-space-volsdf-volume-renderer`
(custom/amortized/models/renderers/generative_space_volsdf_volume_renderer.py:36-462, built on NeuSVolumeRenderer,
threestudio/models/renderers/neus_volume_renderer.py:19-96) on the HIP path: importance-sampled VolSDF rendering of a
generator-conditioned SDF field.  Per step and ray: 128 proposal intervals (no-grad SDF pass) -> transmittance cdf -> 64
resampled edges -> 193 merged intervals -> field with finite-difference normals -> alpha compositing.

Built as a pipeline of four stages on dense [n_rays, S] interval tensors (every ray holds exactly S samples, so the packed layout
is offset = ray * S, count = S — no bincount, no masks, no dummy samples):
    _cache_per_view   generator output per rendered view          (reference :89-130: cache creation / repeat per view)
    _intervals        importance-sampled (t_start, t_end)         (:205-278 prop_sigma_fn + estimator.sampling)
    _shade            field / material / background at the samples (:280-355)
    _composite        ONE fused alpha-compositing pass             (:357-430: render_weight_from_alpha + 4 accumulate_along_rays +
                      (asd_composite_*, mode 2) and a no-grad      comp_normal): weights, opacity, depth, foreground, z-variance
                      second pass for the normal image            and the background blend come out of a single kernel

Two routes through stages 2 and 4 (ASD_VOLSDF, read at every call; "0" = the composed route above, kept as fallback and A/B partner):
the pass-level entries asd_volsdf_* (include/asd_hip.h) enqueue seven launches forward — edges, samples, proposal_cdf, edges, merge_sorted,
samples, composite_fwd — and one backward (two with a trainable variance) around the two field calls, with the material's activation, the
VolSDF density, the normal image and the learned variance (read on the device) inside the kernels.  Eligible: CUDA fp32 rays, use_volsdf,
a material that is colour = sigmoid | identity (features).  Same output dictionary on both routes.
"""
from __future__ import annotations

import os
from dataclasses import dataclass
from typing import Any, Dict, Optional, Tuple

import torch
import torch.nn.functional as F

from . import nerfacc_api, ops
from .estimators import ImportanceEstimator
from .registry import register
from .renderer import VolumeRenderer, background_colour, image_outputs
from .sdf_opacity import LearnedVariance, get_alpha, kernel_color_act, volsdf_density


class _VolSDFCompositeFn(torch.autograd.Function):
    """The compositing pass of the VolSDF renderer as one node: asd_volsdf_composite_fwd / _bwd (density -> alpha -> weights -> every per-ray
    image, the normal image included).  Gradients for sdf, features, bg and the raw variance parameter; normals and edges take none."""

    @staticmethod
    def forward(ctx, sdf, features, bg, inv_std_param, normal, t_edges, color_act):
        sdf, features, bg, t_edges = sdf.contiguous(), features.contiguous(), bg.contiguous(), t_edges.contiguous()
        normal = None if normal is None else normal.detach().contiguous()
        out = ops.volsdf_composite_fwd(sdf, features, normal, t_edges, inv_std_param, bg, color_act)
        saved = [sdf, features, bg, inv_std_param, t_edges, out["weights"], out["opacity"], out["depth"]] + ([] if normal is None else [normal])
        ctx.save_for_backward(*saved)
        ctx.color_act = color_act
        ctx.set_materialize_grads(False)
        return out["weights"], out["opacity"], out["depth"], out["rgb_fg"], out["z_var"], out["comp_rgb"], out["comp_normal"]

    @staticmethod
    def backward(ctx, d_w, d_op, d_dp, d_fg, d_zv, d_comp, d_cn):
        sdf, features, bg, inv_std_param, t_edges, w, op, dp, *rest = ctx.saved_tensors
        normal = rest[0] if rest else None
        d_sdf, d_feat, d_bg, d_p = ops.volsdf_composite_bwd(
            sdf, features, normal, t_edges, inv_std_param, bg, ctx.color_act, dict(weights=w, opacity=op, depth=dp), d_comp_rgb=d_comp, d_rgb_fg=d_fg,
            d_opacity=d_op, d_depth=d_dp, d_z_var=d_zv, d_weights=d_w, d_comp_normal=d_cn if normal is not None else None,
            want_bg=ctx.needs_input_grad[2], want_inv_std=ctx.needs_input_grad[3])
        return d_sdf.view(sdf.shape), d_feat, d_bg, d_p, None, None, None


def _cache_batch(space_cache) -> int:
    """leading (prompt / view) dimension of a generator output: a tensor, or a dict of tensors / lists of tensors"""
    if torch.is_tensor(space_cache):
        return space_cache.shape[0]
    if isinstance(space_cache, dict):
        v = next(iter(space_cache.values()))
        return v.shape[0] if torch.is_tensor(v) else v[0].shape[0]
    raise ValueError("space_cache must be a tensor or a dict")


def _field_in_chunks(field, points: torch.Tensor, chunk: int, **kw) -> Dict[str, torch.Tensor]:
    """field(points[B, Np, 3]) evaluated in slices of the POINT axis (custom/amortized/models/renderers/utils.py: the batch axis
    belongs to the space cache); outputs are re-assembled in the field's own [B * Np, C] row order"""
    B, Np = points.shape[:2]
    if chunk <= 0 or Np <= chunk:
        return field(points, **kw)
    parts = [field(points[:, i:i + chunk], **kw) for i in range(0, Np, chunk)]
    return {k: torch.cat([p[k].view(B, -1, p[k].shape[-1]) for p in parts], dim=1).reshape(B * Np, -1) for k in parts[0]}


@register("generative-space-volsdf-volume-renderer")
class GenerativeSpaceVolSDFVolumeRenderer(VolumeRenderer):
    @dataclass
    class Config(VolumeRenderer.Config):
        num_samples_per_ray: int = 512
        randomized: bool = True
        eval_chunk_size: int = 320000
        learned_variance_init: float = 0.3
        cos_anneal_end_steps: int = 0
        use_volsdf: bool = False
        near_plane: float = 0.0
        far_plane: float = 1e10
        trainable_variance: bool = True
        estimator: str = "occgrid"
        grid_prune: bool = True
        prune_alpha_threshold: bool = True
        num_samples_per_ray_importance: int = 64
        train_chunk_size: int = 0

    cfg: Config

    def configure(self, geometry, material, background) -> None:
        super().configure(geometry, material, background)
        self.variance = LearnedVariance(self.cfg.learned_variance_init, requires_grad=self.cfg.trainable_variance)
        if self.cfg.estimator != "importance":     # the reference builds nothing else for this renderer (:76-78)
            raise NotImplementedError(f"Estimator {self.cfg.estimator} not implemented for generative-space-volsdf-volume-renderer")
        self.estimator = ImportanceEstimator()
        self.cos_anneal_ratio = 1.0
        self.randomized = self.cfg.randomized

    # ---- alpha models ---------------------------------------------------------------------------------------------------------------
    def get_alpha(self, sdf, normal, dirs, dists):
        return get_alpha(sdf, normal, dirs, dists, self.variance(sdf), self.cos_anneal_ratio, self.cfg.use_volsdf)

    def _chunk(self) -> int:
        """point-axis chunk of the field calls: none while training unless train_chunk_size asks for it"""
        return self.cfg.train_chunk_size if self.training else self.cfg.eval_chunk_size

    # ---- stage 1 ----------------------------------------------------------------------------------------------------------------------
    def _cache_per_view(self, space_cache, noise, text_embed, n_views: int):
        if space_cache is None:      # (generators that ignore the noise — the hypernetwork — are called with noise = None)
            space_cache = self.geometry.generate_space_cache(styles=noise, text_embed=text_embed)
        n_cache = _cache_batch(space_cache)
        if n_cache != n_views and self.training:       # several views of one prompt share its cache (4-view groups)
            if n_views < n_cache or n_views % n_cache or not torch.is_tensor(space_cache):
                raise NotImplementedError("per-view repetition is defined for tensor caches with n_views a multiple of the prompts")
            space_cache = space_cache.repeat_interleave(n_views // n_cache, dim=0)
        return space_cache

    # ---- stage 2 ----------------------------------------------------------------------------------------------------------------------
    def _proposal_sdf(self, mid, space_cache) -> torch.Tensor:
        """the no-grad SDF [n, 1] at the proposal mid-points (any shape [..., 3], ray-major)"""
        B = _cache_batch(space_cache)
        with torch.no_grad():
            fused_sdf = getattr(self.geometry, "_use_fused", None)
            if fused_sdf is not None and fused_sdf(mid):
                # the reference evaluates the whole field here and keeps `sdf` (generative_space_volsdf_volume_renderer.py:233-252); the fused
                # fields have an sdf-only entry (same value: the sdf head does not depend on the feature head)
                return self.geometry.forward_sdf(mid.reshape(B, -1, 3), space_cache).reshape(-1, 1)
            return _field_in_chunks(self.geometry, mid.reshape(B, -1, 3), self._chunk(), space_cache=space_cache, output_normal=False)["sdf"]

    def _intervals(self, ro, rd, space_cache) -> Tuple[torch.Tensor, torch.Tensor]:
        if not self.cfg.use_volsdf:
            raise ValueError("Currently only VolSDF supports importance sampling.")

        def proposal_density(t0, t1):      # [n_rays, S] interval edges -> sigma at the mid-points, no gradient
            mid = ro[:, None, :] + rd[:, None, :] * ((t0 + t1) * 0.5)[..., None]
            with torch.no_grad():
                sdf = self._proposal_sdf(mid, space_cache)
                return volsdf_density(sdf, self.variance(sdf)).reshape(t0.shape)

        return self.estimator.sampling(prop_sigma_fns=[proposal_density], prop_samples=[self.cfg.num_samples_per_ray_importance],
                                       num_samples=self.cfg.num_samples_per_ray, n_rays=ro.shape[0], near_plane=self.cfg.near_plane,
                                       far_plane=self.cfg.far_plane, sampling_type="uniform", stratified=self.randomized)

    # ---- stage 3 ----------------------------------------------------------------------------------------------------------------------
    def _shade(self, positions, t_dirs, t_light, rays_d, space_cache, text_embed, n_views: int, extra: Dict[str, Any]):
        geo = _field_in_chunks(self.geometry, positions.reshape(n_views, -1, 3), self._chunk(), space_cache=space_cache, output_normal=True)
        if self.training:
            rgb = self.material(viewdirs=t_dirs, positions=positions, light_positions=t_light, **geo, **extra)
        else:
            n, c = positions.shape[0], max(1, self.cfg.eval_chunk_size)
            rgb = torch.cat([self.material(viewdirs=t_dirs[i:i + c], positions=positions[i:i + c], light_positions=t_light[i:i + c],
                                           **{k: v[i:i + c] for k, v in geo.items()}) for i in range(0, n, c)], dim=0)
        return geo, rgb, self._background(rays_d, text_embed)

    def _background(self, rays_d, text_embed):
        hyper_bg = getattr(self.background, "enabling_hypernet", False)
        return self.background(dirs=rays_d, text_embed=text_embed) if hyper_bg else self.background(dirs=rays_d)

    # ---- stage 4 ----------------------------------------------------------------------------------------------------------------------
    @staticmethod
    def _composite(alpha, rgb, bg_flat, t0, t1, normal, n_rays: int, per_ray: int):
        dev = alpha.device
        offset = torch.arange(n_rays, device=dev, dtype=torch.int32) * per_ray
        count = torch.full((n_rays,), per_ray, device=dev, dtype=torch.int32)
        weights, opacity, depth, fg, z_var, comp = nerfacc_api.composite(alpha, rgb, bg_flat, t0, t1, offset, count, 2)
        comp_normal = None
        if normal is not None:       # the normal image takes no gradient through the normals (reference detaches them): a second,
            with torch.no_grad():    # forward-only pass of the same kernel accumulates sum_i w_i n_i
                acc_n = nerfacc_api.composite(alpha.detach(), normal.detach().contiguous(), torch.zeros_like(bg_flat), t0, t1, offset, count, 2)[3]
                unit = (F.normalize(acc_n, dim=-1) + 1.0) * 0.5
            comp_normal = unit * opacity[:, None]                  # lerp(0, (n + 1) / 2, opacity): differentiable in the opacity only
        return weights, opacity, depth, fg, z_var, comp, comp_normal

    def _outputs(self, vhw, composited, bg, samples, geo) -> Dict[str, torch.Tensor]:
        """the renderer's output dictionary (generative_space_volsdf_volume_renderer.py:395-446): the images, and while training the per-sample tensors"""
        weights, opacity, depth, fg, z_var, comp, comp_normal = composited
        out = image_outputs(vhw, comp, fg, bg, opacity, depth, z_var)
        if comp_normal is not None:
            out["comp_normal"] = comp_normal.reshape(*vhw, 3)
        if self.training:
            t_mid, t_len, t_dirs, ray_indices, positions = samples
            out.update(weights=weights[:, None], t_points=t_mid, t_intervals=t_len, t_dirs=t_dirs, ray_indices=ray_indices, points=positions, **geo)
            out["inv_std"] = self.variance.inv_std
        return out

    # ---- the pass-level route ---------------------------------------------------------------------------------------------------------
    def _color_act(self) -> Optional[int]:
        return kernel_color_act(self.material)

    def _pass_level(self, rays_o) -> bool:
        return (os.environ.get("ASD_VOLSDF", "1") != "0" and rays_o.is_cuda and rays_o.dtype == torch.float32 and self.cfg.use_volsdf
                and self._color_act() is not None)

    def _render_pass_level(self, rays_o, rays_d, bg_color, space_cache, text_embed) -> Dict[str, torch.Tensor]:
        V, H, W = rays_o.shape[:3]
        ro, rd = rays_o.reshape(-1, 3).contiguous(), rays_d.reshape(-1, 3).contiguous().float()
        n_rays = ro.shape[0]
        p = self.variance._inv_std
        t_edges = self.estimator.sampling_volsdf(lambda mid: self._proposal_sdf(mid, space_cache), p.detach(), ro, rd,
                                                 self.cfg.num_samples_per_ray_importance, self.cfg.num_samples_per_ray, self.cfg.near_plane,
                                                 self.cfg.far_plane, stratified=self.randomized)
        positions, t_dirs, t_mid, t_len, ray_indices = ops.volsdf_samples(ro, rd, t_edges)
        geo = _field_in_chunks(self.geometry, positions.reshape(V, -1, 3), self._chunk(), space_cache=space_cache, output_normal=True)
        bg = self._background(rays_d, text_embed)
        weights, opacity, depth, fg, z_var, comp, comp_normal = _VolSDFCompositeFn.apply(
            geo["sdf"], geo["features"], background_colour(bg_color, bg, V, H, W).reshape(n_rays, -1).float(), p, geo.get("normal"), t_edges, self._color_act())
        return self._outputs((V, H, W), (weights, opacity, depth, fg, z_var, comp, comp_normal), bg, (t_mid, t_len, t_dirs, ray_indices, positions), geo)

    # ---- one set of views with one cache entry per view -------------------------------------------------------------------------------
    def _render(self, rays_o, rays_d, light_positions, bg_color, space_cache, text_embed, extra) -> Dict[str, torch.Tensor]:
        V, H, W = rays_o.shape[:3]
        if torch.is_tensor(space_cache) and space_cache.shape[0] != V:
            raise AssertionError("space_cache must have the same batch size as rays_o")
        if self._pass_level(rays_o):
            return self._render_pass_level(rays_o, rays_d, bg_color, space_cache, text_embed)
        ro, rd = rays_o.reshape(-1, 3).contiguous().float(), rays_d.reshape(-1, 3).contiguous().float()
        n_rays = ro.shape[0]
        t0, t1 = self._intervals(ro, rd, space_cache)                     # [n_rays, S]
        S = t0.shape[1]
        ray_indices = torch.arange(n_rays, device=ro.device).repeat_interleave(S)
        t0f, t1f = t0.reshape(-1).contiguous(), t1.reshape(-1).contiguous()
        t_mid, t_len = ((t0f + t1f) * 0.5)[:, None], (t1f - t0f)[:, None]
        t_dirs = rd[ray_indices]
        positions = ro[ray_indices] + t_dirs * t_mid
        t_light = light_positions.reshape(-1, 1, 3).expand(-1, H * W * S, -1).reshape(-1, 3)
        geo, rgb, bg = self._shade(positions, t_dirs, t_light, rays_d, space_cache, text_embed, V, extra)
        alpha = self.get_alpha(geo["sdf"], geo["normal"], t_dirs, t_len)[:, 0]
        weights, opacity, depth, fg, z_var, comp, comp_normal = self._composite(
            alpha, rgb, background_colour(bg_color, bg, V, H, W).reshape(n_rays, -1).float(), t0f, t1f, geo.get("normal"), n_rays, S)
        return self._outputs((V, H, W), (weights, opacity, depth, fg, z_var, comp, comp_normal), bg, (t_mid, t_len, t_dirs, ray_indices, positions), geo)

    def forward(self, rays_o, rays_d, light_positions, bg_color=None, noise=None, space_cache=None, text_embed=None, **kwargs):
        V = rays_o.shape[0]
        cache = self._cache_per_view(space_cache, noise, text_embed, V)
        if self.training or _cache_batch(cache) == V:
            return self._render(rays_o, rays_d, light_positions, bg_color, cache, text_embed, kwargs)
        # evaluation of many views of ONE prompt (orbit videos): view by view against the same cache entry
        if _cache_batch(cache) != 1:
            raise AssertionError("batch_size of space_cache must be 1 or equal to batch_size of rays_o")
        views = [self._render(rays_o[v:v + 1], rays_d[v:v + 1], light_positions[v:v + 1], None if bg_color is None else bg_color[v:v + 1],
                              cache, text_embed, kwargs) for v in range(V)]
        return {k: torch.cat([o[k] for o in views], dim=0) for k in views[0]}

    def update_step(self, epoch: int, global_step: int, on_load_weights: bool = False) -> None:
        pass

    def train(self, mode=True):
        self.randomized = mode and self.cfg.randomized
        if hasattr(self.geometry, "train"):
            self.geometry.train(mode)
        return super().train(mode=mode)

    def eval(self):
        self.randomized = False
        if hasattr(self.geometry, "eval"):
            self.geometry.eval()
        return super().train(False)
