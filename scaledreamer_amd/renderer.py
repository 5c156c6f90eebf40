"""`nerf-volume-renderer` (threestudio/models/renderers/nerf_volume_renderer.py:20-470) on the HIP path.

Same Config, forward signature and output dictionary as the reference class.  With the occupancy-grid
estimator (the shipped single-prompt configs) the sampling / pruning / compaction / compositing all run in
the HIP kernels of csrc/render.hip; geometry and background are called through their module interface, so
any registered geometry works, and the HIP `implicit-volume` / `neural-environment-map-background` plug in
with their fused kernels.
"""
from __future__ import annotations

import os

from dataclasses import dataclass
from typing import Any, Dict, Optional

import torch
import torch.nn.functional as F

import ctypes as C

from . import _lib, nerfacc_api, ops
from .base import BaseModule
from .registry import register, warn


class Renderer(BaseModule):
    """threestudio/models/renderers/base.py:15-72"""

    @dataclass
    class Config(BaseModule.Config):
        radius: float = 1.0

    cfg: Config

    def configure(self, geometry, material, background) -> None:
        @dataclass
        class SubModules:
            geometry: Any
            material: Any
            background: Any

        self.sub_modules = SubModules(geometry, material, background)
        r = self.cfg.radius
        self.register_buffer("bbox", torch.as_tensor([[-r, -r, -r], [r, r, r]], dtype=torch.float32))

    @property
    def geometry(self):
        return self.sub_modules.geometry

    @property
    def material(self):
        return self.sub_modules.material

    @property
    def background(self):
        return self.sub_modules.background

    def set_geometry(self, geometry) -> None:
        self.sub_modules.geometry = geometry

    def set_material(self, material) -> None:
        self.sub_modules.material = material

    def set_background(self, background) -> None:
        self.sub_modules.background = background


class VolumeRenderer(Renderer):
    pass


def chunk_batch(func, chunk_size: int, *args, **kwargs):
    """threestudio/utils/ops.py:116-180 for tensor / dict-of-tensor outputs."""
    if chunk_size <= 0:
        return func(*args, **kwargs)
    B = next(a.shape[0] for a in list(args) + list(kwargs.values()) if isinstance(a, torch.Tensor))
    outs = []
    for i in range(0, max(1, B), chunk_size):
        sl = lambda a: a[i:i + chunk_size] if isinstance(a, torch.Tensor) else a
        outs.append(func(*[sl(a) for a in args], **{k: sl(v) for k, v in kwargs.items()}))
    if isinstance(outs[0], dict):
        return {k: torch.cat([o[k] for o in outs], 0) for k in outs[0]}
    return torch.cat(outs, 0)


class LazyOutputs(dict):
    """Output dictionary whose expensive entries nobody may ever read are produced on first access.

    The reference returns `normal` / `shading_normal` (three extra hash encodes per kept sample: the finite-difference normal,
    implicit_volume.py:137-177) whenever `material.requires_normal` is set (nerf_volume_renderer.py:281-283), although the shipped
    asd_sd_nerf config neither shades with them (NoMaterial) nor weights a loss on them (lambda_orient = 0, asd_sd_nerf.yaml:106).
    Same surface here — the keys exist, `in`, indexing, `.get`, `.items()`, `**out` all work and hand out real, differentiable
    tensors — but an entry registered with `defer` costs nothing until somebody asks for it."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self._deferred = {}

    def defer(self, keys, produce):
        """`produce()` -> dict holding every key of `keys`; called at most once, on the first access to any of them"""
        cell = {"fn": produce, "keys": tuple(keys)}
        for k in keys:
            self._deferred[k] = cell

    def _force(self, key):
        cell = self._deferred.get(key)
        if cell is not None:
            vals = cell["fn"]()
            for k in cell["keys"]:
                if self._deferred.get(k) is cell:          # (a key written or deleted by the user meanwhile stays as the user left it)
                    del self._deferred[k]
                    dict.__setitem__(self, k, vals[k])

    def __getitem__(self, key):
        self._force(key)
        return dict.__getitem__(self, key)

    def get(self, key, default=None):
        return self[key] if key in self else default

    def __contains__(self, key):
        return dict.__contains__(self, key) or key in self._deferred

    # writes replace a deferred entry instead of being overwritten by it on the next read
    def __setitem__(self, key, value):
        self._deferred.pop(key, None)
        dict.__setitem__(self, key, value)

    def __delitem__(self, key):
        if self._deferred.pop(key, None) is None or dict.__contains__(self, key):
            dict.__delitem__(self, key)

    def update(self, *a, **kw):
        for k, v in dict(*a, **kw).items():
            self[k] = v

    def setdefault(self, key, default=None):
        if key not in self:
            self[key] = default
        return self[key]

    _MISSING = object()

    def pop(self, key, default=_MISSING):
        if key in self:
            v = self[key]
            dict.__delitem__(self, key)
            return v
        if default is LazyOutputs._MISSING:
            raise KeyError(key)
        return default

    def __iter__(self):                    # (also sends `{**out}` / dict(out) down the keys() + __getitem__ path); iterates over a
        yield from list(dict.__iter__(self)) + list(self._deferred)     # snapshot: forcing an entry inside the loop moves its key

    def __len__(self):
        return dict.__len__(self) + len(self._deferred)

    def keys(self):
        return list(iter(self))

    def values(self):
        return [self[k] for k in self.keys()]

    def items(self):
        return [(k, self[k]) for k in self.keys()]

    def pending(self):
        """keys not produced yet (tests / tools)"""
        return set(self._deferred)


class _RenderPass:
    """state of one fused training pass (include/asd_hip.h: asd_render_fwd / asd_render_bwd): the parameter block, the tensors its
    pointers refer to (kept alive until the backward pass) and typed views into the workspace"""

    _DT = {"count": torch.int32, "offset": torch.int32, "total": torch.int32, "kept": torch.int32, "koff": torch.int32, "n_kept": torch.int32,
           "ray_idx": torch.int64, "keep": torch.uint8, "c_ray_idx": torch.int32}

    def __init__(self, march_cfg, meta, fcfg, rays_o, rays_d, bits, jitter, early_stop_eps, alpha_thre, prune, color_act, capacity):
        self.march_cfg, self.meta, self.fcfg = march_cfg, meta, fcfg
        self.rays_o, self.rays_d, self.bits, self.jitter = rays_o, rays_d, bits, jitter
        self.n_rays, self.capacity = rays_o.shape[0], int(capacity)
        self.early_stop_eps, self.alpha_thre, self.prune, self.color_act = float(early_stop_eps), float(alpha_thre), int(prune), int(color_act)
        self.layout = _lib.RenderLayout()
        _lib.check(_lib.lib().asd_render_layout_init(_lib.i32(self.n_rays), _lib.i32(self.capacity), C.byref(self.layout)))
        self.ws = None

    def params(self, grid, w1d, w2d, w1f, w2f, bg) -> "_lib.RenderParams":
        p = _lib.RenderParams()
        p.march = self.march_cfg
        p.meta, p.field = C.addressof(self.meta), C.addressof(self.fcfg)
        p.rays_o, p.rays_d, p.n_rays = self.rays_o.data_ptr(), self.rays_d.data_ptr(), self.n_rays
        p.occ_bits, p.jitter = self.bits.data_ptr(), (None if self.jitter is None else self.jitter.data_ptr())
        p.grid, p.w1d, p.w2d, p.w1f, p.w2f, p.bg = (t.data_ptr() for t in (grid, w1d, w2d, w1f, w2f, bg))
        p.early_stop_eps, p.alpha_thre, p.prune, p.color_act, p.capacity = self.early_stop_eps, self.alpha_thre, self.prune, self.color_act, self.capacity
        return p

    def view(self, name: str, cols: int = 0, rows: Optional[int] = None) -> torch.Tensor:
        """typed view of a workspace buffer: per-ray buffers have n_rays rows, per-sample ones `capacity` (or the first `rows`)"""
        dt = self._DT.get(name, torch.float32)
        per_ray = name in ("count", "offset", "kept", "koff", "opacity", "depth", "z_var", "rgb_fg", "comp_rgb")
        n = 1 if name in ("total", "n_kept") else (self.n_rays if per_ray else self.capacity)
        if rows is not None:
            n = rows
        width = max(cols, 1)
        off = getattr(self.layout, name)
        nbytes = n * width * torch.empty(0, dtype=dt).element_size()
        t = self.ws[off:off + nbytes].view(dt)
        return t.view(n, cols) if cols else t


class _RenderFn(torch.autograd.Function):
    """the whole training pass of the renderer as one autograd node: (hash table, four MLP weights, per-ray background) -> (comp_rgb,
    comp_rgb_fg, opacity, depth, z_variance); nothing in between is a Python-issued launch"""

    @staticmethod
    def forward(ctx, grid, w1d, w2d, w1f, w2f, bg, st):
        st.ws = torch.empty(st.layout.total_bytes, dtype=torch.uint8, device=grid.device)
        p = st.params(grid, w1d, w2d, w1f, w2f, bg)
        _lib.check(_lib.lib().asd_render_fwd(C.byref(p), _lib.ptr(st.ws), _lib.stream()))
        ctx.st = st
        ctx.save_for_backward(grid, w1d, w2d, w1f, w2f, bg)
        ctx.set_materialize_grads(False)
        # asd_render_bwd re-reads opacity / depth / weights from st.ws, which autograd does not version-check: the caller gets COPIES of the
        # five per-ray outputs (they are the contiguous tail of the layout: one n_rays * ~36 B copy), so an in-place op on a returned tensor
        # cannot corrupt the gradients and a surviving output does not pin the n_rays * max_steps * ~217 B workspace
        L, n = st.layout, st.n_rays
        tail = st.ws[L.opacity:L.c_feats].clone()

        def out(off, cols):
            t = tail[off - L.opacity:off - L.opacity + n * max(cols, 1) * 4].view(torch.float32)
            return t.view(n, cols) if cols else t
        return out(L.comp_rgb, 3), out(L.rgb_fg, 3), out(L.opacity, 0), out(L.depth, 0), out(L.z_var, 0)

    @staticmethod
    def backward(ctx, d_comp, d_fg, d_op, d_dp, d_zv):
        grid, w1d, w2d, w1f, w2f, bg = ctx.saved_tensors
        st = ctx.st
        d_grid = torch.zeros_like(grid)
        ws_ = (w1d, w2d, w1f, w2f)           # the four small gradients: views of ONE zeroed buffer (16-byte aligned pieces)
        offs, total = [], 0
        for w in ws_:
            offs.append(total)
            total += (w.numel() + 3) // 4 * 4
        flat = torch.zeros(total, device=grid.device, dtype=torch.float32)
        dws = [flat[o:o + w.numel()].view_as(w) for o, w in zip(offs, ws_)]
        if all(g is None for g in (d_comp, d_fg, d_op, d_dp, d_zv)):
            return (d_grid, *dws, None, None)
        p = st.params(grid, w1d, w2d, w1f, w2f, bg)
        nf = C.c_int64(0)
        _lib.check(_lib.lib().asd_render_bwd_workspace(C.byref(p), C.byref(nf)))
        bws = torch.empty(nf.value, device=grid.device, dtype=torch.float32)
        d_bg = torch.empty_like(bg) if ctx.needs_input_grad[5] else None
        k = ops._Keep()
        _lib.check(_lib.lib().asd_render_bwd(C.byref(p), _lib.ptr(st.ws), k(d_comp), k(d_fg), k(d_op), k(d_dp), k(d_zv), _lib.ptr(d_grid),
                                             *(_lib.ptr(t) for t in dws), _lib.ptr(d_bg), _lib.ptr(bws), _lib.stream()))
        if d_bg is not None and d_comp is None:
            d_bg.zero_()
        return (d_grid, *dws, d_bg, None)


def validate_empty_rays(ray_indices, t_start, t_end):
    """threestudio/utils/ops.py:514-520: substitute one dummy sample when nothing was sampled."""
    if ray_indices.nelement() == 0:
        warn("Empty rays_indices!")
        ray_indices = torch.zeros(1, dtype=torch.long, device=ray_indices.device)
        t_start = torch.zeros(1, device=ray_indices.device)
        t_end = torch.zeros(1, device=ray_indices.device)
    return ray_indices, t_start, t_end


# ---- what every route of the three volume renderers builds the same way -------------------------------------------------------------
def background_colour(bg_color, comp_rgb_bg, batch_size: int, height: int, width: int, per_view: bool = True):
    """the colour compositing blends behind each ray: the background's own image unless the caller names a colour — one per view [B, C]
    (expanded over the image; `per_view=False` hands it on as it came, as the reference's neus_volume_renderer.py does), an image
    [B, H, W, C] or rows [n_rays, C].  Images leave as rows."""
    if bg_color is None:
        bg_color = comp_rgb_bg
    elif per_view and bg_color.shape[:-1] == (batch_size,):
        bg_color = bg_color.unsqueeze(1).unsqueeze(1).expand(-1, height, width, -1)
    if bg_color.shape[:-1] == (batch_size, height, width):
        bg_color = bg_color.reshape(batch_size * height * width, -1)
    return bg_color


def image_outputs(bhw, comp_rgb, comp_rgb_fg, comp_rgb_bg, opacity, depth, z_variance=None) -> Dict[str, torch.Tensor]:
    """the per-ray entries of an output dictionary as images [B, H, W, C], in the reference's order"""
    out = {"comp_rgb": comp_rgb.reshape(*bhw, -1), "comp_rgb_fg": comp_rgb_fg.reshape(*bhw, -1), "comp_rgb_bg": comp_rgb_bg.reshape(*bhw, -1),
           "opacity": opacity.reshape(*bhw, 1), "depth": depth.reshape(*bhw, 1)}
    if z_variance is not None:
        out["z_variance"] = z_variance.reshape(*bhw, 1)
    return out


SAMPLE_KEYS = ("weights", "t_points", "t_intervals", "t_dirs", "ray_indices", "points")


def per_sample_entries(n: Optional[int], t0, t1, weights, dirs, ray_indices, points, geo_out) -> Dict[str, torch.Tensor]:
    """the per-sample entries of a training pass's output dictionary (SAMPLE_KEYS, then the geometry's own) from the packed sample tensors:
    all of their rows, or the first n of capacity-sized ones"""
    cut = (lambda t: t) if n is None else (lambda t: t[:n])
    t0, t1 = cut(t0)[..., None], cut(t1)[..., None]
    out = {"weights": cut(weights)[..., None], "t_points": (t0 + t1) / 2.0, "t_intervals": t1 - t0, "t_dirs": cut(dirs),
           "ray_indices": cut(ray_indices), "points": cut(points)}
    out.update({k: cut(v) for k, v in geo_out.items()})
    return out


def kept_points(n_dev, points, rays_o) -> torch.Tensor:
    """`points(n)`, the n written rows of a capacity-sized buffer, with ONE read of the device count — or, of an empty batch, the position
    of the reference's dummy sample (validate_empty_rays): the origin of ray 0"""
    n = int(n_dev.item())
    return points(n) if n > 0 else rays_o[:1].detach()


def defer_per_sample(out: LazyOutputs, n_dev, geometry, rays_o, rays_d, geo_keys, rows) -> None:
    """the per-sample entries of a pass that left the kept count on the device: made with ONE read of the count when somebody first asks for
    one.  `rows(n)` -> (t0, t1, weights, dirs, ray_indices, points, geo_out) holding at least n rows.  An empty batch gives the one dummy
    sample: ray 0, t = 0, no weight, the field's entries at its position zeroed."""
    def per_sample():
        n = int(n_dev.item())
        if n > 0:
            return per_sample_entries(n, *rows(n))
        point = rays_o[:1].detach()
        z = point.new_zeros(1)
        geo_out = {k: v * 0.0 for k, v in geometry(point, output_normal=False).items()}
        return per_sample_entries(None, z, z, z, rays_d[:1], torch.zeros(1, dtype=torch.long, device=z.device), point, geo_out)

    out.defer(SAMPLE_KEYS + tuple(geo_keys), per_sample)


def defer_normals(out: LazyOutputs, geometry, points) -> None:
    """`normal` / `shading_normal` of a material that asks for normals nothing in the call reads: the geometry is evaluated with them at
    `points()` only if somebody indexes one (LazyOutputs)"""
    def lazy_normal():
        g = geometry(points(), output_normal=True)
        return {"normal": g["normal"], "shading_normal": g["shading_normal"]}

    out.defer(("normal", "shading_normal"), lazy_normal)


class OccGridVolumeRenderer(VolumeRenderer):
    """What the two occupancy-grid renderers (nerf-volume-renderer, neus-volume-renderer) share: the estimator and its step size, the
    candidate-capacity rule and the call of the one sampler (nerfacc_api.OccGridEstimator.sample_packed), the dummy sample of an all-miss
    batch, and the occupancy update.  A class says what it prunes with (`_sample`) and what the grid holds (`_occ_eval_fn`)."""

    # upper bound of the capacity-sized candidate buffers (~28 B per candidate across ray_idx / t0 / t1 / points / sigma / keep: 1.3 GB);
    # also keeps every 3-component index of those buffers far below 2^31
    MAX_CANDIDATE_CAPACITY = 48 << 20

    def configure(self, geometry, material, background) -> None:
        super().configure(geometry, material, background)
        if self.cfg.estimator != "occgrid":
            raise NotImplementedError(self._refused_estimator(self.cfg.estimator))
        self.estimator = nerfacc_api.OccGridEstimator(roi_aabb=self.bbox.view(-1), resolution=32, levels=1)
        if not self.cfg.grid_prune:
            self.estimator.occs.fill_(True)
            self.estimator.binaries.fill_(True)
        self.render_step_size = 1.732 * 2 * self.cfg.radius / self.cfg.num_samples_per_ray
        self.randomized = self.cfg.randomized
        self.jitter_fn = lambda n, device: torch.rand(n, device=device)  # injectable

    def _march_cfg(self) -> "_lib.MarchCfg":
        return self.estimator.march_cfg(self.cfg.near_plane, self.cfg.far_plane, self.render_step_size)

    def _capacity(self, n_rays: int) -> Optional[int]:
        """every ray at most max_steps lattice points; None for large batches (256^2 x 4 views: 1.3e8 lattice points)"""
        n_cap = n_rays * int(self._march_cfg().max_steps)
        return n_cap if n_cap <= self.MAX_CANDIDATE_CAPACITY else None

    def _candidates(self, rays_o):
        """(device_count, capacity).  With a pruning pass on the fused field kernels in training, the candidate buffers stand at their
        upper bound and the candidate count stays on the device: the pruning pass only ever looks at [offset, offset + count) of each ray,
        and the field kernel takes the total as a device scalar — no device->host read of it.  Above MAX_CANDIDATE_CAPACITY: exact-size
        buffers after one count read-back."""
        device_count = bool(self.training and self.cfg.grid_prune and self.cfg.prune_alpha_threshold
                            and getattr(self.geometry, "fused", False) and rays_o.is_cuda)
        return device_count, (self._capacity(rays_o.shape[0]) if device_count else None)

    def _candidate_values(self, field_fn, pts, n_dev=None) -> torch.Tensor:
        """field_fn (forward_density / forward_sdf) at the candidate mid-points the marcher produced, [n]: over the first n_dev rows where
        the count stays on the device, in chunks of eval_chunk_size outside training"""
        if pts.shape[0] == 0:
            return pts.new_zeros(0)
        if n_dev is not None:
            vals = field_fn(pts, n_dev=n_dev)
        elif self.training:
            vals = field_fn(pts)
        else:
            vals = chunk_batch(field_fn, self.cfg.eval_chunk_size, pts)
        return vals[..., 0].contiguous().float()

    def _sample_packed(self, rays_o, rays_d, capacity, prune_fn, count_on_device: bool = False):
        jitter = self.jitter_fn(rays_o.shape[0], rays_o.device) if self.randomized else None
        return self.estimator.sample_packed(rays_o, rays_d, self.cfg.near_plane, self.cfg.far_plane, self.render_step_size, jitter,
                                            capacity, prune_fn, count_on_device)

    @staticmethod
    def _dummy_sample(ray_indices, t_starts, t_ends, rays_o, rays_d):
        """the reference's one dummy sample of a batch that kept nothing (validate_empty_rays): ray 0, t = 0, with its packed layout"""
        ray_indices, t_starts, t_ends = validate_empty_rays(ray_indices, t_starts, t_ends)
        positions = rays_o[ray_indices] + rays_d[ray_indices] * 0.0
        count = torch.zeros(rays_o.shape[0], dtype=torch.int32, device=rays_o.device)
        count[0] = 1
        offset = torch.ones(rays_o.shape[0], dtype=torch.int32, device=rays_o.device)
        offset[0] = 0
        return ray_indices, t_starts, t_ends, positions, rays_d[ray_indices], offset, count

    @property
    def last_n_samples(self) -> int:
        """kept samples of the last forward pass (reads the device count of a sync-free pass when asked)"""
        n = getattr(self, "_last_n", 0)
        return int(n.item()) if torch.is_tensor(n) else int(n)

    def update_step(self, epoch: int, global_step: int, on_load_weights: bool = False) -> None:
        if self.cfg.grid_prune and self.training and not on_load_weights:
            self.estimator.update_every_n_steps(step=global_step, occ_eval_fn=self._occ_eval_fn)

    def train(self, mode=True):
        self.randomized = mode and self.cfg.randomized
        return super().train(mode=mode)

    def eval(self):
        self.randomized = False
        return super().eval()


@register("nerf-volume-renderer")
class NeRFVolumeRenderer(OccGridVolumeRenderer):
    @dataclass
    class Config(VolumeRenderer.Config):
        num_samples_per_ray: int = 512
        eval_chunk_size: int = 160000
        randomized: bool = True
        near_plane: float = 0.0
        far_plane: float = 1e10
        return_comp_normal: bool = False
        return_normal_perturb: bool = False
        estimator: str = "occgrid"  # in ["occgrid", "proposal", "importance"]
        grid_prune: bool = True
        prune_alpha_threshold: bool = True
        proposal_network_config: Optional[dict] = None
        prop_optimizer_config: Optional[dict] = None
        prop_scheduler_config: Optional[dict] = None
        num_samples_per_ray_proposal: int = 64
        num_samples_per_ray_importance: int = 64

    cfg: Config

    @staticmethod
    def _refused_estimator(name: str) -> str:
        if name in ("importance", "proposal"):
            return (f"estimator {name!r}: the single-prompt ASD configs use 'occgrid' "
                    "(importance sampling belongs to the amortized renderer; proposal is unused — SURVEY.md §2.2 N9/N10)")
        return "Unknown estimator, should be one of ['occgrid', 'proposal', 'importance']."

    # ------------------------------------------------------------------------------------------
    def _sample(self, rays_o_flatten, rays_d_flatten, sync_free: bool = False):
        """(ray_indices int64, t_starts, t_ends, points, dirs, offset int32, count int32, total) of the kept samples.  `total` is None
        and the sample tensors have exactly the kept length — or, with sync_free (and the fused candidate path), `total` is the kept
        count as an int32 DEVICE scalar and the sample tensors have the candidates' capacity: only their first `total` rows are
        written (ray_indices reads 0 behind them), and no device->host read happens in here at all."""
        device_count, capacity = self._candidates(rays_o_flatten)
        prune_fn = None
        if self.cfg.grid_prune and self.cfg.prune_alpha_threshold:      # (grid_prune alone: the grid prunes, no visibility pass)
            def prune_fn(pts, t0, t1, ray_idx, offset, count, n_dev):
                # sigma at the candidate mid-points (the reference's sigma_fn, nerf_volume_renderer.py:153-167)
                sigma = self._candidate_values(self.geometry.forward_density, pts, n_dev if device_count else None)
                return ops.prune(sigma, t0, t1, offset, count, 1e-4, self.estimator.alpha_threshold(0.01))
        return self._sample_packed(rays_o_flatten, rays_d_flatten, capacity, prune_fn, sync_free)

    def forward(self, rays_o: torch.Tensor, rays_d: torch.Tensor, light_positions: torch.Tensor,
                bg_color: Optional[torch.Tensor] = None, **kwargs) -> Dict[str, torch.Tensor]:
        bhw = batch_size, height, width = rays_o.shape[:3]
        rays_o_flatten = rays_o.reshape(-1, 3).contiguous().float()
        rays_d_flatten = rays_d.reshape(-1, 3).contiguous().float()
        light_positions_flatten = light_positions.reshape(-1, 1, 1, 3).expand(-1, height, width, -1).reshape(-1, 3)
        n_rays = rays_o_flatten.shape[0]

        # Sync-free training path: the kept-sample count stays on the device (the field kernels take it as `n_dev`, compositing is per
        # ray), the per-sample tensors are capacity-sized, and the per-sample entries of the output dictionary are cut to their exact
        # length only if somebody reads them (LazyOutputs) — the host never waits for the GPU inside a step, so it runs ahead of it and
        # its launch latencies disappear from the step (the read-back cost 0.1 ms of GPU idle time plus a host-bound renderer forward).
        # Needs: fused field kernels, a material that is a row-wise function of the features, no consumer of the normal in here.
        sync_free = (self.training and os.environ.get("ASD_SYNC_FREE", "1") != "0" and getattr(self.geometry, "fused", False)
                     and rays_o_flatten.is_cuda and getattr(self.material, "elementwise", False) and not self.cfg.return_comp_normal
                     and not self.cfg.return_normal_perturb
                     and not (self.material.requires_normal and getattr(self.material, "reads_normal", True)))
        if sync_free and self._fused_pass_ok(n_rays):
            return self._forward_fused_pass(bhw, rays_o_flatten, rays_d_flatten, rays_d, bg_color, kwargs)
        with torch.no_grad():
            ray_indices, t_starts_, t_ends_, positions, t_dirs, offset, count, n_dev = self._sample(rays_o_flatten, rays_d_flatten, sync_free)
        if n_dev is not None:
            return self._forward_sync_free(bhw, rays_o_flatten, rays_d_flatten, rays_d, bg_color, ray_indices, t_starts_, t_ends_, positions,
                                           t_dirs, offset, count, n_dev, kwargs)
        if ray_indices.nelement() == 0:
            ray_indices, t_starts_, t_ends_, positions, t_dirs, offset, count = self._dummy_sample(
                ray_indices, t_starts_, t_ends_, rays_o_flatten, rays_d_flatten)
        self._last_n = int(ray_indices.shape[0])
        t_light_positions = light_positions_flatten[ray_indices]

        want_lazy_normal = False
        if self.training:
            # the normal is evaluated with the field only if something inside this call reads it (a shading material, comp_normal,
            # normal_perturb); otherwise it becomes a deferred entry of the output dictionary (LazyOutputs)
            want_normal = bool(self.material.requires_normal)
            now = want_normal and (getattr(self.material, "reads_normal", True) or self.cfg.return_comp_normal or self.cfg.return_normal_perturb)
            want_lazy_normal = want_normal and not now
            geo_out = self.geometry(positions, output_normal=now)
            rgb_fg_all = self.material(viewdirs=t_dirs, positions=positions, light_positions=t_light_positions,
                                       **geo_out, **kwargs)
            comp_rgb_bg = self.background(dirs=rays_d)
        else:
            geo_out = chunk_batch(self.geometry, self.cfg.eval_chunk_size, positions,
                                  output_normal=self.material.requires_normal)
            rgb_fg_all = chunk_batch(self.material, self.cfg.eval_chunk_size, viewdirs=t_dirs, positions=positions,
                                     light_positions=t_light_positions, **geo_out)
            comp_rgb_bg = chunk_batch(self.background, self.cfg.eval_chunk_size, dirs=rays_d)

        # T / alpha / weights + all per-ray accumulations (reference :312-364) in one fused pass
        weights_, opacity_, depth_, comp_rgb_fg, z_variance_, comp_rgb = nerfacc_api.composite(
            geo_out["density"][..., 0], rgb_fg_all, background_colour(bg_color, comp_rgb_bg, *bhw).float(), t_starts_, t_ends_, offset, count, 0
        )
        out = LazyOutputs(image_outputs(bhw, comp_rgb, comp_rgb_fg, comp_rgb_bg, opacity_, depth_, z_variance_))

        def comp_normal_of(normal):
            cn = nerfacc_api.accumulate_along_rays(weights_, values=normal, ray_indices=ray_indices, n_rays=n_rays)
            cn = F.normalize(cn, dim=-1)
            return ((cn + 1.0) / 2.0 * opacity_[..., None]).view(batch_size, height, width, 3)

        if self.training:
            out.update(per_sample_entries(None, t_starts_, t_ends_, weights_, t_dirs, ray_indices, positions, geo_out))
            if want_lazy_normal:
                defer_normals(out, self.geometry, lambda: positions)
            if "normal" in geo_out:
                if self.cfg.return_comp_normal:
                    out["comp_normal"] = comp_normal_of(geo_out["normal"])
                if self.cfg.return_normal_perturb:
                    out["normal_perturb"] = self.geometry(positions + torch.randn_like(positions) * 1e-2,
                                                          output_normal=self.material.requires_normal)["normal"]
        elif "normal" in geo_out:
            out["comp_normal"] = comp_normal_of(geo_out["normal"])
        return out

    # ---- the training pass as one C-ABI entry each way ---------------------------------------------------------------------------
    _COLOR_ACTS = {"sigmoid": 1, "none": 0, None: 0}

    def _fused_pass_ok(self, n_rays: int) -> bool:
        """asd_render_fwd covers: occupancy-grid sampling, a density field on the fused kernels with 3 feature dims, colour =
        sigmoid(features) | features, no normal consumer inside the call (the conditions of the sync-free path, narrowed)"""
        geo, mat = self.geometry, self.material
        fc = getattr(geo, "_fcfg", None)
        return (fc is not None and hasattr(geo, "_weights") and hasattr(geo, "_meta")
                and getattr(geo.cfg, "n_feature_dims", 0) == 3 and fc.field_mode == _lib.ASD_FIELD_DENSITY
                and getattr(mat.cfg, "color_activation", "?") in self._COLOR_ACTS and torch.is_grad_enabled()
                and geo.encoding.encoding.encoding.params.requires_grad and self._capacity(n_rays) is not None)

    def _forward_fused_pass(self, bhw, rays_o_flatten, rays_d_flatten, rays_d, bg_color, kwargs):
        n_rays = rays_o_flatten.shape[0]
        est, geo, material = self.estimator, self.geometry, self.material
        jitter = self.jitter_fn(n_rays, rays_o_flatten.device) if self.randomized else None
        if jitter is not None:
            jitter = jitter.contiguous().float()
        mcfg = self._march_cfg()
        bits = est._bits()                       # (also refreshes the host mirror of the mean occupancy read below)
        prune = self.cfg.grid_prune and self.cfg.prune_alpha_threshold
        early_stop_eps, alpha_thre = (1e-4, est.alpha_threshold(0.01)) if prune else (0.0, 0.0)
        st = _RenderPass(mcfg, geo._meta, geo._fcfg, rays_o_flatten, rays_d_flatten, bits, jitter, early_stop_eps, alpha_thre, prune,
                         self._COLOR_ACTS[material.cfg.color_activation], n_rays * int(mcfg.max_steps))
        comp_rgb_bg = self.background(dirs=rays_d)
        bg_flat = background_colour(bg_color, comp_rgb_bg, *bhw)
        grid = geo.encoding.encoding.encoding.params
        comp_rgb, comp_rgb_fg, opacity, depth, z_var = _RenderFn.apply(grid, *geo._weights(), bg_flat.float().contiguous(), st)
        n_dev = st.view("n_kept")
        self._last_n = n_dev
        out = LazyOutputs(image_outputs(bhw, comp_rgb, comp_rgb_fg, comp_rgb_bg, opacity, depth, z_var))

        def rows(n):
            """the composed (differentiable) evaluation of the same samples — field, material, compositing weights — so that a loss on the
            per-sample entries reaches the parameters as in the reference"""
            t0, t1, pts, dirs = st.view("t0", rows=n), st.view("t1", rows=n), st.view("pts", 3, rows=n), st.view("dirs", 3, rows=n)
            g = geo(pts, output_normal=False)
            rgb = material(viewdirs=dirs, positions=pts, light_positions=None, **g, **kwargs)
            w = nerfacc_api.composite(g["density"][..., 0], rgb, bg_flat.float().detach(), t0, t1, st.view("koff"), st.view("kept"), 0)[0]
            return t0, t1, w, dirs, st.view("ray_idx", rows=n), pts, g

        defer_per_sample(out, n_dev, geo, rays_o_flatten, rays_d_flatten, ("density", "features"), rows)
        if material.requires_normal:
            defer_normals(out, geo, lambda: kept_points(n_dev, lambda n: st.view("pts", 3, rows=n), rays_o_flatten))
        return out

    def _forward_sync_free(self, bhw, rays_o_flatten, rays_d_flatten, rays_d, bg_color, ray_indices, t_starts_, t_ends_, positions, t_dirs,
                           offset, count, n_dev, kwargs):
        """forward() behind the sampler with the kept count on the device (see there): same arithmetic on the first n_dev rows"""
        self._last_n = n_dev
        geo_out = self.geometry(positions, output_normal=False, n_dev=n_dev)
        rgb_fg_all = self.material(viewdirs=t_dirs, positions=positions, light_positions=None, **geo_out, **kwargs)
        comp_rgb_bg = self.background(dirs=rays_d)
        weights_, opacity_, depth_, comp_rgb_fg, z_variance_, comp_rgb = nerfacc_api.composite(
            geo_out["density"][..., 0], rgb_fg_all, background_colour(bg_color, comp_rgb_bg, *bhw).float(), t_starts_, t_ends_, offset, count, 0
        )
        out = LazyOutputs(image_outputs(bhw, comp_rgb, comp_rgb_fg, comp_rgb_bg, opacity_, depth_, z_variance_))
        defer_per_sample(out, n_dev, self.geometry, rays_o_flatten, rays_d_flatten, tuple(geo_out),
                         lambda n: (t_starts_, t_ends_, weights_, t_dirs, ray_indices, positions, geo_out))
        if self.material.requires_normal:
            defer_normals(out, self.geometry, lambda: kept_points(n_dev, lambda n: positions[:n], rays_o_flatten))
        return out

    def _occ_eval_fn(self, x):
        # approximates 1 - exp(-density * step) by its first-order term (reference :436-439)
        return self.geometry.forward_density(x) * self.render_step_size

