"""`stable-diffusion-asynchronous-score-distillation-guidance`
(threestudio/models/guidance/stable_diffusion_asd_guidance.py:24-440) with the diffusion prior behind a small
backend interface, plus the prompt-side helper the guidance consumes
(threestudio/models/prompt_processors/base.py:38-167 `PromptProcessorOutput`).

The reference loads diffusers' StableDiffusionPipeline (fp16) and strings ~60 torch elementwise ops around it.  Here the frozen
UNet / VAE encoder are a `DiffusionBackend` (C-ABI networks) and everything between the rendered image and the scalar loss is one
autograd node (`_ScoreDistillation`) on five fused HIP kernels (csrc/asd_glue.hip); the latents, both noisings and the UNet's
batch layout are written straight into the network's input buffers.  The seams are the reference's own: forward_unet (:319-331)
and encode_images (:171-178).
"""
from __future__ import annotations


from dataclasses import dataclass, field
from typing import Any, Callable, Dict, List, Optional, Tuple

import torch

from .base import BaseObject
from .config import C
from .registry import info, register


def shift_azimuth_deg(azimuth: torch.Tensor) -> torch.Tensor:
    return (azimuth + 180) % 360 - 180


def shifted_expotional_decay(a, b, c, r):
    return a * torch.exp(-b * r) + c


def ddpm_alphas_cumprod(n: int = 1000, beta_start: float = 0.00085, beta_end: float = 0.012) -> torch.Tensor:
    """scaled-linear schedule of SD (in-tree: extern/mvdream/ldm/interface.py:48-76)."""
    betas = torch.linspace(beta_start ** 0.5, beta_end ** 0.5, n, dtype=torch.float64) ** 2
    return torch.cumprod(1.0 - betas, dim=0).float()


@dataclass
class PromptUtils:
    """Output layout of the prompt processors: view-dependent embeddings [4,77,1024] in the order
    side / front / back / overhead (prompt_processors/base.py:100-104) + the Perp-Neg interpolation rules."""
    text_embeddings_vd: torch.Tensor
    uncond_text_embeddings_vd: torch.Tensor
    text_embeddings: Optional[torch.Tensor] = None
    uncond_text_embeddings: Optional[torch.Tensor] = None
    use_perp_neg: bool = True
    overhead_threshold: float = 60.0
    front_threshold: float = 45.0
    back_threshold: float = 45.0
    perp_neg_f_sb: Tuple[float, float, float] = (1, 0.5, -0.606)
    perp_neg_f_fsb: Tuple[float, float, float] = (1, 0.5, +0.967)
    perp_neg_f_fs: Tuple[float, float, float] = (4, 0.5, -2.426)
    perp_neg_f_sf: Tuple[float, float, float] = (4, 0.5, -2.426)

    @staticmethod
    def synthetic(seed: int = 1234, device="cpu", **kw) -> "PromptUtils":
        """ "synthetic random prompts" (BASELINE.json): N(0,1) embeddings, one uncond row."""
        g = torch.Generator().manual_seed(seed)
        vd = torch.randn(4, 77, 1024, generator=g)
        un = torch.randn(1, 77, 1024, generator=g).expand(4, -1, -1).contiguous()
        return PromptUtils(vd.to(device), un.to(device), vd[0].to(device), un[0].to(device), **kw)

    def direction_idx(self, elevation, azimuth, camera_distances):
        """later directions override earlier ones: side < front < back < overhead (base.py:262-294)."""
        idx = torch.zeros_like(elevation, dtype=torch.long)
        azi = shift_azimuth_deg(azimuth)
        idx = torch.where((azi > -self.front_threshold) & (azi < self.front_threshold), torch.ones_like(idx), idx)
        idx = torch.where((azi > 180 - self.back_threshold) | (azi < -180 + self.back_threshold), torch.full_like(idx, 2), idx)
        return torch.where(elevation > self.overhead_threshold, torch.full_like(idx, 3), idx)

    def get_text_embeddings(self, elevation, azimuth, camera_distances, view_dependent_prompting: bool = True):
        batch_size = elevation.shape[0]
        if view_dependent_prompting:
            idx = self.direction_idx(elevation, azimuth, camera_distances)
            text, uncond = self.text_embeddings_vd[idx], self.uncond_text_embeddings_vd[idx]
        else:
            text = self.text_embeddings.expand(batch_size, -1, -1)
            uncond = self.uncond_text_embeddings.expand(batch_size, -1, -1)
        return torch.cat([text, uncond], dim=0)  # (cond, uncond): the reference's order

    def get_text_embeddings_perp_neg(self, elevation, azimuth, camera_distances, view_dependent_prompting: bool = True):
        """prompt_processors/base.py:82-167.  The reference walks the batch in Python and branches on device scalars (one host
        sync per `if`); here the same selection is written with torch.where so that nothing between the VAE forward and the
        UNet launch waits for the GPU.  Output order as the reference: [pos (B), uncond (B), neg (2B: n1_0, n2_0, n1_1, ...)]."""
        assert view_dependent_prompting, "Perp-Neg only works with view-dependent prompting"
        batch_size = elevation.shape[0]
        idx = self.direction_idx(elevation, azimuth, camera_distances)
        side, front, back, overhead = (self.text_embeddings_vd[i] for i in range(4))
        a = torch.abs(shift_azimuth_deg(azimuth)).to(side.dtype)
        over = (idx == 3).view(-1, 1, 1)
        is_front = (a < 90).view(-1, 1, 1)
        r_f = (1 - a / 90).view(-1, 1, 1)             # front <-> side
        r_b = (2.0 - a / 90).view(-1, 1, 1)           # side <-> back
        uncond = self.uncond_text_embeddings_vd[idx]
        pos = torch.where(over, overhead.expand(batch_size, -1, -1),
                          torch.where(is_front, r_f * front + (1 - r_f) * side, r_b * side + (1 - r_b) * back))
        neg1 = torch.where(over, uncond, torch.where(is_front, front.expand(batch_size, -1, -1), side.expand(batch_size, -1, -1)))
        neg2 = torch.where(over, uncond, torch.where(is_front, side.expand(batch_size, -1, -1), front.expand(batch_size, -1, -1)))
        rf, rb = r_f.view(-1), r_b.view(-1)
        w1 = torch.where(a < 90, -shifted_expotional_decay(*self.perp_neg_f_fs, rf), -shifted_expotional_decay(*self.perp_neg_f_sb, rb))
        w2 = torch.where(a < 90, -shifted_expotional_decay(*self.perp_neg_f_sf, 1 - rf), -shifted_expotional_decay(*self.perp_neg_f_fsb, rb))
        zero = torch.zeros_like(w1)
        weights = torch.stack([torch.where(idx == 3, zero, w1), torch.where(idx == 3, zero, w2)], dim=1)
        neg = torch.stack([neg1, neg2], dim=1).reshape(2 * batch_size, *neg1.shape[1:])
        return torch.cat([pos, uncond, neg], dim=0), weights.to(torch.float32)


class DiffusionBackend:
    """The frozen prior behind the guidance, at the two seams of the reference: forward_unet (stable_diffusion_asd_guidance.py:
    319-331) and encode_images (:171-178).  The guidance talks to it through device buffers in the layouts of the C ABI
    (include/asd_hip.h: NHWC fp16 padded to 32 channels in, fp32 NHWC out), so that the fused ASD kernels write the UNet's input
    in place and nothing is re-laid-out between them and the networks:
        vae_forward(x_nhwc32) -> (moments_nhwc fp32, saved)      vae_backward(saved, d_moments_nhwc) -> dx_nhwc32
        decode_latents_bhwc(latents_bhwc fp32, (hl, wl)) -> image_bhwc fp32 in [0,1]
        unet_buffers(N, hl, wl, n_ctx, frames[, shared_reps]) -> UNetIO          unet_run(io) -> io.eps
    The product implementation is scaledreamer_amd.diffusion.engine.HipBackend (C-ABI networks).  Subclasses that only define
    `unet(latents, t, context[, camera, num_frames]) -> eps`, `encode(images[B,3,H,W] in [-1,1]) -> moments[B,8,H/8,W/8]`
    (differentiable w.r.t. the images) and, for latent-space rendering's validation images, `decode(latents[B,4,hl,wl]) ->
    images[B,3,8hl,8wl] in [-1,1]` get the buffer protocol from the adaptors below: the stand-ins of the parity tests and the
    library-op A/B tool (tools/eager_backend.py) use that."""
    scaling_factor: float = 0.18215
    context_dim: int = 1024
    camera_dim: int = 0

    def unet(self, latents: torch.Tensor, t: torch.Tensor, context: torch.Tensor, camera: Optional[torch.Tensor] = None,
             num_frames: int = 1) -> torch.Tensor:
        raise NotImplementedError

    def encode(self, images: torch.Tensor) -> torch.Tensor:
        raise NotImplementedError

    def decode(self, latents: torch.Tensor) -> torch.Tensor:
        """latents [B,4,hl,wl] (divided by the scaling factor) -> images [B,3,8hl,8wl] in [-1,1]: vae.decode of decode_latents (:191)"""
        raise NotImplementedError

    # ---- buffer protocol on top of unet() / encode() / decode() ----------------------------------------------------------------
    def decode_latents_bhwc(self, latents_bhwc: torch.Tensor, latent_hw) -> torch.Tensor:
        """rendered latents fp32 [B,h,w,4] -> image fp32 [B,8hl,8wl,3] in [0,1] (decode_latents :180-194, channels last on both sides)"""
        import torch.nn.functional as F

        z = F.interpolate(latents_bhwc.permute(0, 3, 1, 2).float(), tuple(latent_hw), mode="bilinear", align_corners=False)
        with torch.no_grad():
            img = self.decode(z * (1.0 / self.scaling_factor))
        return (img.float() * 0.5 + 0.5).clamp(0, 1).permute(0, 2, 3, 1).contiguous()

    def vae_forward(self, x_nhwc32: torch.Tensor):
        img = x_nhwc32[..., :3].permute(0, 3, 1, 2).float().detach().requires_grad_(True)
        with torch.enable_grad():
            m = self.encode(img)
        return m.detach().permute(0, 2, 3, 1).float().contiguous(), (img, m)

    def vae_backward(self, saved, d_moments_nhwc: torch.Tensor) -> torch.Tensor:
        img, m = saved
        (g,) = torch.autograd.grad(m, img, d_moments_nhwc.permute(0, 3, 1, 2).to(m.dtype))
        dx = torch.zeros(tuple(img.shape[0:1]) + tuple(img.shape[2:]) + (32,), device=img.device, dtype=torch.float16)
        dx[..., :3] = g.permute(0, 2, 3, 1)
        return dx

    def unet_buffers(self, N: int, hl: int, wl: int, n_ctx: int, frames: int = 1, shared_reps: int = 0) -> "UNetIO":
        # shared_reps: hint that the first shared_reps * N / (shared_reps + 1) entries repeat the same (x, t, camera); ignored here
        cache = self.__dict__.setdefault("_io", {})
        key = (N, hl, wl, n_ctx, frames)
        if key not in cache:
            dev = self.__dict__.get("device", None) or ("cuda" if torch.cuda.is_available() else "cpu")
            stride = (n_ctx + 7) // 8 * 8
            cache[key] = UNetIO(key, torch.zeros((N, hl, wl, 32), device=dev, dtype=torch.float16), torch.zeros(N, device=dev),
                                torch.zeros((N * stride, self.context_dim), device=dev, dtype=torch.float16),
                                torch.zeros((N, self.camera_dim), device=dev, dtype=torch.float16) if self.camera_dim else None,
                                torch.zeros((N, hl, wl, 4), device=dev))
        return cache[key]

    def unet_run(self, io: "UNetIO") -> torch.Tensor:
        N, hl, wl, n_ctx, frames = io.key
        ctx = io.context.view(N, -1, io.context.shape[-1])[:, :n_ctx].float()
        kw = {} if io.camera is None else dict(camera=io.camera.float(), num_frames=frames)
        with torch.no_grad():
            eps = self.unet(io.x[..., :4].permute(0, 3, 1, 2).float(), io.t, ctx, **kw)
        io.eps.copy_(eps.permute(0, 2, 3, 1))
        return io.eps


@dataclass
class UNetIO:
    """persistent input / output buffers of one UNet input shape (asd_unet_fwd's argument layouts)"""
    key: Tuple[int, int, int, int, int]     # (N, hl, wl, n_ctx, frames)
    x: torch.Tensor                          # fp16 [N, hl, wl, 32]
    t: torch.Tensor                          # fp32 [N]
    context: torch.Tensor                    # fp16 [N * ctx_stride, context_dim], padding rows zero
    camera: Optional[torch.Tensor]           # fp16 [N, 16] | None
    eps: torch.Tensor                        # fp32 [N, hl, wl, 4]

    def set_context(self, context: torch.Tensor) -> None:
        N, n_ctx = self.key[0], self.key[3]
        self.context.view(N, -1, self.context.shape[-1])[:, :n_ctx].copy_(context)


_BACKEND_FACTORY: Dict[str, Callable[..., DiffusionBackend]] = {}


def register_backend(name: str):
    def deco(fn):
        _BACKEND_FACTORY[name] = fn
        return fn
    return deco


WEIGHTING = {"sds": 0, "uniform": 1, "fantasia3d": 2}


class _ScoreDistillation(torch.autograd.Function):
    """loss_asd(rgb) as ONE autograd node on the fused HIP kernels of csrc/asd_glue.hip around the two frozen networks:
         forward : image_prep -> VAE encoder -> latents (+ both noisings, written into the UNet's input) -> UNet -> score (CFG /
                   Perp-Neg / w(t) / nan_to_num / loss)
         backward: latents_bwd -> VAE encoder input gradient -> image_prep adjoint
       Latent mode (job["latent_mode"], rgb_as_latents: the render carries the 4 latent channels) has no VAE in it:
         forward : latent_input (resize + both noisings) -> UNet -> score          backward: latent_input adjoint
       The loss is 0.5 * ||z - sg(z - g)||^2 / B, i.e. its value is 0.5 ||g||^2 / B and d loss / d z = g / B: g is computed once in
       the forward pass and only rescaled here."""

    @staticmethod
    def forward(ctx, rgb, backend, job):
        from ._lib import check, f32, i32, lib, ptr, stream

        l = lib()
        B, h, w, _ = rgb.shape
        H = job["image_size"]
        hl = H // 8
        C_ = 4
        dev = rgb.device
        rgb32 = rgb.detach().contiguous().float()
        latent_mode = bool(job.get("latent_mode"))
        if not latent_mode:
            x = torch.empty((B, H, H, 32), device=dev, dtype=torch.float16)
            check(l.asd_image_prep_fwd(ptr(rgb32), i32(B), i32(h), i32(w), i32(H), i32(H), ptr(x), stream()))
            moments, saved = backend.vae_forward(x)
        n_rep, n_neg = job["n_rep"], job["n_neg"]
        # the first n_rep * B entries repeat the same noised latents / timesteps / cameras under different prompts (asd_latents_fwd below)
        io = backend.unet_buffers((n_rep + 1) * B, hl, hl, job["n_ctx"], job["frames"], shared_reps=n_rep)
        neg_w = job["neg_w"]
        if job.get("context_fill") is not None:
            neg_w = job["context_fill"](io)          # asd_prompt_context: prompt selection written into io.context on the device
        else:
            io.set_context(job["context"])
        if io.camera is not None:
            io.camera.copy_(job["camera"])
        latents = torch.empty((B, C_, hl, hl), device=dev, dtype=torch.float32)
        alphas = job["alphas"]
        if latent_mode:      # the resized render is the latents: no VAE call, no VAE workspace
            check(l.asd_latent_input_fwd(ptr(rgb32), ptr(job["noise"]), ptr(job["t"]), ptr(job["t_plus"]), ptr(alphas), i32(B), i32(h), i32(w), i32(hl),
                                         i32(hl), i32(n_rep), ptr(latents), ptr(io.x), ptr(io.t), stream()))
        else:
            check(l.asd_latents_fwd(ptr(moments), ptr(job["post_noise"]), ptr(job["noise"]), ptr(job["t"]), ptr(job["t_plus"]), ptr(alphas), i32(B), i32(C_),
                                    i32(hl), i32(hl), f32(backend.scaling_factor), i32(n_rep), ptr(latents), ptr(io.x), ptr(io.t), stream()))
        eps = backend.unet_run(io)
        grad = torch.empty_like(latents)
        scratch = torch.empty(B + 2, device=dev, dtype=torch.float32)
        check(l.asd_score_fwd(ptr(eps), i32(B), i32(C_), i32(hl * hl), i32(n_neg), ptr(neg_w), f32(job["guidance_scale"]), ptr(job["t"]), ptr(alphas),
                              i32(job["weighting"]), f32(job["grad_clip"] or 0.0), ptr(grad), ptr(scratch), ptr(scratch[B:]), stream()))
        ctx.latent_mode, ctx.dims, ctx.in_dtype = latent_mode, (B, h, w, H, hl, C_), rgb.dtype
        if latent_mode:
            ctx.save_for_backward(grad)
        else:
            ctx.backend, ctx.saved_vae = backend, saved
            ctx.save_for_backward(grad, moments, job["post_noise"])
        loss, norm = scratch[B], scratch[B + 1]
        ctx.mark_non_differentiable(norm)
        return loss, norm

    @staticmethod
    def backward(ctx, d_loss, _d_norm):
        from ._lib import check, f32, i32, lib, ptr, stream

        l = lib()
        B, h, w, H, hl, C_ = ctx.dims
        up = d_loss.detach().reshape(1).float().contiguous()
        if ctx.latent_mode:
            (grad,) = ctx.saved_tensors
            d_render = torch.empty((B, h, w, 4), device=grad.device, dtype=torch.float32)
            check(l.asd_latent_input_bwd(ptr(grad), ptr(up), i32(B), i32(h), i32(w), i32(hl), i32(hl), ptr(d_render), stream()))
            return d_render.to(ctx.in_dtype), None, None
        grad, moments, post_noise = ctx.saved_tensors
        d_m = torch.empty_like(moments)
        check(l.asd_latents_bwd(ptr(grad), ptr(moments), ptr(post_noise), ptr(up), i32(B), i32(C_), i32(hl), i32(hl), f32(ctx.backend.scaling_factor),
                                ptr(d_m), stream()))
        dx = ctx.backend.vae_backward(ctx.saved_vae, d_m)
        d_rgb = torch.empty((B, h, w, 3), device=grad.device, dtype=torch.float32)
        check(l.asd_image_prep_bwd(ptr(dx), i32(B), i32(h), i32(w), i32(H), i32(H), ptr(d_rgb), stream()))
        return d_rgb.to(ctx.in_dtype), None, None


class _AsdGuidanceBase(BaseObject):
    """what the SD and the MVDream guidance share: the timestep window and its annealing, the shifted timestep t+, the random
    draws (injectable: SURVEY.md Appendix C #5/#6) and the fused score-distillation node."""

    image_size = 512

    def _setup(self, backend: DiffusionBackend) -> None:
        self.backend = backend
        self.num_train_timesteps = 1000
        lo = self.cfg.min_step_percent if isinstance(self.cfg.min_step_percent, (int, float)) else 0.02
        hi = self.cfg.max_step_percent if isinstance(self.cfg.max_step_percent, (int, float)) else 0.98
        self.set_min_max_steps(lo, hi)
        self.alphas = ddpm_alphas_cumprod(self.num_train_timesteps).to(self.device)
        self.grad_clip_val: Optional[float] = None
        if self.cfg.weighting_strategy not in WEIGHTING:
            raise ValueError(f"Unknown weighting strategy: {self.cfg.weighting_strategy}")
        # the four random draws of a step, in the reference's order; tests replace them for "identical inputs"
        self.posterior_noise_fn = torch.randn_like
        self.noise_fn = torch.randn_like
        self.timestep_fn = lambda lo, hi, n, device: torch.randint(lo, hi, [n], dtype=torch.long, device=device)
        self.rand_fn = lambda shape, device: torch.rand(*shape, device=device)

    def set_min_max_steps(self, min_step_percent=0.02, max_step_percent=0.98):
        self.min_step = int(self.num_train_timesteps * min_step_percent)
        self.max_step = int(self.num_train_timesteps * max_step_percent)

    def update_step(self, epoch: int, global_step: int, on_load_weights: bool = False):
        if self.cfg.grad_clip is not None:
            self.grad_clip_val = C(self.cfg.grad_clip, epoch, global_step)
        self.set_min_max_steps(C(self.cfg.min_step_percent, epoch, global_step), C(self.cfg.max_step_percent, epoch, global_step))

    def get_t_plus(self, t: torch.Tensor) -> torch.Tensor:
        """t+ = clamp(t + floor(u * clamp(plus_ratio * (t - min_step), 0, T - 1 - t)), 1, T - 1), u = 1 or U[0,1) per element
        (stable_diffusion_asd_guidance.py:294-316)."""
        if self.cfg.plus_ratio < 0.0:
            raise AssertionError("plus_ratio must be >= 0")
        T = self.num_train_timesteps
        if t.is_cuda and t.dtype == torch.long:        # one launch (asd_timestep_plus) instead of a dozen one-element tensor ops
            import ctypes as C

            from . import _lib

            t = t.contiguous()
            u = self.rand_fn(t.shape, t.device).float().contiguous() if self.cfg.plus_random else None
            out = torch.empty_like(t)
            _lib.check(_lib.lib().asd_timestep_plus(_lib.ptr(t), _lib.ptr(u), _lib.i32(t.numel()), C.c_int64(int(self.min_step)), C.c_int64(int(T)),
                                                    _lib.f32(float(self.cfg.plus_ratio)), _lib.ptr(out), _lib.stream()))
            return out
        room = (self.cfg.plus_ratio * (t - self.min_step)).clamp(torch.zeros_like(t), T - t - 1)
        if self.cfg.plus_random:
            room = room * self.rand_fn(t.shape, t.device)
        return (t + room.to(torch.long)).clamp(1, T - 1)

    @staticmethod
    def _check_channels(rgb: torch.Tensor, rgb_as_latents: bool) -> None:
        if rgb_as_latents and (rgb.dim() != 4 or rgb.shape[-1] != 4):
            raise ValueError(f"rgb_as_latents=True needs a render of 4 latent channels [B,h,w,4]; got {rgb.shape[-1]} channels "
                             f"(shape {tuple(rgb.shape)})")

    def _distill(self, rgb: torch.Tensor, context: Optional[torch.Tensor], neg_w: Optional[torch.Tensor], n_rep: int, shared_t: bool,
                 camera: Optional[torch.Tensor] = None, frames: int = 1, context_fill=None, n_ctx: Optional[int] = None,
                 n_neg: Optional[int] = None, rgb_as_latents: bool = False) -> Dict[str, Any]:
        """context [ (n_rep + 1) * B, n_ctx, D ] + neg_w [B, n_neg], or context_fill(io) -> neg_w which writes io.context itself"""
        if not rgb.is_cuda:
            from ._lib import AsdError

            raise AsdError("the ASD guidance runs on the HIP path only (device tensors; there is no CPU fallback)")
        B, dev, hl = rgb.shape[0], rgb.device, self.image_size // 8
        like = torch.empty((B, 4, hl, hl), device=dev, dtype=torch.float32)
        # latent mode has no posterior to sample: the reference draws only `noise` there, and the draw order is the contract
        post_noise = None if rgb_as_latents else self.posterior_noise_fn(like).float().contiguous()        # VAE posterior sample
        noise = self.noise_fn(like).float().contiguous()                        # shared by both timesteps
        t = self.timestep_fn(self.min_step, self.max_step + 1, 1 if shared_t else B, dev).to(dev)
        t_plus = self.get_t_plus(t)
        if shared_t:                                                             # one t for the views of a group
            t, t_plus = t.repeat(B), t_plus.repeat(B)
        if n_neg is None:
            n_neg = 0 if neg_w is None else neg_w.shape[1]
        job = dict(image_size=self.image_size, n_rep=n_rep, n_neg=n_neg, frames=frames, context_fill=context_fill, latent_mode=rgb_as_latents,
                   n_ctx=context.shape[1] if n_ctx is None else n_ctx, context=context, camera=camera, post_noise=post_noise, noise=noise, t=t.contiguous(), t_plus=t_plus.contiguous(),
                   alphas=self.alphas.to(dev), neg_w=None if neg_w is None else neg_w.float().contiguous(),
                   guidance_scale=float(self.cfg.guidance_scale), weighting=WEIGHTING[self.cfg.weighting_strategy], grad_clip=self.grad_clip_val)
        loss, norm = _ScoreDistillation.apply(rgb, self.backend, job)
        return {"loss_asd": loss, "grad_norm": norm, "min_step": self.min_step, "max_step": self.max_step}


@register("stable-diffusion-asynchronous-score-distillation-guidance")
class SDTimestepShiftedScoreDistillationGuidance(_AsdGuidanceBase):
    @dataclass
    class Config(BaseObject.Config):
        pretrained_model_name_or_path: str = "stabilityai/stable-diffusion-2-1-base"
        enable_memory_efficient_attention: bool = False
        enable_sequential_cpu_offload: bool = False
        enable_attention_slicing: bool = False
        enable_channels_last_format: bool = True
        guidance_scale: float = 7.5
        grad_clip: Optional[Any] = None
        half_precision_weights: bool = True
        min_step_percent: Any = 0.02
        max_step_percent: Any = 0.98
        weighting_strategy: str = "sds"
        plus_ratio: float = 0.1
        plus_random: bool = False
        view_dependent_prompting: bool = True
        guidance_perp_neg: float = 0.0
        # build-specific: which DiffusionBackend executes the frozen prior, and the seed of the random-init
        # weights used when no checkpoint exists at pretrained_model_name_or_path (none exists offline)
        backend: str = "hip"
        weights_seed: int = 1
        allow_random_weights: bool = False     # without it a missing checkpoint is an error, never a silent random prior

    cfg: Config
    image_size = 512                           # get_latents resizes to 512x512 before the VAE (:204)

    def configure(self, backend: Optional[DiffusionBackend] = None) -> None:
        info("Loading Stable Diffusion ...")
        if not self.cfg.half_precision_weights and backend is None and self.cfg.backend == "hip":
            # the engine holds fp16 weights and activations with fp32 accumulation (the reference's own arithmetic for this config,
            # asd_sd_nerf.yaml: half_precision_weights: true); an fp32 prior is not implemented — refuse instead of running fp16 silently
            raise NotImplementedError("half_precision_weights: false — the HIP diffusion engine is fp16 / fp32-accumulate only")
        self.weights_dtype = torch.float16 if self.cfg.half_precision_weights else torch.float32
        if backend is None:
            if self.cfg.backend not in _BACKEND_FACTORY:
                from .diffusion import engine  # noqa: F401  (registers "hip" / "hip-mvdream"; raises if libasd_hip.so is missing)
            backend = _BACKEND_FACTORY[self.cfg.backend](self.cfg, self.device, self.weights_dtype)
        self._setup(backend)
        self.use_perp_neg = self.cfg.guidance_perp_neg != 0
        info(f"Loaded Stable Diffusion! ({getattr(self.backend, 'weights_source', 'caller-supplied backend')})")

    def conditioning(self, prompt_utils, elevation, azimuth, camera_distances):
        """UNet context in the batch order of get_eps (:377-394): text | uncond | (2 negatives per sample) | text (the shifted-t
        branch), and the Perp-Neg weights scaled by -guidance_perp_neg."""
        B = elevation.shape[0]
        if self.use_perp_neg:
            if not prompt_utils.use_perp_neg:
                raise AssertionError("guidance_perp_neg needs a prompt processor with use_perp_neg")
            emb, w = prompt_utils.get_text_embeddings_perp_neg(elevation, azimuth, camera_distances, self.cfg.view_dependent_prompting)
            return torch.cat([emb, emb[:B]], dim=0), w * (-1.0 * self.cfg.guidance_perp_neg)
        emb = prompt_utils.get_text_embeddings(elevation, azimuth, camera_distances, self.cfg.view_dependent_prompting)
        return torch.cat([emb, emb[:B]], dim=0), None

    def __call__(self, rgb: torch.Tensor, prompt_utils, elevation, azimuth, camera_distances, rgb_as_latents=False,
                 guidance_eval=False, **kwargs) -> Dict[str, Any]:
        self._check_channels(rgb, rgb_as_latents)
        fill = self._device_conditioning(prompt_utils, elevation, azimuth, rgb) if rgb.is_cuda else None
        if fill is not None:
            return self._distill(rgb, None, None, 4 if self.use_perp_neg else 2, shared_t=False, context_fill=fill,
                                 n_ctx=prompt_utils.text_embeddings_vd.shape[1], n_neg=2 if self.use_perp_neg else 0, rgb_as_latents=rgb_as_latents)
        context, neg_w = self.conditioning(prompt_utils, elevation, azimuth, camera_distances)
        n_rep = context.shape[0] // rgb.shape[0] - 1
        return self._distill(rgb, context.to(rgb.device), None if neg_w is None else neg_w.to(rgb.device), n_rep, shared_t=False,
                             rgb_as_latents=rgb_as_latents)

    def decode_latents(self, latents: torch.Tensor, latent_height: int = 64, latent_width: int = 64) -> torch.Tensor:
        """stable_diffusion_asd_guidance.py:180-194: latents [B,4,H,W] -> bilinear resize to (latent_height, latent_width), 1 / scaling
        factor, VAE decoder, clamp(0.5 x + 0.5, 0, 1) -> [B,3,8 latent_height,8 latent_width] in the input's dtype."""
        if latents.dim() != 4 or latents.shape[1] != 4:
            raise ValueError(f"decode_latents needs latents [B,4,H,W]; got {latents.shape[1] if latents.dim() == 4 else '?'} channels "
                             f"(shape {tuple(latents.shape)})")
        img = self.backend.decode_latents_bhwc(latents.detach().permute(0, 2, 3, 1).float().contiguous(), (latent_height, latent_width))
        return img.permute(0, 3, 1, 2).to(latents.dtype)

    def _device_conditioning(self, prompt_utils, elevation, azimuth, rgb):
        """`conditioning` as one kernel launch that writes the UNet's context buffer (csrc/asd_glue.hip: asd_prompt_context) — for the
        stock PromptUtils; any other prompt processor goes through its own get_text_embeddings* methods."""
        if type(prompt_utils) is not PromptUtils:
            return None
        vd = self.cfg.view_dependent_prompting
        if self.use_perp_neg and not (vd and prompt_utils.use_perp_neg):
            return None                                  # conditioning() raises the reference's errors for these
        import ctypes as C_

        from ._lib import check, f32, i32, lib, ptr, stream

        dev = rgb.device
        key = (id(prompt_utils), vd, str(dev))
        cache = self.__dict__.setdefault("_prompt_tables", {})
        if key not in cache:                             # fp32 tables on the device, once per prompt processor
            if vd:
                text, unc = prompt_utils.text_embeddings_vd, prompt_utils.uncond_text_embeddings_vd
            else:
                text, unc = prompt_utils.text_embeddings[None], prompt_utils.uncond_text_embeddings[None]
            pu = prompt_utils
            params = [pu.overhead_threshold, pu.front_threshold, pu.back_threshold, *pu.perp_neg_f_sb, *pu.perp_neg_f_fsb, *pu.perp_neg_f_fs,
                      *pu.perp_neg_f_sf]
            cache[key] = (text.to(dev, torch.float32).contiguous(), unc.to(dev, torch.float32).contiguous(), (C_.c_float * 15)(*params), prompt_utils)
        text, unc, params, _keep = cache[key]
        B = rgb.shape[0]
        el, az = elevation.to(dev, torch.float32).contiguous(), azimuth.to(dev, torch.float32).contiguous()
        perp, scale = self.use_perp_neg, -1.0 * self.cfg.guidance_perp_neg

        def fill(io):
            n_tok, dim = text.shape[1], text.shape[2]
            stride = io.context.shape[0] // io.key[0]
            w = torch.empty((B, 2), device=dev, dtype=torch.float32) if perp else None
            check(lib().asd_prompt_context(ptr(text), ptr(unc), i32(text.shape[0]), i32(n_tok), i32(dim), ptr(el), ptr(az), i32(B), i32(int(perp)),
                                           params, f32(scale), ptr(io.context), i32(stride), ptr(w), stream()))
            return w

        return fill


def normalize_camera(camera_matrix: torch.Tensor) -> torch.Tensor:
    """extern/mvdream/camera_utils.py:45-57: camera location projected onto the unit sphere, flattened to [B,16]."""
    cam = camera_matrix.reshape(-1, 4, 4).clone()
    tr = cam[:, :3, 3]
    cam[:, :3, 3] = tr / (torch.norm(tr, dim=1, keepdim=True) + 1e-8)
    return cam.reshape(-1, 16)


@register("mvdream-asynchronous-score-distillation-guidance")
class MVDreamTimestepShiftedScoreDistillationGuidance(_AsdGuidanceBase):
    """threestudio/models/guidance/mvdream_asd_guidance.py:26-304: 4-view groups share one timestep, the UNet batch is
    [x_t | x_t | x_t+] with contexts [cond | uncond | cond], camera-conditioned with cross-view self-attention, plain CFG
    (no Perp-Neg), VAE at 256x256 -> 32x32 latents."""

    @dataclass
    class Config(BaseObject.Config):
        model_name: str = "sd-v2.1-base-4view"
        ckpt_path: Optional[str] = None
        grad_clip: Optional[Any] = None
        half_precision_weights: bool = True
        guidance_scale: float = 7.5
        n_view: int = 4
        min_step_percent: Any = 0.02
        max_step_percent: Any = 0.98
        weighting_strategy: str = "sds"
        plus_ratio: float = 0.1
        plus_random: bool = False
        camera_condition_type: str = "rotation"
        view_dependent_prompting: bool = False
        backend: str = "hip-mvdream"
        weights_seed: int = 1
        allow_random_weights: bool = False

    cfg: Config
    image_size = 256                           # mvdream_asd_guidance.py:133-135

    def configure(self, backend: Optional[DiffusionBackend] = None) -> None:
        info("Loading Multiview Diffusion ...")
        if backend is None:
            if self.cfg.backend not in _BACKEND_FACTORY:
                from .diffusion import engine  # noqa: F401
            # The reference builds this model in fp32 (mvdream_asd_guidance.py:40,67: `half_precision_weights` is declared but never
            # applied).  The HIP engine computes in fp16 operands with fp32 accumulation for both priors; the deviation from the
            # fp32 reference is bounded at full width by tests/test_gpu_unet_engine.py::test_full_mvdream_unet_b12_matches_reference_golden
            # (< 1e-2, north_star's tolerance) and reported as such by bench.py (`dtype`).
            backend = _BACKEND_FACTORY[self.cfg.backend](self.cfg, self.device, torch.float16)
        self.weights_dtype = torch.float16
        self._setup(backend)

    def get_camera_cond(self, camera: torch.Tensor, fovy=None) -> torch.Tensor:
        if self.cfg.camera_condition_type != "rotation":
            raise NotImplementedError(f"Unknown camera_condition_type={self.cfg.camera_condition_type}")
        return normalize_camera(camera).flatten(start_dim=1)

    def __call__(self, rgb: torch.Tensor, prompt_utils, elevation, azimuth, camera_distances, c2w, rgb_as_latents: bool = False,
                 fovy=None, input_is_latent=False, **kwargs) -> Dict[str, Any]:
        if input_is_latent:       # (the reference declares the argument and never reads it, mvdream_asd_guidance.py:177)
            raise NotImplementedError("input_is_latent is not implemented; latent-space rendering is rgb_as_latents=True")
        self._check_channels(rgb, rgb_as_latents)
        if c2w is None:
            raise NotImplementedError("the multi-view prior is camera-conditioned: c2w is required")
        B = rgb.shape[0]
        emb = prompt_utils.get_text_embeddings(elevation, azimuth, camera_distances, self.cfg.view_dependent_prompting)
        half = emb.shape[0] // 2
        cond, uncond = emb[:half].repeat(B // half, 1, 1), emb[half:].repeat(B // half, 1, 1)
        context = torch.cat([cond, uncond, cond], dim=0).to(rgb.device)
        camera = self.get_camera_cond(c2w, fovy).repeat(3, 1).to(rgb.device)
        return self._distill(rgb, context, None, n_rep=2, shared_t=True, camera=camera, frames=self.cfg.n_view, rgb_as_latents=rgb_as_latents)
