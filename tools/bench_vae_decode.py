"""Time per `decode_latents` call on the HIP path against the same VAE decoder run as fp16 PyTorch-ROCm library ops, same GPU, same
process, alternating, with warm-up.  Evaluation-time path: the figure is reported, not gated.

  python tools/bench_vae_decode.py [--batches 1 4] [--latent 64] [--ch 128] [--iters 10] [--warmup 3] [--rounds 3]

Prints one JSON line: per batch the chunk the HIP path walked it in and its workspace, the median / min call time of both sides in ms
(device events around the whole call) and the largest difference between the two images.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from scaledreamer_amd.diffusion import weights as W  # noqa: E402


def torch_decoder(p, cfg: W.VAEConfig, z: torch.Tensor) -> torch.Tensor:
    """post_quant_conv + Decoder.forward (model.py:619-655) as torch library ops in z's dtype; z [B,4,hl,wl] already divided by the
    scaling factor -> [B,3,8hl,8wl] before any clamp.  `p`: LDM-named parameters on z's device and dtype."""

    def gn(x, name, silu=True):
        y = F.group_norm(x, 32, p[name + ".weight"], p[name + ".bias"], 1e-6)
        return F.silu(y) if silu else y

    def conv(x, name, pad=1):
        return F.conv2d(x, p[name + ".weight"], p[name + ".bias"], padding=pad)

    def res(x, name):
        h = conv(gn(x, name + ".norm1"), name + ".conv1")
        h = conv(gn(h, name + ".norm2"), name + ".conv2")
        if name + ".nin_shortcut.weight" in p:
            x = conv(x, name + ".nin_shortcut", 0)
        return x + h

    def attn(x, name):
        B, Cc, Hh, Ww = x.shape
        h = gn(x, name + ".norm", silu=False)
        q, k, v = (conv(h, f"{name}.{n}", 0).reshape(B, Cc, Hh * Ww) for n in ("q", "k", "v"))
        w = torch.softmax(torch.bmm(q.permute(0, 2, 1), k) * (int(Cc) ** -0.5), dim=2)
        h = torch.bmm(v, w.permute(0, 2, 1)).reshape(B, Cc, Hh, Ww)
        return x + conv(h, name + ".proj_out", 0)

    h = conv(conv(z, "post_quant_conv", 0), "decoder.conv_in")
    h = res(h, "decoder.mid.block_1")
    h = attn(h, "decoder.mid.attn_1")
    h = res(h, "decoder.mid.block_2")
    for lvl in reversed(range(len(cfg.ch_mult))):
        for b in range(cfg.num_res_blocks + 1):
            h = res(h, f"decoder.up.{lvl}.block.{b}")
        if lvl != 0:
            h = conv(F.interpolate(h, scale_factor=2.0, mode="nearest"), f"decoder.up.{lvl}.upsample.conv")
    return conv(gn(h, "decoder.norm_out"), "decoder.conv_out")


def torch_decode_latents(p, cfg: W.VAEConfig, latents_bchw: torch.Tensor, latent_hw, dtype=torch.float16):
    """decode_latents (stable_diffusion_asd_guidance.py:180-194) on library ops: (image in [0,1], pre-clamp output), fp32 NCHW"""
    z = F.interpolate(latents_bchw.float(), tuple(latent_hw), mode="bilinear", align_corners=False) * (1.0 / cfg.scale_factor)
    raw = torch_decoder(p, cfg, z.to(dtype)).float()
    return (raw * 0.5 + 0.5).clamp(0, 1), raw


def _time(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    out = []
    for _ in range(iters):
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 4])
    ap.add_argument("--latent", type=int, default=64)
    ap.add_argument("--ch", type=int, default=128)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--seed", type=int, default=22)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_vae_decode needs a GPU: a CPU timing says nothing about this path")
    from scaledreamer_amd.diffusion.vae_hip import HipVAEDecoder

    dev = torch.device("cuda", 0)
    cfg = W.VAEConfig(ch=a.ch)
    params = W.gen_params(W.vae_decoder_layout(cfg)[0], a.seed)
    dec = HipVAEDecoder(params, cfg, dev)
    p16 = {k: v.to(dev, torch.float16) for k, v in params.items()}
    result = {"what": "decode_latents", "latent": a.latent, "image": a.latent * dec.up, "ch": a.ch, "gpu": torch.cuda.get_device_name(0), "cases": []}
    for B in a.batches:
        g = torch.Generator().manual_seed(a.seed + B)
        lat = (torch.randn(B, a.latent, a.latent, 4, generator=g) * cfg.scale_factor).to(dev)
        lat_bchw = lat.permute(0, 3, 1, 2).contiguous()
        hw = (a.latent, a.latent)
        hip = lambda: dec(lat, hw)
        lib_ops = lambda: torch_decode_latents(p16, cfg, lat_bchw, hw)[0]
        with torch.no_grad():
            for _ in range(a.warmup):
                img_h, img_t = hip(), lib_ops()
            torch.cuda.synchronize()
            th, tt = [], []
            for _ in range(a.rounds):            # alternate the two sides: other work shares the host
                th += _time(hip, a.iters)
                tt += _time(lib_ops, a.iters)
        result["cases"].append({"batch": B, "chunk": dec.chunk_for(B, *hw), "workspace_bytes": dec.workspace_bytes(dec.chunk_for(B, *hw), *hw),
                                "hip_ms_median": statistics.median(th), "hip_ms_min": min(th), "torch_fp16_ms_median": statistics.median(tt),
                                "torch_fp16_ms_min": min(tt), "max_abs_image_diff": float((img_h.permute(0, 3, 1, 2) - img_t).abs().max())})
    print(json.dumps(result))


if __name__ == "__main__":
    main()
