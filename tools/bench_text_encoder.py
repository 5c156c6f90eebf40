"""Strings per second of the CLIP text encoder on the HIP path (diffusion/text_hip.HipClipTextEncoder) at the SD-2.1 size with seeded random
weights, against the same arithmetic run as fp16 PyTorch-ROCm library ops on the same GPU in the same process, in alternating batches with
warm-up; and the split of one HIP batch between its kinds of calls.  Off the step path: the figures are reported, not gated.

  python tools/bench_text_encoder.py [--strings 1024] [--chunk 256] [--iters 5] [--warmup 2] [--rounds 3] [--layers 23]

Prints one JSON line: median / min time of a batch of both sides in ms (device events around the whole call, ids already on the host),
strings per second from the medians, the largest difference between the two last_hidden_states, and the share of a bracketed HIP batch
spent in GEMMs, causal attention, GELU, LayerNorm and the embedding (device events around every call of that kind; the brackets add
host work, so the shares are of the bracketed batch, not of the timed one).
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

SD21_TEXT = dict(vocab_size=49408, hidden_size=1024, intermediate_size=4096, num_hidden_layers=23, num_attention_heads=16, max_position_embeddings=77,
                 hidden_act="gelu", layer_norm_eps=1e-5, eos_token_id=2)


def random_state(cfg: dict, seed: int):
    """HF's keys with seeded values that keep activations O(1), fp16"""
    g = torch.Generator().manual_seed(seed)
    C_, I = cfg["hidden_size"], cfg["intermediate_size"]
    rn = lambda *s, std=1.0: (torch.randn(*s, generator=g) * std).half()
    sd = {"embeddings.token_embedding.weight": rn(cfg["vocab_size"], C_, std=0.5),
          "embeddings.position_embedding.weight": rn(cfg["max_position_embeddings"], C_, std=0.5),
          "final_layer_norm.weight": (1.0 + 0.1 * torch.randn(C_, generator=g)).half(), "final_layer_norm.bias": rn(C_, std=0.1)}
    for i in range(cfg["num_hidden_layers"]):
        p = f"encoder.layers.{i}."
        for n in ("layer_norm1", "layer_norm2"):
            sd[p + n + ".weight"], sd[p + n + ".bias"] = (1.0 + 0.1 * torch.randn(C_, generator=g)).half(), rn(C_, std=0.1)
        for n in ("q_proj", "k_proj", "v_proj", "out_proj"):
            sd[p + f"self_attn.{n}.weight"], sd[p + f"self_attn.{n}.bias"] = rn(C_, C_, std=C_ ** -0.5), rn(C_, std=0.1)
        sd[p + "mlp.fc1.weight"], sd[p + "mlp.fc1.bias"] = rn(I, C_, std=C_ ** -0.5), rn(I, std=0.1)
        sd[p + "mlp.fc2.weight"], sd[p + "mlp.fc2.bias"] = rn(C_, I, std=I ** -0.5), rn(C_, std=0.1)
    return sd


def torch_tower(w, cfg: dict, ids: torch.Tensor, chunk: int) -> torch.Tensor:
    """CLIPTextModel.forward as torch library ops on fp16 tensors (w: HF's keys on the device), in the same chunks: last_hidden_state"""
    heads, eps = cfg["num_attention_heads"], cfg["layer_norm_eps"]
    outs = []
    for i in range(0, ids.shape[0], chunk):
        part = ids[i:i + chunk]
        n, T = part.shape
        x = F.embedding(part, w["embeddings.token_embedding.weight"]) + w["embeddings.position_embedding.weight"][:T]
        C_ = x.shape[-1]
        split = lambda t: t.view(n, T, heads, C_ // heads).transpose(1, 2)
        for layer in range(cfg["num_hidden_layers"]):
            p = f"encoder.layers.{layer}."
            lin = lambda t, nm: F.linear(t, w[p + nm + ".weight"], w[p + nm + ".bias"])
            h = F.layer_norm(x, (C_,), w[p + "layer_norm1.weight"], w[p + "layer_norm1.bias"], eps)
            a = F.scaled_dot_product_attention(split(lin(h, "self_attn.q_proj")), split(lin(h, "self_attn.k_proj")), split(lin(h, "self_attn.v_proj")),
                                               is_causal=True)
            x = x + lin(a.transpose(1, 2).reshape(n, T, C_), "self_attn.out_proj")
            h = F.layer_norm(x, (C_,), w[p + "layer_norm2.weight"], w[p + "layer_norm2.bias"], eps)
            x = x + lin(F.gelu(lin(h, "mlp.fc1")), "mlp.fc2")
        outs.append(F.layer_norm(x, (C_,), w["final_layer_norm.weight"], w["final_layer_norm.bias"], eps))
    return torch.cat(outs)


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


def split_of_a_batch(enc, ids) -> dict:
    """ms per kind of call over one batch: every call of the module-level entries of text_hip bracketed by device events"""
    from scaledreamer_amd.diffusion import text_hip as TH

    names = {"gemm": "gemm", "causal_attention": "attention", "gelu": "gelu", "quick_gelu": "gelu", "layernorm": "layernorm", "embed": "embed"}
    events, saved = {k: [] for k in set(names.values())}, {}
    for fn_name, kind in names.items():
        fn = saved[fn_name] = getattr(TH, fn_name)

        def bracketed(*a, _fn=fn, _kind=kind, **kw):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = _fn(*a, **kw)
            e1.record()
            events[_kind].append((e0, e1))
            return out

        setattr(TH, fn_name, bracketed)
    try:
        enc(ids)
        torch.cuda.synchronize()
    finally:
        for fn_name, fn in saved.items():
            setattr(TH, fn_name, fn)
    return {k: sum(a.elapsed_time(b) for a, b in v) for k, v in events.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--strings", type=int, default=1024)
    ap.add_argument("--chunk", type=int, default=256)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--layers", type=int, default=SD21_TEXT["num_hidden_layers"])
    ap.add_argument("--seed", type=int, default=31)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_text_encoder needs a GPU: a CPU timing says nothing about this path")
    from scaledreamer_amd.diffusion.text_hip import HipClipTextEncoder

    dev = torch.device("cuda", 0)
    cfg = dict(SD21_TEXT, num_hidden_layers=a.layers)
    sd = random_state(cfg, a.seed)
    enc = HipClipTextEncoder(sd, cfg, dev, chunk=a.chunk)
    w16 = {k: v.to(dev) for k, v in sd.items()}
    g = torch.Generator().manual_seed(a.seed + 1)
    ids = torch.randint(3, cfg["vocab_size"] - 2, (a.strings, 77), generator=g)
    ids[:, 0] = cfg["vocab_size"] - 2
    for r in range(a.strings):                     # an end token (the highest id) somewhere in every row, padding after it
        p = 2 + (r * 7) % 74
        ids[r, p], ids[r, p + 1:] = cfg["vocab_size"] - 1, 0
    ids_dev = ids.to(dev)
    hip = lambda: enc(ids)[0]
    lib_ops = lambda: torch_tower(w16, cfg, ids_dev, a.chunk)
    with torch.no_grad():
        for _ in range(a.warmup):
            out_h, out_t = hip(), lib_ops()
        torch.cuda.synchronize()
        th, tt = [], []
        for _ in range(a.rounds):                  # alternate the two sides: other work shares the host
            th += _time(hip, a.iters)
            tt += _time(lib_ops, a.iters)
        split = split_of_a_batch(enc, ids)
    total = sum(split.values())
    result = {"what": "clip_text_encoder", "gpu": torch.cuda.get_device_name(0), "config": {k: cfg[k] for k in ("hidden_size", "num_hidden_layers", "intermediate_size", "hidden_act")},
              "strings": a.strings, "chunk": a.chunk, "runs_per_side": a.rounds * a.iters,
              "hip_ms_median": statistics.median(th), "hip_ms_min": min(th), "torch_fp16_ms_median": statistics.median(tt), "torch_fp16_ms_min": min(tt),
              "hip_strings_per_s": a.strings / statistics.median(th) * 1e3, "torch_fp16_strings_per_s": a.strings / statistics.median(tt) * 1e3,
              "max_abs_diff_last_hidden_state": float((out_h.float() - out_t.float()).abs().max()),
              "bracketed_batch_ms": total, "split_ms": split, "split_share": {k: v / total for k, v in split.items()}}
    print(json.dumps(result))


if __name__ == "__main__":
    main()
