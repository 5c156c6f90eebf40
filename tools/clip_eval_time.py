"""Throughput of the CLIP image tower on the HIP path at the evaluation's size: ViT-L/14 with seeded random weights, a batch
of 120 frames of 512 x 1536 (three-panel test grids), scored against 415 random text features.

    python tools/clip_eval_time.py [--batch 120] [--reps 20]

Three figures, one JSON line:
  * images/s of ClipVisionTower (front end, tower, projection) — the median batch, host clock around a device synchronise, after two
    warm-up batches (the first call of a GEMM shape tunes its plan);
  * images/s of the same arithmetic as torch fp16 eager ops (F.linear, F.layer_norm, F.scaled_dot_product_attention) behind the same HIP
    front end, in runs that alternate with the HIP tower's;
  * the share of a bracketed batch (tower + scoring) spent in the entries of csrc/clip.hip: each call of preprocess / embed / quick_gelu /
    score is bracketed by device synchronises and summed.
useful_tflops counts the GEMM and attention operations of 257 tokens per image over the HIP tower's time: a whole-program rate."""
import argparse
import json
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

VIT_L14 = dict(hidden_size=1024, intermediate_size=4096, num_hidden_layers=24, num_attention_heads=16, image_size=224, patch_size=14,
               projection_dim=768, layer_norm_eps=1e-5, hidden_act="quick_gelu")


def random_state(cfg, device):
    g = torch.Generator(device=device).manual_seed(7)
    C_, I, D, P = cfg["hidden_size"], cfg["intermediate_size"], cfg["projection_dim"], cfg["patch_size"]
    L = (cfg["image_size"] // P) ** 2 + 1
    rn = lambda *s, std=1.0: torch.randn(*s, generator=g, device=device) * std
    sd = {"vision_model.embeddings.class_embedding": rn(C_, std=0.5),
          "vision_model.embeddings.patch_embedding.weight": rn(C_, 3, P, P, std=(3 * P * P) ** -0.5),
          "vision_model.embeddings.position_embedding.weight": rn(L, C_, std=0.5), "visual_projection.weight": rn(D, C_, std=C_ ** -0.5)}
    norms = ["vision_model.pre_layrnorm", "vision_model.post_layernorm"]
    for i in range(cfg["num_hidden_layers"]):
        p = f"vision_model.encoder.layers.{i}."
        norms += [p + "layer_norm1", p + "layer_norm2"]
        for n in ("q_proj", "k_proj", "v_proj", "out_proj"):
            sd[p + f"self_attn.{n}.weight"], sd[p + f"self_attn.{n}.bias"] = rn(C_, C_, std=C_ ** -0.5), rn(C_, std=0.1)
        sd[p + "mlp.fc1.weight"], sd[p + "mlp.fc1.bias"] = rn(I, C_, std=C_ ** -0.5), rn(I, std=0.1)
        sd[p + "mlp.fc2.weight"], sd[p + "mlp.fc2.bias"] = rn(C_, I, std=I ** -0.5), rn(C_, std=0.1)
    for n in norms:
        sd[n + ".weight"], sd[n + ".bias"] = 1.0 + rn(C_, std=0.1), rn(C_, std=0.1)
    return sd


class EagerTower:
    """the tower's arithmetic as torch fp16 ops, from the patch rows of the HIP front end"""

    def __init__(self, sd, cfg, tower):
        self.w = {k: v.half() for k, v in sd.items()}
        self.cfg, self.tower = cfg, tower

    @torch.no_grad()
    def __call__(self, frames):
        from scaledreamer_amd import clip_eval as CE

        w, cfg, t = self.w, self.cfg, self.tower
        B, C_, heads, eps = frames.shape[0], t.C, t.heads, t.eps
        ln = lambda x, n: F.layer_norm(x, (C_,), w[n + ".weight"], w[n + ".bias"], eps)
        x = (CE.preprocess(frames, t.S, t.P) @ t.w_patch.t()).view(B, -1, C_)
        e = "vision_model.embeddings."
        x = ln(torch.cat([w[e + "class_embedding"].expand(B, 1, C_), x], 1) + w[e + "position_embedding.weight"], "vision_model.pre_layrnorm")
        split = lambda y: y.view(B, -1, heads, 64).transpose(1, 2)
        for i in range(cfg["num_hidden_layers"]):
            p = f"vision_model.encoder.layers.{i}."
            lin = lambda y, n: F.linear(y, w[p + n + ".weight"], w[p + n + ".bias"])
            h = ln(x, p + "layer_norm1")
            a = F.scaled_dot_product_attention(split(lin(h, "self_attn.q_proj")), split(lin(h, "self_attn.k_proj")), split(lin(h, "self_attn.v_proj")))
            x = x + lin(a.transpose(1, 2).reshape(B, -1, C_), "self_attn.out_proj")
            f = lin(ln(x, p + "layer_norm2"), "mlp.fc1")
            x = x + lin(f * torch.sigmoid(1.702 * f), "mlp.fc2")
        return (ln(x[:, 0], "vision_model.post_layernorm") @ w["visual_projection.weight"].t()).float()


def useful_flops(cfg):
    C_, I, P = cfg["hidden_size"], cfg["intermediate_size"], cfg["patch_size"]
    g2 = (cfg["image_size"] // P) ** 2
    L = g2 + 1
    layer = 2 * L * C_ * 3 * C_ + 4 * L * L * C_ + 2 * L * C_ * C_ + 4 * L * C_ * I
    return 2 * g2 * 3 * P * P * C_ + cfg["num_hidden_layers"] * layer + 2 * C_ * cfg["projection_dim"]


def timed(fn, *args):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn(*args)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=120)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--height", type=int, default=512)
    ap.add_argument("--width", type=int, default=1536)
    ap.add_argument("--prompts", type=int, default=415)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    from scaledreamer_amd import clip_eval as CE

    dev = torch.device("cuda")
    cfg = dict(VIT_L14)
    sd = random_state(cfg, dev)
    tower = CE.ClipVisionTower(sd, cfg, dev)
    eager = EagerTower(sd, cfg, tower)
    g = torch.Generator(device=dev).manual_seed(8)
    frames = torch.randint(0, 256, (a.batch, a.height, a.width, 3), generator=g, device=dev, dtype=torch.uint8)
    txt = F.normalize(torch.randn(a.prompts, cfg["projection_dim"], generator=g, device=dev), dim=-1)
    own = torch.zeros(a.batch, dtype=torch.int32, device=dev)
    with torch.no_grad():
        for _ in range(2):
            e_hip, e_ref = tower(frames), eager(frames)
        n = lambda t: F.normalize(t.double(), dim=-1)
        diff = float((n(e_hip) - n(e_ref)).abs().max())
        hip_s, eager_s = [], []
        for _ in range(a.reps):
            hip_s.append(timed(tower, frames)[0])
            eager_s.append(timed(eager, frames)[0])
        spent = {}

        def bracket(name):
            fn = getattr(CE, name)

            def wrapped(*args, **kw):
                t, out = timed(lambda: fn(*args, **kw))
                spent[name] = spent.get(name, 0.0) + t
                return out
            return fn, wrapped

        saved = {}
        for name in ("preprocess", "embed", "quick_gelu", "score"):
            saved[name], wrapped = bracket(name)
            setattr(CE, name, wrapped)
        try:
            whole, _ = timed(lambda: CE.score(tower(frames), txt, own))
        finally:
            for name, fn in saved.items():
                setattr(CE, name, fn)
    hip, eag = statistics.median(hip_s), statistics.median(eager_s)
    print(json.dumps({"model": "ViT-L/14 random weights", "batch": a.batch, "frame": [a.height, a.width],
                      "hip_images_per_s": round(a.batch / hip, 1), "eager_fp16_images_per_s": round(a.batch / eag, 1),
                      "hip_batch_s": [round(t, 4) for t in hip_s], "eager_batch_s": [round(t, 4) for t in eager_s],
                      "useful_tflops": round(useful_flops(cfg) * a.batch / hip / 1e12, 1),
                      "max_diff_of_normalised_embeddings": diff,
                      "bracketed_batch_s": round(whole, 4), "clip_entries_s": {k: round(v, 5) for k, v in spent.items()},
                      "clip_entries_share": round(sum(spent.values()) / whole, 4)}))


if __name__ == "__main__":
    main()
