"""Helpers of test_clip_cpu.py / test_gpu_clip.py: float64 restatements of HF CLIP's two towers (written from the published arithmetic:
pre-LN transformer blocks, quick-GELU, class token + learned positions, pre / post LayerNorm, projection without bias), a second run of the
vision tower that rounds to fp16 wherever scaledreamer_amd.clip_eval stores an fp16 tensor, a numpy application of the resize tables and a
float64 scorer.  Nothing here imports transformers or reads a file."""
import math

import numpy as np
import torch

CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)

TINY_VISION = dict(hidden_size=128, intermediate_size=512, num_hidden_layers=2, num_attention_heads=2, image_size=42, patch_size=14,
                   projection_dim=64, layer_norm_eps=1e-5, hidden_act="quick_gelu")
TINY_TEXT = dict(vocab_size=100, hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=4, max_position_embeddings=77,
                 projection_dim=64, layer_norm_eps=1e-5, hidden_act="quick_gelu")


def _ln(x, w, b, eps):
    m = x.mean(-1, keepdim=True)
    v = ((x - m) ** 2).mean(-1, keepdim=True)
    return (x - m) / torch.sqrt(v + eps) * w + b


def quick_gelu64(x):
    return x * torch.sigmoid(1.702 * x)


def r16(t):
    """round to fp16 and come back to float64"""
    return t.to(torch.float16).double()


def random_vision_state(cfg, seed, scale=1.0):
    """HF's keys with seeded values; LayerNorm weights around 1, everything else at a size that keeps activations O(1)"""
    g = torch.Generator().manual_seed(seed)
    C_, I, D, P = cfg["hidden_size"], cfg["intermediate_size"], cfg["projection_dim"], cfg["patch_size"]
    L = (cfg["image_size"] // P) ** 2 + 1
    rn = lambda *s, std=1.0: torch.randn(*s, generator=g, dtype=torch.float64) * std * scale
    sd = {"vision_model.embeddings.class_embedding": rn(C_, std=0.5),
          "vision_model.embeddings.patch_embedding.weight": rn(C_, 3, P, P, std=(3 * P * P) ** -0.5),
          "vision_model.embeddings.position_embedding.weight": rn(L, C_, std=0.5),
          "visual_projection.weight": rn(D, C_, std=C_ ** -0.5)}
    for n in ("vision_model.pre_layrnorm", "vision_model.post_layernorm"):
        sd[n + ".weight"], sd[n + ".bias"] = 1.0 + rn(C_, std=0.1), rn(C_, std=0.1)
    for i in range(cfg["num_hidden_layers"]):
        p = f"vision_model.encoder.layers.{i}."
        for n in ("layer_norm1", "layer_norm2"):
            sd[p + n + ".weight"], sd[p + n + ".bias"] = 1.0 + rn(C_, std=0.1), rn(C_, std=0.1)
        for n in ("q_proj", "k_proj", "v_proj", "out_proj"):
            sd[p + f"self_attn.{n}.weight"], sd[p + f"self_attn.{n}.bias"] = rn(C_, C_, std=C_ ** -0.5), rn(C_, std=0.1)
        sd[p + "mlp.fc1.weight"], sd[p + "mlp.fc1.bias"] = rn(I, C_, std=C_ ** -0.5), rn(I, std=0.1)
        sd[p + "mlp.fc2.weight"], sd[p + "mlp.fc2.bias"] = rn(C_, I, std=I ** -0.5), rn(C_, std=0.1)
    return sd


def random_text_state(cfg, seed):
    g = torch.Generator().manual_seed(seed)
    C_, I, D = cfg["hidden_size"], cfg["intermediate_size"], cfg["projection_dim"]
    rn = lambda *s, std=1.0: torch.randn(*s, generator=g, dtype=torch.float64) * std
    sd = {"text_model.embeddings.token_embedding.weight": rn(cfg["vocab_size"], C_, std=0.5),
          "text_model.embeddings.position_embedding.weight": rn(cfg["max_position_embeddings"], C_, std=0.5),
          "text_model.final_layer_norm.weight": 1.0 + rn(C_, std=0.1), "text_model.final_layer_norm.bias": rn(C_, std=0.1),
          "text_projection.weight": rn(D, C_, std=C_ ** -0.5)}
    for i in range(cfg["num_hidden_layers"]):
        p = f"text_model.encoder.layers.{i}."
        for n in ("layer_norm1", "layer_norm2"):
            sd[p + n + ".weight"], sd[p + n + ".bias"] = 1.0 + rn(C_, std=0.1), rn(C_, std=0.1)
        for n in ("q_proj", "k_proj", "v_proj", "out_proj"):
            sd[p + f"self_attn.{n}.weight"], sd[p + f"self_attn.{n}.bias"] = rn(C_, C_, std=C_ ** -0.5), rn(C_, std=0.1)
        sd[p + "mlp.fc1.weight"], sd[p + "mlp.fc1.bias"] = rn(I, C_, std=C_ ** -0.5), rn(I, std=0.1)
        sd[p + "mlp.fc2.weight"], sd[p + "mlp.fc2.bias"] = rn(C_, I, std=I ** -0.5), rn(C_, std=0.1)
    return sd


def _heads(t, heads):
    n, T, C_ = t.shape
    return t.view(n, T, heads, C_ // heads).transpose(1, 2)


def vision_ref64(sd, cfg, pixels, fp16_stores=False):
    """pixels float64 [B, 3, S, S] (already normalised) -> image_embeds float64 [B, D], not normalised.
    fp16_stores: round to fp16 at every tensor the HIP schedule stores in fp16 (patch rows, patch GEMM output, tokens, every LayerNorm,
    q, k, V^T without its bias, the attention output, both residual sums, fc1 and quick-GELU outputs, the folded out-projection bias);
    the sums themselves and the softmax stay exact."""
    r = r16 if fp16_stores else (lambda t: t)
    w = {k: v.double() for k, v in sd.items()}
    C_, heads, P, eps = cfg["hidden_size"], cfg["num_attention_heads"], cfg["patch_size"], cfg["layer_norm_eps"]
    B, _, S, _ = pixels.shape
    g = S // P
    # patch rows: row (b, py, px), column (c, dy, dx)
    rows = r(pixels.double()).view(B, 3, g, P, g, P).permute(0, 2, 4, 1, 3, 5).reshape(B, g * g, 3 * P * P)
    e = "vision_model.embeddings."
    pe = r(rows @ w[e + "patch_embedding.weight"].reshape(C_, -1).t())
    x = torch.cat([w[e + "class_embedding"].expand(B, 1, C_), pe], 1) + w[e + "position_embedding.weight"]
    x = r(_ln(x, w["vision_model.pre_layrnorm.weight"], w["vision_model.pre_layrnorm.bias"], eps))
    for i in range(cfg["num_hidden_layers"]):
        p = f"vision_model.encoder.layers.{i}."
        lin = lambda t, n: t @ w[p + n + ".weight"].t() + w[p + n + ".bias"]
        h = r(_ln(x, w[p + "layer_norm1.weight"], w[p + "layer_norm1.bias"], eps))
        q, k = r(lin(h, "self_attn.q_proj")), r(lin(h, "self_attn.k_proj"))
        if fp16_stores:
            v = r(h @ w[p + "self_attn.v_proj.weight"].t())
            b_o = r(w[p + "self_attn.out_proj.bias"] + w[p + "self_attn.out_proj.weight"] @ w[p + "self_attn.v_proj.bias"])
        else:
            v, b_o = lin(h, "self_attn.v_proj"), w[p + "self_attn.out_proj.bias"]
        q, k, v = _heads(q, heads), _heads(k, heads), _heads(v, heads)
        a = torch.softmax(q @ k.transpose(-1, -2) * (C_ // heads) ** -0.5, -1) @ v
        a = r(a.transpose(1, 2).reshape(B, -1, C_))
        x = r(a @ w[p + "self_attn.out_proj.weight"].t() + b_o + x)
        h = r(_ln(x, w[p + "layer_norm2.weight"], w[p + "layer_norm2.bias"], eps))
        f = r(quick_gelu64(r(lin(h, "mlp.fc1"))))
        x = r(lin(f, "mlp.fc2") + x)
    cls = r(_ln(x[:, 0], w["vision_model.post_layernorm.weight"], w["vision_model.post_layernorm.bias"], eps))
    return cls @ w["visual_projection.weight"].t()


def text_ref64(sd, cfg, ids):
    """input_ids int64 [P, T] -> text_embeds float64 [P, D], not normalised (pooled at the first highest id: the end-of-text token)"""
    w = {k: v.double() for k, v in sd.items()}
    heads, eps = cfg["num_attention_heads"], cfg["layer_norm_eps"]
    n, T = ids.shape
    x = w["text_model.embeddings.token_embedding.weight"][ids] + w["text_model.embeddings.position_embedding.weight"][:T]
    C_ = x.shape[-1]
    mask = torch.full((T, T), -math.inf, dtype=torch.float64).triu(1)
    for i in range(cfg["num_hidden_layers"]):
        p = f"text_model.encoder.layers.{i}."
        lin = lambda t, nm: t @ w[p + nm + ".weight"].t() + w[p + nm + ".bias"]
        h = _ln(x, w[p + "layer_norm1.weight"], w[p + "layer_norm1.bias"], eps)
        q, k, v = (_heads(lin(h, f"self_attn.{s}_proj"), heads) for s in "qkv")
        a = torch.softmax(q @ k.transpose(-1, -2) * (C_ // heads) ** -0.5 + mask, -1) @ v
        x = x + lin(a.transpose(1, 2).reshape(n, T, C_), "self_attn.out_proj")
        h = lin(_ln(x, w[p + "layer_norm2.weight"], w[p + "layer_norm2.bias"], eps), "mlp.fc1")
        x = x + lin(quick_gelu64(h), "mlp.fc2")
    x = _ln(x, w["text_model.final_layer_norm.weight"], w["text_model.final_layer_norm.bias"], eps)
    return x[torch.arange(n), ids.argmax(-1)] @ w["text_projection.weight"].t()


def text_ids(cfg, eos_positions, seed):
    """rows of random tokens with the end-of-text token (the highest id) at the given positions and, as CLIP's tokenizer pads, after them"""
    g = torch.Generator().manual_seed(seed)
    eos, T = cfg["vocab_size"] - 1, cfg["max_position_embeddings"]
    ids = torch.randint(0, eos - 1, (len(eos_positions), T), generator=g)
    ids[:, 0] = eos - 1                                       # begin-of-text
    for r, p in enumerate(eos_positions):
        ids[r, p:] = eos
    return ids


def normalise_u8(u8):
    """uint8 [B, S, S, 3] -> fp32 [B, 3, S, S]: (u8 / 255 - mean) / std, every step in fp32"""
    x = torch.as_tensor(u8).to(torch.float32) / np.float32(255.0)
    x = (x - torch.tensor(CLIP_MEAN, dtype=torch.float32)) / torch.tensor(CLIP_STD, dtype=torch.float32)
    return x.permute(0, 3, 1, 2).contiguous()


def patch_rows(x, P):
    """[B, 3, S, S] -> [B g^2, 3 P^2]: row (b, py, px), column (c, dy, dx)"""
    B, _, S, _ = x.shape
    g = S // P
    return x.view(B, 3, g, P, g, P).permute(0, 2, 4, 1, 3, 5).reshape(B * g * g, 3 * P * P)


def _pass(img, bounds, kk):
    """one resize pass along axis 0 of img uint8 [n_in, ...] in int32"""
    out = np.empty((bounds.shape[0],) + img.shape[1:], np.uint8)
    src = img.astype(np.int32)
    for xx, (xmin, n) in enumerate(bounds):
        k = kk[xx, :n].astype(np.int32).reshape((n,) + (1,) * (img.ndim - 1))
        acc = (1 << 21) + (src[xmin:xmin + n] * k).sum(0, dtype=np.int32)
        out[xx] = np.clip(acc >> 22, 0, 255)
    return out


def apply_tables(frame, S, tables):
    """frame uint8 [H, Wfull, 3]: crop the left H x H square, horizontal pass, vertical pass (none when H == S); tables = (bounds, kk) of H -> S"""
    H = frame.shape[0]
    sq = np.ascontiguousarray(frame[:, :H])
    if H == S:
        return sq.copy()
    bounds, kk = tables
    hor = _pass(sq.transpose(1, 0, 2), bounds, kk).transpose(1, 0, 2)        # [H, S, 3]
    return _pass(hor, bounds, kk)


def pil_resize(frame, S):
    from PIL import Image

    H = frame.shape[0]
    im = Image.fromarray(frame).convert("RGB")
    return np.asarray(im.crop((0, 0, H, H)).resize((S, S), resample=Image.BILINEAR))


def random_frames(B, H, W, seed):
    """uint8 [B, H, W, 3]: noise over a smooth ramp, so both flat areas and full-range steps occur"""
    rng = np.random.default_rng(seed)
    ramp = (np.arange(W)[None, :, None] * 255 // max(W - 1, 1) + np.arange(H)[:, None, None] * 3) % 256
    x = rng.integers(0, 256, (B, H, W, 3))
    x[:, : H // 2] = (ramp[: H // 2] + x[:, : H // 2] // 8) % 256
    return x.astype(np.uint8)


def score_ref64(img, txt, own):
    """float64 (sim [B], top1 [B], margin [B]): margin = best - second best logit of each image (inf when P == 1)"""
    img, txt = img.double(), txt.double()
    n = img / img.norm(dim=-1, keepdim=True)
    logits = n @ txt.t()
    top = logits.topk(min(2, txt.shape[0]), -1).values
    margin = top[:, 0] - top[:, 1] if txt.shape[0] > 1 else torch.full((img.shape[0],), math.inf, dtype=torch.float64)
    return logits[torch.arange(img.shape[0]), own.long()], logits.argmax(-1), margin
