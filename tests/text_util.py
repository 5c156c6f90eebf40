"""Helpers of test_text_prompts_cpu.py / test_gpu_text_encoder.py: the golden of tests/golden/make_goldens_text.py, a float64 restatement of
HF's CLIPTextModel (written from the published arithmetic: token + position embedding, pre-LN blocks with causally masked softmax
attention, exact-form or quick GELU, final LayerNorm, the row at argmax / at the first end token as the pooled output), a second run of
it that rounds to fp16 wherever scaledreamer_amd.diffusion.text_hip stores an fp16 tensor, a model directory writer and a stub tokenizer.
Nothing here imports transformers."""
import json
import math
import os
import zlib

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "text_encoder_small.npz")
_cache = {}


def golden():
    """dict(config, sd {HF key without prefix: fp16 tensor}, input_ids int64 [4, 77], last_hidden_state / pooler_output fp32, hashes)"""
    if not _cache:
        g = np.load(GOLDEN)
        _cache.update(config=json.loads(str(g["config_json"])), sd={k[2:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("w.")},
                      input_ids=torch.from_numpy(g["input_ids"]), last_hidden_state=torch.from_numpy(g["last_hidden_state"]),
                      pooler_output=torch.from_numpy(g["pooler_output"]),
                      hashes=[(str(m), str(p), str(t), str(n)) for m, p, t, n in zip(g["hash_model"], g["hash_prompt"], g["hash_type"], g["hash_name"])])
    return _cache


def _ln(x, w, b, eps):
    m = x.mean(-1, keepdim=True)
    v = ((x - m) ** 2).mean(-1, keepdim=True)
    return (x - m) / torch.sqrt(v + eps) * w + b


def gelu64(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def quick_gelu64(x):
    return x * torch.sigmoid(1.702 * x)


def r16(t):
    return t.to(torch.float16).double()


def pool_positions(ids, eos_token_id):
    """HF's rule: argmax of the ids when eos_token_id == 2 (legacy), else the first position holding eos_token_id"""
    return ids.argmax(-1) if eos_token_id == 2 else (ids == eos_token_id).int().argmax(-1)


def tower_ref64(sd, cfg, ids, fp16_stores=False):
    """input_ids int64 [P, L] -> (last_hidden_state float64 [P, L, C], pooled float64 [P, C]).
    fp16_stores: round to fp16 at every tensor the HIP schedule stores in fp16 (the embedding sum, every LayerNorm, the fused qkv, the
    attention output, both residual sums, fc1 and GELU outputs); the sums themselves and the softmax stay exact."""
    r = r16 if fp16_stores else (lambda t: t)
    w = {(k[len("text_model."):] if k.startswith("text_model.") else k): v.double() for k, v in sd.items()}
    heads, eps, act = cfg["num_attention_heads"], cfg.get("layer_norm_eps", 1e-5), cfg.get("hidden_act", "quick_gelu")
    act_fn = gelu64 if act == "gelu" else quick_gelu64
    n, T = ids.shape
    x = r(w["embeddings.token_embedding.weight"][ids] + w["embeddings.position_embedding.weight"][:T])
    C_ = x.shape[-1]
    hd = C_ // heads
    mask = torch.full((T, T), -math.inf, dtype=torch.float64).triu(1)
    split = lambda t: t.view(n, T, heads, hd).transpose(1, 2)
    for i in range(cfg["num_hidden_layers"]):
        p = f"encoder.layers.{i}."
        lin = lambda t, nm: t @ w[p + nm + ".weight"].t() + w[p + nm + ".bias"]
        h = r(_ln(x, w[p + "layer_norm1.weight"], w[p + "layer_norm1.bias"], eps))
        q, k, v = (split(r(lin(h, f"self_attn.{s}_proj"))) for s in "qkv")
        a = torch.softmax(q @ k.transpose(-1, -2) * hd ** -0.5 + mask, -1) @ v
        a = r(a.transpose(1, 2).reshape(n, T, C_))
        x = r(lin(a, "self_attn.out_proj") + x)
        h = r(_ln(x, w[p + "layer_norm2.weight"], w[p + "layer_norm2.bias"], eps))
        f = r(act_fn(r(lin(h, "mlp.fc1"))))
        x = r(lin(f, "mlp.fc2") + x)
    x = r(_ln(x, w["final_layer_norm.weight"], w["final_layer_norm.bias"], eps))
    return x, x[torch.arange(n), pool_positions(ids, cfg.get("eos_token_id", 2))]


def write_model_dir(root, sd, cfg, prefix="text_model."):
    """<root>/text_encoder/{config.json, pytorch_model.bin} with the published checkpoints' key prefix (or none)"""
    d = os.path.join(str(root), "text_encoder")
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, "config.json"), "w") as f:
        json.dump(cfg, f)
    torch.save({prefix + k: v.clone() for k, v in sd.items()}, os.path.join(d, "pytorch_model.bin"))
    return str(root)


def stub_tokenizer(vocab, length=77, log=None):
    """tokenize(list of str) -> int64 [n, length]: begin token vocab - 2, one seeded word per character (ids 3 .. vocab - 3), the end token
    vocab - 1 (the highest id), zeros after it; distinct strings give distinct rows.  log (a list) receives every string it is given."""

    def tokenize(prompts):
        rows = []
        for s in prompts:
            if log is not None:
                log.append(s)
            words = [3 + zlib.crc32(f"{i}:{s[:i + 1]}".encode()) % (vocab - 5) for i in range(min(len(s), length - 2))]
            rows.append([vocab - 2] + words + [vocab - 1] + [0] * (length - 2 - len(words)))
        return torch.tensor(rows, dtype=torch.long)

    return tokenize
