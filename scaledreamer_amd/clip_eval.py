"""CLIP similarity and recall@1 of test renders: the scoring stage of the amortized workflow (train -> `test()` renders
`it<N>-test/<prompt>/<index>.png` -> score), what the reference does with evaluation/CLIP/evaluation_amortized.py.

The image tower is HF's `CLIPVisionModelWithProjection` arithmetic on the HIP entries: the front end, the token assembly, quick-GELU and the
scoring are csrc/clip.hip, everything between them is asd_gemm_f16 / asd_layernorm_f16 / asd_attention_f16.  Activations and weights are
fp16, accumulation and statistics fp32, the projected embedding and the scoring fp32.  There is no fallback: a config outside the
supported family is a NotImplementedError, a missing library an AsdError.

Layout of the token matrix: [B, Lpad, C] with L = (S/P)^2 + 1 tokens per image and Lpad = L rounded up to 8 (ViT-L/14: 257 -> 264), the
key stride asd_attention_f16 asks for.  That entry has no query stride, so the queries run over all Lpad rows; the padding rows start as
zeros, stay finite (LayerNorm of a constant row is beta), are masked as keys (lk = L) and are never read as results.

V^T comes out of the GEMM directly (C^T form: V^T = W_v X^T, the weight as the A operand); its bias is folded into the out-projection's,
b_out + W_out b_v, because the softmax rows sum to 1.

The text tower runs once per evaluation over P x 77 tokens, as fp32 tensor ops on the device (the project's stance on text encoders, see
prompt_processors.py): it is off the per-image path.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import math
import os
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch
import torch.nn.functional as F

from ._lib import AsdError, check, f32, i32, lib, ptr, stream

PRECISION_BITS = 22
IMAGE_SUFFIXES = (".png", ".jpg", ".jpeg", ".bmp")


# ---- host tables of the resize ---------------------------------------------------------------------------------------------------------
def resize_tables(n_in: int, n_out: int) -> Tuple[np.ndarray, np.ndarray]:
    """PIL's bilinear coefficients of one pass n_in -> n_out on 8-bit data: bounds int32 [n_out, 2] = (first input index, tap count) and
    kk int32 [n_out, ksize], the taps in 22-bit fixed point (unused entries 0).  A pass is clip8((2^21 + sum in[xmin + x] kk[x]) >> 22)."""
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = 1.0 * fs
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((n_out, 2), np.int32)
    kk = np.zeros((n_out, ksize), np.int32)
    for xx in range(n_out):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), n_in)
        n = xmax - xmin
        w = np.maximum(0.0, 1.0 - np.abs((np.arange(n) + xmin - center + 0.5) / fs))
        ww = float(w.sum())
        if ww != 0.0:
            w = w / ww
        bounds[xx] = (xmin, n)
        kk[xx, :n] = (w * (1 << PRECISION_BITS) + 0.5).astype(np.int64)       # taps are >= 0: (int)(0.5 + w 2^22) truncates
    return bounds, kk


_tables: Dict[tuple, tuple] = {}


def _device_tables(n_in: int, n_out: int, device):
    key = (n_in, n_out, str(device))
    if key not in _tables:
        b, k = resize_tables(n_in, n_out)
        _tables[key] = (torch.from_numpy(b).to(device), torch.from_numpy(k).to(device))
    return _tables[key]


# ---- the HIP entries -------------------------------------------------------------------------------------------------------------------
def patch_kpad(patch: int) -> int:
    """columns of a patch row: 3 P^2 rounded up to the 8 asd_gemm_f16 needs of K"""
    return (3 * patch * patch + 7) // 8 * 8


def preprocess(frames: torch.Tensor, size: int, patch: int, want_resized: bool = False, out: Optional[torch.Tensor] = None):
    """frames uint8 [B, H, Wfull, 3] on the device -> patch rows fp16 [B (size/patch)^2, Kpad] (and the resized uint8 [B, size, size, 3]).
    out: a [B g^2, Kpad] fp16 view to write into (any row stride, unit column stride)."""
    assert frames.dtype == torch.uint8 and frames.dim() == 4 and frames.shape[-1] == 3 and frames.is_cuda and frames.is_contiguous()
    B, H, W = int(frames.shape[0]), int(frames.shape[1]), int(frames.shape[2])
    g, kpad = size // patch, patch_kpad(patch)
    if out is None:
        out = torch.empty((B * g * g, kpad), device=frames.device, dtype=torch.float16)
    assert out.dtype == torch.float16 and tuple(out.shape) == (B * g * g, kpad) and out.stride(1) == 1
    resized = torch.empty((B, size, size, 3), device=frames.device, dtype=torch.uint8) if want_resized else None
    bounds = kk = tmp = None
    ksize = 0
    if H != size and W >= H:
        bounds, kk = _device_tables(H, size, frames.device)
        ksize = int(kk.shape[1])
        tmp = torch.empty((B, H, size, 3), device=frames.device, dtype=torch.uint8)
    check(lib().asd_clip_preprocess_u8(ptr(frames), i32(B), i32(H), i32(W), i32(size), i32(patch), i32(kpad), ptr(bounds), ptr(kk), i32(ksize),
                                       ptr(tmp), ptr(resized), C.c_void_p(out.data_ptr()), i32(out.stride(0)), stream()))
    return (out, resized) if want_resized else out


def embed(patch_out: torch.Tensor, class_embedding, position_embedding, gamma, beta, eps: float, batch: int, lpad: int,
          out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """LayerNorm(cat(class, patches) + position) -> [batch, lpad, C] fp16, rows >= g2 + 1 of each image zero"""
    g2, c = patch_out.shape[0] // batch, patch_out.shape[1]
    assert patch_out.shape[0] == batch * g2 and tuple(position_embedding.shape) == (g2 + 1, c)
    if out is None:
        out = torch.empty((batch, lpad, c), device=patch_out.device, dtype=torch.float16)
    check(lib().asd_clip_embed_f16(ptr(patch_out), ptr(class_embedding), ptr(position_embedding), ptr(gamma), ptr(beta), f32(eps), i32(batch),
                                   i32(g2), i32(c), i32(lpad), ptr(out), stream()))
    return out


def quick_gelu(x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x sigmoid(1.702 x), fp16; out may be x"""
    assert x.dtype == torch.float16
    if out is None:
        out = torch.empty_like(x)
    check(lib().asd_quick_gelu_f16(ptr(x), C.c_int64(x.numel()), ptr(out), stream()))
    return out


def score(img: torch.Tensor, txt: torch.Tensor, own: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """img fp32 [B, D] (any scale), txt fp32 [P, D] (L2-normalised), own int32 [B] -> (sim fp32 [B], top1 int32 [B])"""
    assert img.dtype == torch.float32 and txt.dtype == torch.float32 and own.dtype == torch.int32 and img.shape[1] == txt.shape[1]
    B, D, P = int(img.shape[0]), int(img.shape[1]), int(txt.shape[0])
    sim = torch.empty(B, device=img.device, dtype=torch.float32)
    top1 = torch.empty(B, device=img.device, dtype=torch.int32)
    need = lib().asd_clip_score_workspace(C.c_int64(B), C.c_int64(P))
    if need < 0:
        raise AsdError(lib().asd_last_error().decode())
    ws = torch.empty(max(need, 4), device=img.device, dtype=torch.uint8)
    check(lib().asd_clip_score_f32(ptr(img), ptr(txt), ptr(own), C.c_int64(B), C.c_int64(P), i32(D), ptr(sim), ptr(top1), ptr(ws), C.c_int64(need),
                                   stream()))
    return sim, top1


# ---- towers ----------------------------------------------------------------------------------------------------------------------------
def _sub(config: dict, key: str) -> dict:
    """the vision / text part of a CLIP config.json (or the dict itself when it already is one)"""
    c = dict(config.get(key, config))
    if "projection_dim" not in c and "projection_dim" in config:
        c["projection_dim"] = config["projection_dim"]
    return c


class ClipVisionTower:
    """CLIPVisionModelWithProjection on the HIP path: frames uint8 [B, H, Wfull, 3] -> image embeddings fp32 [B, projection_dim]
    (not normalised).  state_dict holds HF's keys; weights are cast to fp16 once, here."""

    SUPPORTED = "CLIP ViT with head dim 64, hidden_act quick_gelu, hidden size a multiple of 8 and <= 2048 (ViT-B/32, B/16, L/14)"

    def __init__(self, state_dict: Dict[str, torch.Tensor], config: dict, device="cuda"):
        c = _sub(config, "vision_config")
        self.C, self.heads, self.layers = int(c["hidden_size"]), int(c["num_attention_heads"]), int(c["num_hidden_layers"])
        self.S, self.P, self.eps = int(c["image_size"]), int(c["patch_size"]), float(c.get("layer_norm_eps", 1e-5))
        act = c.get("hidden_act", "quick_gelu")
        if self.C % self.heads or self.C // self.heads != 64 or act != "quick_gelu" or self.C % 8 or self.C > 2048 or self.S % self.P:
            raise NotImplementedError(f"vision config (hidden {self.C}, heads {self.heads}, act {act}, image {self.S}, patch {self.P}) is outside the "
                                      f"supported family: {self.SUPPORTED}")
        self.g = self.S // self.P
        self.L = self.g * self.g + 1
        self.Lpad = (self.L + 7) // 8 * 8
        self.kpad = patch_kpad(self.P)
        self.device = torch.device(device)
        h16 = lambda t: t.detach().to(self.device, torch.float32).to(torch.float16).contiguous()
        sd = state_dict
        e = "vision_model.embeddings."
        wp = sd[e + "patch_embedding.weight"].detach().float().reshape(self.C, -1)
        self.w_patch = h16(F.pad(wp, (0, self.kpad - wp.shape[1])))
        self.cls, self.pos = h16(sd[e + "class_embedding"]), h16(sd[e + "position_embedding.weight"])
        assert tuple(self.pos.shape) == (self.L, self.C), "position_embedding does not fit image_size / patch_size"
        self.pre = (h16(sd["vision_model.pre_layrnorm.weight"]), h16(sd["vision_model.pre_layrnorm.bias"]))
        self.post = (h16(sd["vision_model.post_layernorm.weight"]), h16(sd["vision_model.post_layernorm.bias"]))
        self.w_proj = h16(sd["visual_projection.weight"])
        self.D = int(self.w_proj.shape[0])
        self.blocks = []
        for n in range(self.layers):
            p = f"vision_model.encoder.layers.{n}."
            g = lambda k: sd[p + k].detach().to(self.device, torch.float32)
            self.blocks.append(dict(
                ln1=(h16(g("layer_norm1.weight")), h16(g("layer_norm1.bias"))), ln2=(h16(g("layer_norm2.weight")), h16(g("layer_norm2.bias"))),
                w_qk=h16(torch.cat([g("self_attn.q_proj.weight"), g("self_attn.k_proj.weight")])),
                b_qk=h16(torch.cat([g("self_attn.q_proj.bias"), g("self_attn.k_proj.bias")])),
                w_v=h16(g("self_attn.v_proj.weight")), w_o=h16(g("self_attn.out_proj.weight")),
                b_o=h16(g("self_attn.out_proj.bias") + g("self_attn.out_proj.weight") @ g("self_attn.v_proj.bias")),
                w_fc1=h16(g("mlp.fc1.weight")), b_fc1=h16(g("mlp.fc1.bias")), w_fc2=h16(g("mlp.fc2.weight")), b_fc2=h16(g("mlp.fc2.bias"))))

    def tokens(self, frames: torch.Tensor) -> torch.Tensor:
        """the token matrix after the pre-LayerNorm: [B Lpad, C] fp16"""
        from .diffusion import hip_ops as H

        B = int(frames.shape[0])
        pe = H.gemm(preprocess(frames, self.S, self.P), self.w_patch)
        return embed(pe, self.cls, self.pos, self.pre[0], self.pre[1], self.eps, B, self.Lpad).view(B * self.Lpad, self.C)

    def __call__(self, frames: torch.Tensor) -> torch.Tensor:
        from .diffusion import hip_ops as H

        B, Cc = int(frames.shape[0]), self.C
        x = self.tokens(frames)
        for w in self.blocks:
            h = H.layernorm(x, w["ln1"][0], w["ln1"][1], self.eps)
            qk = H.gemm(h, w["w_qk"], bias=w["b_qk"])
            vT = H.gemm(w["w_v"], h)                                                    # [C, B Lpad]
            o = H.attention(qk[:, :Cc], qk[:, Cc:], vT, B, self.heads, self.Lpad, self.L, self.Lpad, scale=64 ** -0.5)
            x = H.gemm(o, w["w_o"], bias=w["b_o"], residual=x)
            h = H.layernorm(x, w["ln2"][0], w["ln2"][1], self.eps)
            f = H.gemm(h, w["w_fc1"], bias=w["b_fc1"])
            quick_gelu(f, out=f)
            x = H.gemm(f, w["w_fc2"], bias=w["b_fc2"], residual=x)
        cls = x.view(B, self.Lpad, Cc)[:, 0].contiguous()
        return H.gemm(H.layernorm(cls, self.post[0], self.post[1], self.eps), self.w_proj, out_f32=True)


class ClipTextTower:
    """CLIPTextModelWithProjection as fp32 tensor ops: token + position embedding, pre-LN blocks with a causal mask and quick-GELU,
    final_layer_norm, the row at input_ids.argmax(-1) (the end-of-text token has the highest id), text_projection, L2 normalisation."""

    def __init__(self, state_dict: Dict[str, torch.Tensor], config: dict, device="cuda", dtype=torch.float32):
        c = _sub(config, "text_config")
        self.heads, self.layers, self.eps = int(c["num_attention_heads"]), int(c["num_hidden_layers"]), float(c.get("layer_norm_eps", 1e-5))
        act = c.get("hidden_act", "quick_gelu")
        if act != "quick_gelu":
            raise NotImplementedError(f"text config with hidden_act {act}: only quick_gelu CLIP text towers are supported")
        self.device = torch.device(device)
        self.w = {k: v.detach().to(self.device, dtype) for k, v in state_dict.items() if k.startswith("text_model.") or k == "text_projection.weight"}

    def _ln(self, x, name):
        return F.layer_norm(x, x.shape[-1:], self.w[name + ".weight"], self.w[name + ".bias"], self.eps)

    def _lin(self, x, name):
        return F.linear(x, self.w[name + ".weight"], self.w[name + ".bias"])

    @torch.no_grad()
    def text_features(self, input_ids: torch.Tensor, chunk: int = 256) -> torch.Tensor:
        """input_ids int64 [P, T] -> L2-normalised features [P, D]"""
        ids = input_ids.to(self.device).long()
        return torch.cat([self._features(ids[i:i + chunk]) for i in range(0, ids.shape[0], chunk)])

    def _features(self, ids: torch.Tensor) -> torch.Tensor:
        n, T = ids.shape
        x = self.w["text_model.embeddings.token_embedding.weight"][ids] + self.w["text_model.embeddings.position_embedding.weight"][:T]
        hd = x.shape[-1] // self.heads
        mask = torch.full((T, T), float("-inf"), device=self.device, dtype=x.dtype).triu(1)
        split = lambda t: t.view(n, T, self.heads, hd).transpose(1, 2)
        for i in range(self.layers):
            p = f"text_model.encoder.layers.{i}."
            h = self._ln(x, p + "layer_norm1")
            q, k, v = (split(self._lin(h, p + f"self_attn.{s}_proj")) for s in "qkv")
            a = torch.softmax(q @ k.transpose(-1, -2) * hd ** -0.5 + mask, -1) @ v
            x = x + self._lin(a.transpose(1, 2).reshape(n, T, -1), p + "self_attn.out_proj")
            h = self._lin(self._ln(x, p + "layer_norm2"), p + "mlp.fc1")
            x = x + self._lin(h * torch.sigmoid(1.702 * h), p + "mlp.fc2")
        x = self._ln(x, "text_model.final_layer_norm")
        pooled = x[torch.arange(n, device=self.device), ids.argmax(-1)]
        f = pooled @ self.w["text_projection.weight"].t()
        return f / f.norm(dim=-1, keepdim=True)


# ---- scorer ----------------------------------------------------------------------------------------------------------------------------
def _is_image(name: str) -> bool:
    return name.lower().endswith(IMAGE_SUFFIXES)


def _frame_key(name: str):
    stem = os.path.splitext(name)[0]
    return (0, int(stem), name) if stem.isdigit() else (1, 0, name)


class ClipScorer:
    """Mean image-text similarity and recall@1 over a prompt set.  `vision` maps uint8 frames [B, H, Wfull, 3] on the device to image
    embeddings fp32 [B, D]; the text side is a ClipTextTower with a `tokenize_fn(list of str) -> input_ids [P, 77]`, or precomputed
    L2-normalised features given to set_prompts."""

    def __init__(self, vision: Callable, text: Optional[ClipTextTower] = None, tokenize_fn: Optional[Callable] = None, device="cuda"):
        self.vision, self.text, self.tokenize_fn, self.device = vision, text, tokenize_fn, torch.device(device)
        self.prompts: List[str] = []
        self.names: List[str] = []
        self.txt: Optional[torch.Tensor] = None
        self._sim: Dict[int, List[float]] = {}
        self._hit: Dict[int, List[bool]] = {}

    @classmethod
    def from_pretrained(cls, local_dir: str, tokenize_fn: Optional[Callable] = None, device="cuda") -> "ClipScorer":
        """a local directory with config.json and model.safetensors or pytorch_model.bin (HF's CLIPModel layout); nothing is downloaded"""
        with open(os.path.join(local_dir, "config.json")) as f:
            config = json.load(f)
        st, pt = os.path.join(local_dir, "model.safetensors"), os.path.join(local_dir, "pytorch_model.bin")
        if os.path.exists(st):
            from safetensors.torch import load_file

            sd = load_file(st)
        elif os.path.exists(pt):
            sd = torch.load(pt, map_location="cpu", weights_only=True)
        else:
            raise FileNotFoundError(f"{local_dir}: neither model.safetensors nor pytorch_model.bin")
        if tokenize_fn is None and os.path.exists(os.path.join(local_dir, "vocab.json")):
            tokenize_fn = _local_tokenizer(local_dir)
        return cls(ClipVisionTower(sd, config, device), ClipTextTower(sd, config, device), tokenize_fn, device)

    def set_prompts(self, prompts: Sequence[str], text_features: Optional[torch.Tensor] = None, names: Optional[Sequence[str]] = None) -> None:
        """the candidate set of recall@1; text_features [P, D] (L2-normalised) replaces the text tower; names: the keys of results()"""
        self.prompts = list(prompts)
        self.names = list(names) if names is not None else list(prompts)
        if text_features is None:
            if self.text is None or self.tokenize_fn is None:
                raise ValueError("ClipScorer needs text_features, or a text tower with a tokenize_fn")
            text_features = self.text.text_features(torch.as_tensor(self.tokenize_fn(self.prompts)))
        self.txt = text_features.to(self.device, torch.float32).contiguous()
        assert self.txt.shape[0] == len(self.prompts)
        self._sim, self._hit = {}, {}

    @torch.no_grad()
    def add(self, frames_u8: torch.Tensor, prompt_index: int) -> Tuple[List[float], List[bool]]:
        """score frames uint8 [B, H, Wfull, 3] (on the device, e.g. ops.image_grid's output) of prompt `prompt_index`"""
        assert self.txt is not None, "set_prompts first"
        emb = self.vision(frames_u8.to(self.device).contiguous())
        own = torch.full((emb.shape[0],), int(prompt_index), device=self.device, dtype=torch.int32)
        sim, top1 = score(emb.float().contiguous(), self.txt, own)
        sims, hits = sim.cpu().numpy().tolist(), (top1 == own).cpu().numpy().tolist()
        self._sim.setdefault(prompt_index, []).extend(sims)
        self._hit.setdefault(prompt_index, []).extend(hits)
        return sims, hits

    def results(self) -> Tuple[Dict[str, float], Dict[str, float]]:
        """({name: mean similarity}, {name: recall@1}) over the prompts that have images, averaged in float64 on the host"""
        names = self.names
        sim = {names[i]: sum(v) / len(v) for i, v in self._sim.items()}
        rec = {names[i]: sum(v) / len(v) for i, v in self._hit.items()}
        return sim, rec

    def evaluate_dir(self, result_dir: str, batch_size: int = 120, text_features: Optional[torch.Tensor] = None):
        """result_dir/<prompt with _ for spaces>/<index>.png, as `test()` writes it.  Every sub-directory is a recall@1 candidate; one without
        images is left out of the averages.  Writes similarity.txt and recall.txt into result_dir and returns both dicts."""
        from PIL import Image

        names = sorted(d for d in os.listdir(result_dir) if os.path.isdir(os.path.join(result_dir, d)))
        self.set_prompts([n.replace("_", " ") for n in names], text_features, names)
        for idx, name in enumerate(names):
            sub = os.path.join(result_dir, name)
            files = sorted((f for f in os.listdir(sub) if _is_image(f)), key=_frame_key)
            batch: List[np.ndarray] = []
            for f in files + [None]:
                img = None if f is None else np.asarray(Image.open(os.path.join(sub, f)).convert("RGB"))
                if batch and (img is None or len(batch) == batch_size or img.shape != batch[0].shape):
                    self.add(torch.from_numpy(np.stack(batch)).to(self.device), idx)
                    batch = []
                if img is not None:
                    batch.append(img)
        sim, rec = self.results()
        for fname, d in (("similarity.txt", sim), ("recall.txt", rec)):
            with open(os.path.join(result_dir, fname), "w") as f:
                for k, v in d.items():
                    f.write(f"{k}: {v}\n")
                f.write(f"avgerage: {sum(d.values()) / len(d) if d else float('nan')}\n")       # sic: the reference's spelling
        return sim, rec


def _local_tokenizer(local_dir: str) -> Callable:
    def tokenize(prompts):
        from transformers import CLIPTokenizer

        tok = CLIPTokenizer.from_pretrained(local_dir, local_files_only=True)
        return tok(list(prompts), padding="max_length", max_length=tok.model_max_length, truncation=True, return_tensors="pt").input_ids

    return tokenize


def main(argv=None) -> None:
    ap = argparse.ArgumentParser(description="CLIP similarity and recall@1 of a directory of test renders")
    ap.add_argument("--result_dir", type=str, required=True)
    ap.add_argument("--model_dir", type=str, required=True, help="local directory with config.json, the weights and the tokenizer files")
    ap.add_argument("--num_images", type=int, default=100, help="accepted for compatibility; every image found is scored")
    ap.add_argument("--device", type=str, default="cuda:0")
    ap.add_argument("--batch_size", type=int, default=120)
    a = ap.parse_args(argv)
    torch.cuda.set_device(torch.device(a.device))
    sim, rec = ClipScorer.from_pretrained(a.model_dir, device=a.device).evaluate_dir(a.result_dir, a.batch_size)
    print(f"Average similarity: {sum(sim.values()) / max(len(sim), 1)}")
    print(f"Average recall@1: {sum(rec.values()) / max(len(rec), 1)}")
    print("Results saved to: ", a.result_dir)


if __name__ == "__main__":
    main()
