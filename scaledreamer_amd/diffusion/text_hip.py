"""CLIP text encoder on the HIP path: HF `CLIPTextModel` arithmetic (token + position embedding, pre-LN blocks with causal self-attention
and a GELU MLP, final LayerNorm, the end-of-text row as the pooled output) on the entries of csrc/text.hip plus asd_gemm_f16 /
asd_layernorm_f16.  It replaces the reference's one-string-per-call fp32 text encoder of the prompt processors
(custom/amortized/models/prompt_processors/stable_diffusion_multi_prompt_processor.py:58-70): strings are encoded in chunks of sequences.

Weights, activations and the residual stream are fp16; accumulation, LayerNorm statistics, scores and softmax are fp32.  q, k and v come
from ONE GEMM (N = 3C) and the attention reads the three column blocks in place.  There is no fallback: a config outside the supported
family is a NotImplementedError, a missing library an AsdError."""
from __future__ import annotations

import ctypes as C
import json
import os
from typing import Dict, Optional, Tuple

import torch

from .._lib import check, f32, i32, lib, ptr, stream
from . import hip_ops as H

MAX_L = 128


def _p(t: torch.Tensor):
    return C.c_void_p(t.data_ptr())


def embed(input_ids: torch.Tensor, token_embedding: torch.Tensor, position_embedding: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """input_ids [P, L] (any integer dtype, host or device) -> x fp16 [P L, C] = token_embedding[id] + position_embedding[t].
    An id outside [0, vocab) is a ValueError, raised here on the host (the kernel only clamps)."""
    assert input_ids.dim() == 2 and token_embedding.dtype == position_embedding.dtype == torch.float16
    Pn, L = int(input_ids.shape[0]), int(input_ids.shape[1])
    vocab, c = int(token_embedding.shape[0]), int(token_embedding.shape[1])
    assert position_embedding.shape[0] >= L and position_embedding.shape[1] == c, "position_embedding shorter than the sequence"
    host = input_ids.detach().cpu()
    if Pn and (int(host.min()) < 0 or int(host.max()) >= vocab):
        raise ValueError(f"input_ids outside [0, {vocab}): min {int(host.min())}, max {int(host.max())}")
    dev = token_embedding.device
    ids = host.to(torch.int32).contiguous().to(dev)
    if out is None:
        out = torch.empty((Pn * L, c), device=dev, dtype=torch.float16)
    assert out.dtype == torch.float16 and tuple(out.shape) == (Pn * L, c) and out.is_contiguous()
    check(lib().asd_text_embed_f16(ptr(ids), i32(Pn), i32(L), i32(vocab), i32(c), ptr(token_embedding), ptr(position_embedding), ptr(out), stream()))
    return out


def causal_attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, batch: int, heads: int, L: int, scale: Optional[float] = None,
                     out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """q, k, v: [batch L, heads 64] fp16 views with unit column stride and their own row strides (column blocks of one qkv matrix are
    fine) -> o [batch L, heads 64]; query t attends to keys 0 .. t of its sequence."""
    for t in (q, k, v):
        assert t.dtype == torch.float16 and t.dim() == 2 and t.stride(1) == 1 and tuple(t.shape) == (batch * L, heads * 64)
    if out is None:
        out = torch.empty((batch * L, heads * 64), device=q.device, dtype=torch.float16)
    assert out.dtype == torch.float16 and out.stride(1) == 1 and tuple(out.shape) == (batch * L, heads * 64)
    check(lib().asd_attention_causal_f16(_p(q), i32(q.stride(0)), _p(k), i32(k.stride(0)), _p(v), i32(v.stride(0)), _p(out), i32(out.stride(0)),
                                         i32(batch), i32(heads), i32(L), f32(64 ** -0.5 if scale is None else scale), stream()))
    return out


def gelu(x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """0.5 x (1 + erf(x / sqrt 2)), fp16; out may be x"""
    assert x.dtype == torch.float16
    if out is None:
        out = torch.empty_like(x)
    check(lib().asd_gelu_f16(ptr(x), C.c_int64(x.numel()), ptr(out), stream()))
    return out


def quick_gelu(x: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    check(lib().asd_quick_gelu_f16(ptr(x), C.c_int64(x.numel()), ptr(out), stream()))
    return out


def layernorm(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float, out: torch.Tensor) -> torch.Tensor:
    check(lib().asd_layernorm_f16(ptr(x), i32(x.shape[0]), i32(x.shape[1]), ptr(gamma), ptr(beta), f32(eps), ptr(out), stream()))
    return out


gemm = H.gemm           # the schedule below calls the module-level names, so a tool can bracket each kind of call (tools/bench_text_encoder.py)


class HipClipTextEncoder:
    """CLIPTextModel on the HIP path: input_ids [P, L] -> (last_hidden_state fp16 [P, L, C], pooled fp32 [P, C]).  state_dict holds HF's
    keys, with or without the `text_model.` prefix; weights are cast to fp16 and q / k / v are concatenated once, here."""

    SUPPORTED = ("CLIP text tower with head dim 64, hidden_act gelu or quick_gelu, hidden size a multiple of 8 and max_position_embeddings <= 128 "
                 "(SD-1.x ViT-L/14 text, SD-2.x OpenCLIP ViT-H text)")

    def __init__(self, state_dict: Dict[str, torch.Tensor], config: dict, device="cuda", chunk: int = 256):
        c = dict(config.get("text_config", config))
        self.C, self.heads, self.layers = int(c["hidden_size"]), int(c["num_attention_heads"]), int(c["num_hidden_layers"])
        self.I, self.vocab, self.max_pos = int(c["intermediate_size"]), int(c["vocab_size"]), int(c["max_position_embeddings"])
        self.eps, self.act = float(c.get("layer_norm_eps", 1e-5)), c.get("hidden_act", "quick_gelu")
        self.eos = int(c.get("eos_token_id", 2))
        if (self.C % self.heads or self.C // self.heads != 64 or self.act not in ("gelu", "quick_gelu") or self.C % 8 or self.I % 8
                or not 1 <= self.max_pos <= MAX_L):
            raise NotImplementedError(f"text config (hidden {self.C}, heads {self.heads}, act {self.act}, intermediate {self.I}, positions "
                                      f"{self.max_pos}) is outside the supported family: {self.SUPPORTED}")
        assert chunk >= 1
        self.chunk, self.device = int(chunk), torch.device(device)
        sd = {(k[len("text_model."):] if k.startswith("text_model.") else k): v for k, v in state_dict.items()}
        g = lambda k: sd[k].detach().to(self.device, torch.float32)
        h16 = lambda t: t.to(torch.float16).contiguous()
        self.tok, self.pos = h16(g("embeddings.token_embedding.weight")), h16(g("embeddings.position_embedding.weight"))
        assert tuple(self.tok.shape) == (self.vocab, self.C) and tuple(self.pos.shape) == (self.max_pos, self.C), "embedding tables do not fit the config"
        self.final = (h16(g("final_layer_norm.weight")), h16(g("final_layer_norm.bias")))
        self.blocks = []
        for n in range(self.layers):
            p = f"encoder.layers.{n}."
            self.blocks.append(dict(
                ln1=(h16(g(p + "layer_norm1.weight")), h16(g(p + "layer_norm1.bias"))), ln2=(h16(g(p + "layer_norm2.weight")), h16(g(p + "layer_norm2.bias"))),
                w_qkv=h16(torch.cat([g(p + f"self_attn.{s}_proj.weight") for s in "qkv"])),
                b_qkv=h16(torch.cat([g(p + f"self_attn.{s}_proj.bias") for s in "qkv"])),
                w_o=h16(g(p + "self_attn.out_proj.weight")), b_o=h16(g(p + "self_attn.out_proj.bias")),
                w_fc1=h16(g(p + "mlp.fc1.weight")), b_fc1=h16(g(p + "mlp.fc1.bias")), w_fc2=h16(g(p + "mlp.fc2.weight")), b_fc2=h16(g(p + "mlp.fc2.bias"))))
        self._buf: Dict[str, torch.Tensor] = {}
        self._rows = 0

    @classmethod
    def from_pretrained(cls, model_dir: str, device="cuda", chunk: int = 256) -> "HipClipTextEncoder":
        """<model_dir>/text_encoder/config.json and model.safetensors or pytorch_model.bin (a diffusers pipeline directory); nothing is downloaded"""
        from .checkpoint import _first_existing, _read_state_dict

        d = os.path.join(model_dir, "text_encoder")
        path = _first_existing(os.path.join(d, "model.safetensors"), os.path.join(d, "pytorch_model.bin"))
        if path is None or not os.path.isfile(os.path.join(d, "config.json")):
            raise FileNotFoundError(f"{d}: needs config.json and model.safetensors or pytorch_model.bin")
        with open(os.path.join(d, "config.json")) as f:
            config = json.load(f)
        return cls(_read_state_dict(path), config, device, chunk)

    def _buffers(self, rows: int) -> Dict[str, torch.Tensor]:
        """activation buffers for up to `rows` token rows, allocated once and reused by every chunk"""
        if rows > self._rows:
            mk = lambda n: torch.empty((rows, n), device=self.device, dtype=torch.float16)
            self._buf = dict(x=mk(self.C), x2=mk(self.C), h=mk(self.C), o=mk(self.C), qkv=mk(3 * self.C), f=mk(self.I))
            self._rows = rows
        return self._buf

    def release(self) -> None:
        """drop the weights and the activation buffers"""
        self._buf, self._rows, self.blocks = {}, 0, []
        self.tok = self.pos = self.final = None

    def _encode(self, ids: torch.Tensor) -> torch.Tensor:
        n, L, Cc = int(ids.shape[0]), int(ids.shape[1]), self.C
        M = n * L
        b = {k: v[:M] for k, v in self._buffers(M).items()}          # the first chunk is the largest: later ones reuse its buffers
        x, x2 = embed(ids, self.tok, self.pos, out=b["x"]), b["x2"]
        for w in self.blocks:
            h = layernorm(x, w["ln1"][0], w["ln1"][1], self.eps, out=b["h"])
            qkv = gemm(h, w["w_qkv"], bias=w["b_qkv"], out=b["qkv"])
            o = causal_attention(qkv[:, :Cc], qkv[:, Cc:2 * Cc], qkv[:, 2 * Cc:], n, self.heads, L, out=b["o"])
            gemm(o, w["w_o"], bias=w["b_o"], residual=x, out=x2)
            x, x2 = x2, x
            h = layernorm(x, w["ln2"][0], w["ln2"][1], self.eps, out=b["h"])
            f = gemm(h, w["w_fc1"], bias=w["b_fc1"], out=b["f"])
            (gelu if self.act == "gelu" else quick_gelu)(f, out=f)
            gemm(f, w["w_fc2"], bias=w["b_fc2"], residual=x, out=x2)
            x, x2 = x2, x
        return layernorm(x, self.final[0], self.final[1], self.eps, out=torch.empty_like(x)).view(n, L, Cc)

    @torch.no_grad()
    def __call__(self, input_ids) -> Tuple[torch.Tensor, torch.Tensor]:
        ids = torch.as_tensor(input_ids).detach().cpu().long()
        assert ids.dim() == 2 and 1 <= ids.shape[1] <= self.max_pos, f"input_ids must be [P, L] with 1 <= L <= {self.max_pos}"
        if not self.blocks and self.layers:
            raise RuntimeError("HipClipTextEncoder was released")
        if self.eos == 2:
            where = ids.argmax(-1)                                        # HF's legacy rule: the end-of-text token has the highest id
        else:
            where = (ids == self.eos).int().argmax(-1)                    # the first end-of-text position
        hidden = torch.cat([self._encode(ids[i:i + self.chunk]) for i in range(0, ids.shape[0], self.chunk)]) if ids.shape[0] else \
            torch.empty((0, ids.shape[1], self.C), device=self.device, dtype=torch.float16)
        pooled = hidden[torch.arange(ids.shape[0], device=self.device), where.to(self.device)].float()
        return hidden, pooled
