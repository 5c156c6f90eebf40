"""Golden vectors for the CLIP text encoder on the HIP path and the multi-prompt processor's cache names.

  python tests/golden/make_goldens_text.py     # writes tests/golden/text_encoder_small.npz  (CPU, needs `transformers`)

Runs transformers' own CLIPTextModel — the class the reference's prompt processors call
(custom/amortized/models/prompt_processors/stable_diffusion_multi_prompt_processor.py:48-70) — seeded and randomly initialised at
hidden 128 / 2 heads / 2 layers / intermediate 256 / vocab 512 / 77 positions, hidden_act "gelu", eos_token_id 2 (the legacy pooling
rule SD-2.1's text encoder takes: the row at input_ids.argmax).  The weights are rounded to fp16 BEFORE the forward pass and stored as
fp16, so the fixture's outputs are exact fp32 functions of what it stores.  Four rows of token ids put the end token (the highest id)
at positions 1 (the empty prompt), 5, 40 and 76 (no padding).  The cache file names are hash_prompt of the reference's
prompt_processors/utils.py, imported in place (ref_harness.REFERENCE), for three (model, prompt, type) triples.
"""
from __future__ import annotations

import importlib.util
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from ref_harness import REFERENCE  # noqa: E402

CONFIG = dict(vocab_size=512, hidden_size=128, intermediate_size=256, num_hidden_layers=2, num_attention_heads=2, max_position_embeddings=77,
              hidden_act="gelu", layer_norm_eps=1e-5, eos_token_id=2, bos_token_id=0, pad_token_id=1)
EOS_POSITIONS = (1, 5, 40, 76)
HASH_TRIPLES = (("pretrained/stable-diffusion-2-1-base", "a DSLR photo of an owl", "global"),
                ("pretrained/stable-diffusion-2-1-base", "a DSLR photo of an owl, back view", "local"),
                ("stabilityai/stable-diffusion-2-1-base", "", "local"))


def input_ids(seed: int = 7) -> torch.Tensor:
    """[4, 77]: begin token 510, random words below it, the end token 511 (the highest id) at EOS_POSITIONS and, as CLIP's tokenizer pads
    SD-2.1's vocabulary, zeros after it"""
    g = torch.Generator().manual_seed(seed)
    V, T = CONFIG["vocab_size"], CONFIG["max_position_embeddings"]
    ids = torch.randint(3, V - 2, (len(EOS_POSITIONS), T), generator=g)
    ids[:, 0] = V - 2
    for r, p in enumerate(EOS_POSITIONS):
        ids[r, p] = V - 1
        ids[r, p + 1:] = 0
    return ids


def main() -> None:
    from transformers import CLIPTextConfig, CLIPTextModel

    torch.manual_seed(20)
    model = CLIPTextModel(CLIPTextConfig(**CONFIG)).eval()
    g = torch.Generator().manual_seed(21)
    sd = {}
    for k, v in model.state_dict().items():
        if not v.is_floating_point():
            continue
        # HF's initialisation leaves LayerNorms at (1, 0) and biases at 0: give every tensor a seeded value so that none of them drops out
        if k.endswith("layer_norm1.weight") or k.endswith("layer_norm2.weight") or k.endswith("final_layer_norm.weight"):
            v = 1.0 + 0.1 * torch.randn(v.shape, generator=g)
        elif k.endswith(".bias"):
            v = 0.1 * torch.randn(v.shape, generator=g)
        elif "embedding" in k:
            v = 0.5 * torch.randn(v.shape, generator=g)
        else:
            v = torch.randn(v.shape, generator=g) * v.shape[1] ** -0.5
        sd[k] = v.to(torch.float16)
    missing = model.load_state_dict({k: v.float() for k, v in sd.items()}, strict=False)
    assert not missing.unexpected_keys and all("position_ids" in k for k in missing.missing_keys), missing
    ids = input_ids()
    with torch.no_grad():
        out = model(input_ids=ids)
    last, pooled = out.last_hidden_state.float(), out.pooler_output.float()
    rows = last[torch.arange(ids.shape[0]), ids.argmax(-1)]
    assert torch.equal(pooled, rows), "pooler_output is not the row at argmax"
    assert ids.argmax(-1).tolist() == list(EOS_POSITIONS)

    spec = importlib.util.spec_from_file_location("ref_prompt_utils", os.path.join(REFERENCE, "custom/amortized/models/prompt_processors/utils.py"))
    ref_utils = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref_utils)
    hashes = [ref_utils.hash_prompt(*t) for t in HASH_TRIPLES]

    arrays = {"w." + k: v.numpy() for k, v in sd.items()}
    arrays.update(input_ids=ids.numpy().astype(np.int64), last_hidden_state=last.numpy(), pooler_output=pooled.numpy(),
                  config_json=np.array(json.dumps(CONFIG)),
                  hash_model=np.array([t[0] for t in HASH_TRIPLES]), hash_prompt=np.array([t[1] for t in HASH_TRIPLES]),
                  hash_type=np.array([t[2] for t in HASH_TRIPLES]), hash_name=np.array(hashes))
    path = os.path.join(HERE, "text_encoder_small.npz")
    np.savez_compressed(path, **arrays)
    print(f"wrote {path}: {os.path.getsize(path)} bytes, {len(sd)} weight tensors, |last| max {float(last.abs().max()):.3f}")


if __name__ == "__main__":
    main()
