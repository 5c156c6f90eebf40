"""`stable-diffusion-multi-prompt-processor` without a GPU: registry, the reference's cache names and direction strings, the library split,
the eval mode, the cache written through a stub encoder, the MultiPromptUtils mapping, and the float64 restatement of the text tower
(text_util.tower_ref64) pinned to transformers' CLIPTextModel by the golden of tests/golden/make_goldens_text.py."""
import json
import os

import pytest
import torch

import text_util as T

MODEL = "pretrained/stable-diffusion-2-1-base"
LIBRARY = {"train": ["a red car", "an owl, carved from wood", "a blue chair", "a teapot", "a brass key"], "val": ["a red car", "a teapot"], "test": ["a blue chair"]}
C_ = 16


class StubEncoder:
    """(last_hidden_state [n, 77, C], pooled [n, C]) that depend on the ids only; counts its calls and the rows it has seen"""

    def __init__(self):
        self.calls, self.rows, self.released = 0, 0, 0

    def __call__(self, ids):
        self.calls += 1
        self.rows += int(ids.shape[0])
        base = ids.double()[:, :, None] * 1e-3 + torch.arange(C_, dtype=torch.float64)[None, None, :]
        hidden = torch.sin(base).to(torch.float16)                        # fp16, as the HIP encoder returns it
        return hidden, hidden[torch.arange(ids.shape[0]), ids.argmax(-1)].float()

    def release(self):
        self.released += 1


def _processor(tmp_path, enc, log=None, **over):
    import scaledreamer_amd.plugins  # noqa: F401
    from scaledreamer_amd.registry import find

    lib_dir = tmp_path / "load"
    os.makedirs(lib_dir, exist_ok=True)
    with open(lib_dir / "tiny_library.json", "w") as f:
        json.dump(LIBRARY, f)
    kw = {k: over.pop(k) for k in ("rank", "n_ranks") if k in over}
    cfg = dict(prompt_library="tiny_library", prompt_library_dir=str(lib_dir), pretrained_model_name_or_path=MODEL, cache_dir=str(tmp_path / "cache"),
               negative_prompt="ugly, blurry", **over)
    return find("stable-diffusion-multi-prompt-processor")(cfg, tokenize_fn=T.stub_tokenizer(512, log=log), encoder_factory=lambda: enc,
                                                           rank=kw.get("rank", 0), n_ranks=kw.get("n_ranks", 1))


def test_registry_resolves_the_name_the_amortized_presets_use():
    import scaledreamer_amd.plugins  # noqa: F401
    from scaledreamer_amd import presets
    from scaledreamer_amd.multiprompt_processors import StableDiffusionMultiPromptProcessor
    from scaledreamer_amd.registry import find

    assert find("stable-diffusion-multi-prompt-processor") is StableDiffusionMultiPromptProcessor
    assert find(presets.asd_sd_hyper_ingp(["x"])["system"]["prompt_processor_type"]) is StableDiffusionMultiPromptProcessor


def test_config_has_the_reference_fields_and_defaults():
    from scaledreamer_amd.multiprompt_processors import StableDiffusionMultiPromptProcessor as P

    c = P.Config()
    want = dict(prompt_library="magic3d_prompt_library", prompt_library_dir="load", prompt_library_format="json", eval_prompt=None, eval_prompt_target=None,
                pretrained_model_name_or_path="runwayml/stable-diffusion-v1-5", negative_prompt="", overhead_threshold=60.0, front_threshold=45.0,
                back_threshold=45.0, view_dependent_prompt_front=False, use_cache=True, spawn=False, cache_dir=".threestudio_cache/text_embeddings",
                use_perp_neg=False, perp_neg_f_sb=(1, 0.5, -0.606), perp_neg_f_fsb=(1, 0.5, +0.967), perp_neg_f_fs=(4, 0.5, -2.426),
                perp_neg_f_sf=(4, 0.5, -2.426), use_prompt_debiasing=False, use_local_text_embeddings=False)
    assert {k: getattr(c, k) for k in c.__dataclass_fields__} == want


def test_cache_file_names_are_the_reference_hashes():
    from scaledreamer_amd.multiprompt_processors import hash_prompt

    hashes = T.golden()["hashes"]
    assert len(hashes) == 3 and {t for _, _, t, _ in hashes} == {"global", "local"}
    for model, prompt, type_, name in hashes:
        assert hash_prompt(model, prompt, type_) == name


def test_direction_strings_in_both_forms():
    from scaledreamer_amd.multiprompt_processors import DIRECTIONS, direction_prompts

    assert DIRECTIONS == ("side", "front", "back", "overhead")
    assert direction_prompts("an owl", False) == ["an owl, side view", "an owl, front view", "an owl, back view", "an owl, overhead view"]
    assert direction_prompts("an owl", True) == ["side view of an owl", "front view of an owl", "backside view of an owl", "overhead view of an owl"]


def test_library_split_takes_every_split_by_rank(tmp_path):
    from scaledreamer_amd.multiprompt_processors import shard

    assert shard(LIBRARY, 0, 1) == LIBRARY["train"] + LIBRARY["val"] + LIBRARY["test"]
    assert shard(LIBRARY, 0, 2) == ["a red car", "a blue chair", "a brass key", "a red car", "a blue chair"]
    assert shard(LIBRARY, 1, 2) == ["an owl, carved from wood", "a teapot", "a teapot"]
    enc = StubEncoder()
    pp = _processor(tmp_path, enc, rank=1, n_ranks=2)
    assert pp.prompt_library == ["an owl, carved from wood", "a teapot", "a teapot"]
    assert list(pp.prompts_vd) == ["an owl, carved from wood", "a teapot"]
    with pytest.raises(ValueError, match=r"Prompt \[a red car\] is not in the prompt library\."):
        pp("a red car")
    with pytest.raises(ValueError, match="not in the prompt library"):
        pp(["a teapot", "ugly, blurry"])                                   # the negative prompt has embeddings but is no library prompt


def test_eval_prompt_mode_needs_no_library_file(tmp_path):
    import scaledreamer_amd.plugins  # noqa: F401
    from scaledreamer_amd.registry import find

    enc = StubEncoder()
    mk = lambda **kw: find("stable-diffusion-multi-prompt-processor")(
        dict(prompt_library_dir=str(tmp_path / "nowhere"), cache_dir=str(tmp_path / "cache"), view_dependent_prompt_front=True, **kw),
        tokenize_fn=T.stub_tokenizer(512), encoder_factory=lambda: enc)
    pp = mk(eval_prompt="a fox")
    assert pp.prompt_library == ["a fox"] and pp.prompts_vd["a fox"][2] == "backside view of a fox"
    pp = mk(eval_prompt="a fox", eval_prompt_target="a hare")
    assert pp.prompt_library == ["a fox", "a hare"]
    assert torch.equal(pp("a hare").get_global_text_embeddings(), pp.global_text_embeddings["a hare"][None])
    with pytest.raises(NotImplementedError):
        mk(eval_prompt="a fox", use_prompt_debiasing=True)


def test_stub_encoder_fills_the_cache_once(tmp_path):
    """5 distinct library prompts + 20 view-dependent strings + the negative prompt = 26 strings (the directions leave the negative prompt as
    it is, base.py:210-212), so 52 files: one CPU fp32 tensor each, [C] under the global name and [77, C] under the local one"""
    from scaledreamer_amd.multiprompt_processors import hash_prompt

    enc, log = StubEncoder(), []
    pp = _processor(tmp_path, enc, log)
    strings = pp.all_strings()
    assert len(strings) == 26 and strings[:8] == LIBRARY["train"] + ["ugly, blurry", "a red car, side view", "a red car, front view"]
    assert sorted(log) == sorted(strings) and enc.rows == 26 and enc.calls == pp.encode_calls == 1 and enc.released == 1
    cache = tmp_path / "cache"
    assert len(os.listdir(cache)) == 52
    tok = T.stub_tokenizer(512)
    for s in strings:
        g = torch.load(cache / f"{hash_prompt(MODEL, s, 'global')}.pt")
        l = torch.load(cache / f"{hash_prompt(MODEL, s, 'local')}.pt")
        assert g.dtype == l.dtype == torch.float32 and g.device.type == l.device.type == "cpu" and tuple(g.shape) == (C_,) and tuple(l.shape) == (77, C_)
        assert g.untyped_storage().nbytes() == C_ * 4 and l.untyped_storage().nbytes() == 77 * C_ * 4      # no batch-sized storage behind a row
        hidden, pooled = StubEncoder()(tok([s]))
        assert torch.equal(l, hidden[0].float()) and torch.equal(g, pooled[0])
    # a second configure finds every file and encodes nothing
    enc2, log2 = StubEncoder(), []
    pp2 = _processor(tmp_path, enc2, log2)
    assert enc2.calls == 0 and pp2.encode_calls == 0 and log2 == []
    assert all(torch.equal(pp2.local_text_embeddings[p], pp.local_text_embeddings[p]) for p in LIBRARY["train"])
    # one file removed: that string alone is encoded again; use_cache = False encodes everything
    os.remove(cache / f"{hash_prompt(MODEL, 'a teapot, back view', 'local')}.pt")
    enc3, log3 = StubEncoder(), []
    _processor(tmp_path, enc3, log3)
    assert log3 == ["a teapot, back view"] and enc3.calls == 1
    enc4 = StubEncoder()
    _processor(tmp_path, enc4, use_cache=False)
    assert enc4.rows == 26


def test_multi_prompt_utils_mapping(tmp_path):
    """base.py:391-406: per prompt the global, the local and the four view-dependent local embeddings; uncond from the negative prompt"""
    from scaledreamer_amd.multiprompt import MultiPromptUtils
    from scaledreamer_amd.multiprompt_processors import hash_prompt

    pp = _processor(tmp_path, StubEncoder(), use_perp_neg=True, front_threshold=30.0, back_threshold=20.0, overhead_threshold=50.0,
                    use_local_text_embeddings=False, perp_neg_f_sb=(2, 0.25, -0.5))
    cache = tmp_path / "cache"
    load = lambda s, t: torch.load(cache / f"{hash_prompt(MODEL, s, t)}.pt")
    batch = ["a teapot", "a red car", "a teapot"]
    pu = pp(batch)
    assert isinstance(pu, MultiPromptUtils)
    for i, p in enumerate(batch):
        assert torch.equal(pu.global_text_embeddings[i].cpu(), load(p, "global")) and torch.equal(pu.local_text_embeddings[i].cpu(), load(p, "local"))
        assert torch.equal(pu.text_embeddings_vd[i].cpu(), torch.stack([load(f"{p}, {d} view", "local") for d in ("side", "front", "back", "overhead")]))
    assert torch.equal(pu.uncond_text_embeddings.cpu(), load("ugly, blurry", "local"))
    assert torch.equal(pu.uncond_text_embeddings_vd.cpu(), torch.stack([load("ugly, blurry", "local")] * 4))
    assert tuple(torch.stack(pu.text_embeddings_vd).shape) == (3, 4, 77, C_) and tuple(pu.uncond_text_embeddings_vd.shape) == (4, 77, C_)
    assert (pu.use_perp_neg, pu.front_threshold, pu.back_threshold, pu.overhead_threshold) == (True, 30.0, 20.0, 50.0)
    assert pu.perp_neg_f_sb == (2, 0.25, -0.5) and pu.perp_neg_f_fsb == (1, 0.5, 0.967) and pu.perp_neg_f_fs == pu.perp_neg_f_sf == (4, 0.5, -2.426)
    assert not pu.use_local_text_embeddings and tuple(pu.get_global_text_embeddings().shape) == (3, C_)
    assert tuple(pp("a teapot").get_global_text_embeddings().shape) == (1, C_)                # a plain string is a batch of one
    el, az = torch.tensor([0.0, 0.0, 70.0]), torch.tensor([0.0, 90.0, 0.0])
    assert tuple(pu.get_text_embeddings(el, az, torch.ones(3)).shape) == (6, 77, C_)
    pp_local = _processor(tmp_path, StubEncoder(), use_local_text_embeddings=True)
    assert tuple(pp_local(batch).get_global_text_embeddings().shape) == (3, 77, C_)


def test_default_tokenizer_failure_names_what_is_missing(tmp_path, monkeypatch):
    """without `transformers` the default tokenizer is an AsdError that says so"""
    import sys

    from scaledreamer_amd._lib import AsdError
    from scaledreamer_amd.multiprompt_processors import local_tokenizer

    monkeypatch.setitem(sys.modules, "transformers", None)               # makes `import transformers` an ImportError
    with pytest.raises(AsdError, match="transformers"):
        local_tokenizer(str(tmp_path))(["a fox"])


def test_restatement_reproduces_the_golden():
    """text_util.tower_ref64 against transformers' CLIPTextModel to 1e-5 absolute: the restatement is in float64, the golden in fp32 over
    values of a few units, so what is left is the golden's own fp32 rounding"""
    g = T.golden()
    cfg, ids = g["config"], g["input_ids"]
    assert tuple(ids.shape) == (4, 77) and ids.argmax(-1).tolist() == [1, 5, 40, 76] and cfg["hidden_act"] == "gelu" and cfg["eos_token_id"] == 2
    assert all(v.dtype == torch.float16 for v in g["sd"].values())
    last, pooled = T.tower_ref64(g["sd"], cfg, ids)
    e_last = float((last - g["last_hidden_state"].double()).abs().max())
    e_pool = float((pooled - g["pooler_output"].double()).abs().max())
    print(f"restatement vs golden: last_hidden_state {e_last:.2e}, pooler_output {e_pool:.2e}")
    assert e_last <= 1e-5 and e_pool <= 1e-5
    assert torch.equal(g["pooler_output"], g["last_hidden_state"][torch.arange(4), ids.argmax(-1)])
    # the other pooling rule and the other activation are restated too
    assert T.pool_positions(torch.tensor([[5, 9, 7, 9]]), 9).tolist() == [1] and T.pool_positions(torch.tensor([[5, 9, 7, 9]]), 2).tolist() == [1]
    assert T.pool_positions(torch.tensor([[5, 7, 9, 3]]), 7).tolist() == [1]


def test_encoder_rejects_configs_outside_the_family():
    from scaledreamer_amd.diffusion.text_hip import HipClipTextEncoder

    cfg = T.golden()["config"]
    for bad in (dict(num_attention_heads=4), dict(hidden_act="gelu_new"), dict(max_position_embeddings=129), dict(hidden_size=192, num_attention_heads=3, intermediate_size=12)):
        with pytest.raises(NotImplementedError, match="supported family"):
            HipClipTextEncoder({}, dict(cfg, **bad), device="cpu")


def test_single_prompt_processor_still_raises_without_cache_or_weights(tmp_path):
    import scaledreamer_amd.plugins  # noqa: F401
    from scaledreamer_amd.registry import find

    cfg = dict(prompt="never cached", pretrained_model_name_or_path=str(tmp_path / "no-such-model"))
    with pytest.raises(FileNotFoundError, match="not found"):
        find("stable-diffusion-prompt-processor")(cfg, cache_dir=str(tmp_path / "cache"))
    assert not os.path.exists(tmp_path / "cache") or not os.listdir(tmp_path / "cache")
