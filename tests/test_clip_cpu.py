"""CLIP evaluation, the parts that need no GPU: the float64 restatements of clip_util against HF's models, the host tables of the resize
against PIL byte for byte, the text tower's tensor-op composition against the restatement, and evaluate_dir's walk, averaging and file
format over a stub tower."""
import os

import numpy as np
import pytest
import torch

import clip_util as U


def _hf_vision(cfg, sd):
    tr = pytest.importorskip("transformers")
    hc = tr.CLIPVisionConfig(**cfg, attn_implementation="sdpa")       # the eager form takes its softmax in fp32 whatever the model dtype
    m = tr.CLIPVisionModelWithProjection(hc).double().eval()
    missing, unexpected = m.load_state_dict(sd, strict=False)
    assert not unexpected and all("position_ids" in k for k in missing), (missing, unexpected)
    return m


def test_vision_restatement_matches_transformers():
    for cfg in (dict(U.TINY_VISION), dict(U.TINY_VISION, num_hidden_layers=1, image_size=56, num_attention_heads=4, hidden_size=64)):
        sd = U.random_vision_state(cfg, seed=3)
        m = _hf_vision(cfg, sd)
        px = torch.randn(2, 3, cfg["image_size"], cfg["image_size"], dtype=torch.float64, generator=torch.Generator().manual_seed(4))
        with torch.no_grad():
            want = m(pixel_values=px).image_embeds
        got = U.vision_ref64(sd, cfg, px)
        err = float((got - want).abs().max())
        print(f"vision restatement vs transformers: {err:.2e}")
        assert err <= 1e-12


def test_text_restatement_matches_transformers():
    tr = pytest.importorskip("transformers")
    cfg = dict(U.TINY_TEXT)
    eos = cfg["vocab_size"] - 1
    hc = tr.CLIPTextConfig(**cfg, eos_token_id=eos, bos_token_id=eos - 1, pad_token_id=eos, attn_implementation="sdpa")
    m = tr.CLIPTextModelWithProjection(hc).double().eval()
    sd = U.random_text_state(cfg, seed=5)
    missing, unexpected = m.load_state_dict(sd, strict=False)
    assert not unexpected and all("position_ids" in k for k in missing), (missing, unexpected)
    ids = U.text_ids(cfg, [5, 20, 40, 76], seed=6)
    with torch.no_grad():
        want = m(input_ids=ids).text_embeds
    got = U.text_ref64(sd, cfg, ids)
    err = float((got - want).abs().max())
    print(f"text restatement vs transformers: {err:.2e}")
    assert err <= 1e-12


def test_text_tower_matches_restatement():
    from scaledreamer_amd.clip_eval import ClipTextTower

    cfg = dict(U.TINY_TEXT)
    sd = U.random_text_state(cfg, seed=7)
    ids = U.text_ids(cfg, [5, 20, 40, 76], seed=8)
    want = U.text_ref64(sd, cfg, ids)
    want = want / want.norm(dim=-1, keepdim=True)
    got = ClipTextTower(sd, {"text_config": cfg, "projection_dim": 64}, device="cpu", dtype=torch.float64).text_features(ids, chunk=3)
    assert float((got - want).abs().max()) <= 1e-12
    got32 = ClipTextTower(sd, cfg, device="cpu").text_features(ids)
    assert got32.dtype == torch.float32 and float((got32.double() - want).abs().max()) <= 1e-4
    with pytest.raises(NotImplementedError):
        ClipTextTower(sd, dict(cfg, hidden_act="gelu"), device="cpu")


@pytest.mark.parametrize("H", [37, 100, 224, 225, 512])
def test_resize_tables_reproduce_pil(H):
    from scaledreamer_amd.clip_eval import resize_tables

    frame = U.random_frames(1, H, H + 17, seed=H)[0]
    bounds, kk = resize_tables(H, 224)
    assert bounds.dtype == np.int32 and kk.dtype == np.int32 and bounds.shape == (224, 2) and kk.shape[0] == 224
    assert (bounds[:, 0] >= 0).all() and (bounds[:, 0] + bounds[:, 1] <= H).all() and (bounds[:, 1] <= kk.shape[1]).all() and (kk >= 0).all()
    got = U.apply_tables(frame, 224, (bounds, kk))
    want = U.pil_resize(frame, 224)
    assert got.shape == want.shape == (224, 224, 3)
    assert int((got != want).sum()) == 0


def test_vision_tower_refuses_configs_outside_the_family():
    from scaledreamer_amd.clip_eval import ClipVisionTower

    for bad in (dict(num_attention_heads=4), dict(hidden_act="gelu"), dict(hidden_size=2112, num_attention_heads=33)):
        with pytest.raises(NotImplementedError, match="head dim 64"):
            ClipVisionTower({}, dict(U.TINY_VISION, **bad), device="cpu")


class _StubTower:
    """image embedding = a fixed feature chosen by the frame's first byte"""

    def __init__(self, feats):
        self.feats = feats

    def __call__(self, frames):
        return self.feats[frames[:, 0, 0, 0].long()]


def test_evaluate_dir_walk_averages_and_files(tmp_path, monkeypatch):
    from PIL import Image

    from scaledreamer_amd import clip_eval as CE

    def score64(img, txt, own):
        sim, top1, _ = U.score_ref64(img, txt, own)
        return sim.float(), top1.int()

    monkeypatch.setattr(CE, "score", score64)
    g = torch.Generator().manual_seed(11)
    txt = torch.randn(4, 16, generator=g)
    txt = txt / txt.norm(dim=-1, keepdim=True)
    names = ["a_red_fox", "empty_one", "moon", "zebra_on_a_hill"]                  # sorted; prompt index = position
    feats = torch.randn(8, 16, generator=g) * 0.05
    # byte v -> feature: near its own prompt's text for v < 6, near another prompt's for the two "wrong" frames
    plan = {"a_red_fox": {"10.png": 0, "2.png": 1, "1.png": 6}, "moon": {"0.png": 2, "1.png": 3}, "zebra_on_a_hill": {"3.png": 4, "0.png": 5, "7.bmp": 7}}
    near = {0: 0, 1: 0, 6: 2, 2: 2, 3: 2, 4: 3, 5: 3, 7: 0}
    for v, p in near.items():
        feats[v] += 3.0 * txt[p]
    os.makedirs(tmp_path / "empty_one")
    (tmp_path / "notes.txt").write_text("not a prompt directory")
    for name, files in plan.items():
        os.makedirs(tmp_path / name)
        for fname, v in files.items():
            Image.fromarray(np.full((8, 12, 3), v, np.uint8)).save(tmp_path / name / fname)
        (tmp_path / name / "readme.md").write_text("not an image")
    seen = []

    def fake_tokenizer(prompts):
        seen.extend(prompts)
        return torch.zeros(len(prompts), 77, dtype=torch.long)

    class _Text:
        def text_features(self, ids):
            assert tuple(ids.shape) == (4, 77)
            return txt

    scorer = CE.ClipScorer(_StubTower(feats), _Text(), fake_tokenizer, device="cpu")
    sim, rec = scorer.evaluate_dir(str(tmp_path), batch_size=2)
    assert seen == ["a red fox", "empty one", "moon", "zebra on a hill"]
    assert list(sim) == list(rec) == ["a_red_fox", "moon", "zebra_on_a_hill"]       # the empty directory is a candidate, not a result
    unit = feats / feats.norm(dim=-1, keepdim=True)
    for i, name in enumerate(names):
        if name not in plan:
            continue
        vals = [float((unit[v] @ txt[i]).float()) for v in plan[name].values()]
        assert sim[name] == pytest.approx(sum(vals) / len(vals), abs=1e-6)
        hits = [near[v] == i for v in plan[name].values()]
        assert rec[name] == sum(hits) / len(hits)
    assert rec == {"a_red_fox": 2 / 3, "moon": 1.0, "zebra_on_a_hill": 2 / 3}
    for fname, d in (("similarity.txt", sim), ("recall.txt", rec)):
        lines = (tmp_path / fname).read_text().split("\n")
        assert lines[-1] == "" and len(lines) == len(d) + 2
        assert lines[:-2] == [f"{k}: {v}" for k, v in d.items()]
        assert lines[-2] == f"avgerage: {sum(d.values()) / len(d)}"
    # the in-memory path gives the same numbers as the walk
    scorer.set_prompts([n.replace("_", " ") for n in names], txt, names)
    for i, name in enumerate(names):
        if name in plan:
            scorer.add(torch.tensor(list(plan[name].values()), dtype=torch.uint8).view(-1, 1, 1, 1).expand(-1, 8, 12, 3), i)
    sim2, rec2 = scorer.results()
    assert rec2 == rec and all(sim2[k] == pytest.approx(sim[k], abs=1e-7) for k in sim)
