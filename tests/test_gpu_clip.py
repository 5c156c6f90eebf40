"""CLIP evaluation on the HIP path (csrc/clip.hip, scaledreamer_amd/clip_eval.py): each new entry against a float64 or byte-exact
reference at the smallest shapes where it can go wrong, asd_attention_f16 at the tower's shapes, the whole image tower against the float64
restatement of clip_util within three times the error of that restatement's own fp16-store emulation, and the scorer end to end over a
synthetic directory.  Bounds are stated where they are used; none comes from what the kernels give."""
import math
import os

import numpy as np
import pytest
import torch

import clip_util as U
from gemm_edge_util import SENT16, Guarded, rand16
from test_gpu_attention_edges import _check as attention_check
from test_gpu_attention_edges import _inputs as attention_inputs
from test_gpu_attention_edges import _ref_and_bound as attention_ref_and_bound

pytestmark = pytest.mark.gpu

S, P = 224, 14


def _fp16_ulp(x):
    """spacing of fp16 at |x| (float64 tensor): 2^(e - 11) for |x| = m 2^e with m in [0.5, 1), 2^-24 in the subnormal range"""
    _, e = torch.frexp(x.abs())
    return torch.maximum(torch.ldexp(torch.ones_like(x), e - 11), torch.full_like(x, 2.0 ** -24))


@pytest.mark.parametrize("B,H,W", [(2, 100, 250), (1, 512, 1536), (3, 224, 224), (1, 37, 64), (1, 225, 300)])
def test_preprocess_matches_pil_bytes_and_fp32_normalisation(B, H, W):
    from scaledreamer_amd import clip_eval as CE

    frames = U.random_frames(B, H, W, seed=H + W)
    want_u8 = np.stack([U.pil_resize(f, S) for f in frames])
    g, kpad = S // P, CE.patch_kpad(P)
    assert kpad == 592
    out = Guarded(B * g * g, kpad)
    _, resized = CE.preprocess(torch.from_numpy(frames).cuda(), S, P, want_resized=True, out=out.view)
    assert bool(out.intact()), "preprocess wrote outside its [B g^2, Kpad] patch rows"
    diff = int((resized.cpu().numpy() != want_u8).sum())
    print(f"preprocess B{B} H{H} W{W}: {diff} bytes differ from PIL")
    assert diff == 0
    got = out.view.cpu()
    assert bool((got[:, 3 * P * P:].view(torch.int16) == 0).all()), "padding columns are not exactly +0"
    want = U.patch_rows(U.normalise_u8(want_u8), P).half().double()
    err = (got[:, :3 * P * P].double() - want).abs()
    ulps = float((err / _fp16_ulp(want)).max())
    print(f"preprocess B{B} H{H} W{W}: patch rows within {ulps:.2f} fp16 ulp of the fp32 normalisation")
    assert ulps <= 1.0


def test_preprocess_rejects_a_frame_narrower_than_high():
    from scaledreamer_amd import clip_eval as CE
    from scaledreamer_amd._lib import AsdError

    with pytest.raises(AsdError, match="narrower"):
        CE.preprocess(torch.zeros(1, 64, 63, 3, dtype=torch.uint8, device="cuda"), S, P)
    with pytest.raises(AsdError, match="narrower"):
        CE.preprocess(torch.zeros(1, 224, 200, 3, dtype=torch.uint8, device="cuda"), S, P)


@pytest.mark.parametrize("B,g2,C_", [(3, 9, 128), (2, 256, 128), (1, 256, 1024)])
def test_embed_matches_float64_layernorm(B, g2, C_):
    """|err| <= 2^-10 |ref| + 1e-5 max|ref|: one fp16 store rounding (2^-11 relative), doubled, plus fp32 statistics"""
    from scaledreamer_amd import clip_eval as CE

    L = g2 + 1
    lpad = (L + 7) // 8 * 8
    patch, cls, pos = rand16(B * g2, C_, seed=1), rand16(C_, seed=2), rand16(L, C_, seed=3, scale=0.5)
    gamma, beta = (1.0 + 0.2 * rand16(C_, seed=4).float()).half(), rand16(C_, seed=5, scale=0.3)
    buf = torch.empty(B * lpad + 16, C_, dtype=torch.float16, device="cuda")
    buf.view(torch.int16).fill_(SENT16)
    out = buf[8:8 + B * lpad].view(B, lpad, C_)
    CE.embed(patch, cls, pos, gamma, beta, 1e-5, B, lpad, out=out)
    assert bool((buf[:8].view(torch.int16) == SENT16).all() & (buf[8 + B * lpad:].view(torch.int16) == SENT16).all()), "embed wrote outside its rows"
    x = torch.cat([cls.double().expand(B, 1, C_), patch.double().view(B, g2, C_)], 1) + pos.double()
    ref = U._ln(x, gamma.double(), beta.double(), 1e-5)
    err = (out[:, :L].double() - ref).abs()
    bound = 2.0 ** -10 * ref.abs() + 1e-5 * ref.abs().max()
    ratio = float((err / bound).max())
    print(f"embed B{B} g2 {g2} C{C_}: worst err/bound {ratio:.3f}")
    assert ratio <= 1.0
    if lpad > L:
        assert bool((out[:, L:].contiguous().view(torch.int16) == 0).all()), "padding rows are not exactly zero"
    else:
        assert L % 8 == 0


QG_SPECIALS = [0.0, -0.0, 65504.0, -65504.0, 1e-4, -1e-4, 12.0, -12.0]


@pytest.mark.parametrize("n", [1, 7, 8 * 1024 + 3])
def test_quick_gelu(n):
    """|err| <= 2^-10 |ref| + 2^-24: the fp16 store (half an ulp, doubled; half the smallest subnormal) over an fp32 evaluation.  The
    special values are rotated through the short launches so every one of them is an input of every n."""
    from scaledreamer_amd import clip_eval as CE

    worst = 0.0
    for start in range(len(QG_SPECIALS) if n < len(QG_SPECIALS) else 1):
        sp = (QG_SPECIALS[start:] + QG_SPECIALS[:start])[:n]
        x = (rand16(n, seed=60 + start).float() * 3.0).half()
        x[:len(sp)] = torch.tensor(sp, dtype=torch.float16, device="cuda")
        buf = torch.empty(n + 24, dtype=torch.float16, device="cuda")
        buf.view(torch.int16).fill_(SENT16)
        y = buf[8:8 + n]
        CE.quick_gelu(x, out=y)
        assert bool((buf[:8].view(torch.int16) == SENT16).all() & (buf[8 + n:].view(torch.int16) == SENT16).all()), "quick_gelu wrote outside y"
        ref = U.quick_gelu64(x.double())
        err = (y.double() - ref).abs()
        assert bool(torch.isfinite(y).all())
        worst = max(worst, float((err / (2.0 ** -10 * ref.abs() + 2.0 ** -24)).max()))
    print(f"quick_gelu n {n}: worst err/bound {worst:.3f}")
    assert worst <= 1.0


@pytest.mark.parametrize("B,heads,lq,lk,lks", [(3, 2, 257, 257, 264), (3, 2, 10, 10, 16)])
def test_attention_at_the_tower_shapes(B, heads, lq, lk, lks):
    """the existing entry through its wrapper at ViT-L/14's token count and the tiny tower's, +-60000 in the masked key rows"""
    from scaledreamer_amd.diffusion import hip_ops as H

    q, k, v = attention_inputs(B, heads, lq, lk, lks, seed=70)
    got = H.attention(q, k, v.t().contiguous(), B, heads, lq, lk, lks)
    ref, bound = attention_ref_and_bound(q, k, v, B, heads, lq, lk, lks)
    attention_check(got, ref, bound, f"clip B{B} h{heads} lq{lq} lk{lk} stride{lks}")


def _tower_case(layers, size, seed):
    """(config, fp16-rounded float64 state dict, frames uint8 [3, size, size + 6, 3], fp16-rounded pixels float64 [3, 3, size, size])"""
    cfg = dict(U.TINY_VISION, num_hidden_layers=layers, image_size=size)
    sd = {k: U.r16(v) for k, v in U.random_vision_state(cfg, seed).items()}
    frames = U.random_frames(3, size, size + 6, seed=seed + 1)
    pixels = U.normalise_u8(np.ascontiguousarray(frames[:, :, :size])).half().double()
    return cfg, sd, frames, pixels


@pytest.mark.parametrize("layers,size", [(2, 42), (1, 224)])
def test_tower_against_float64_within_three_emulation_errors(layers, size):
    """max |n(hip) - n(ref64)| <= 3 E_emu on the L2-normalised embedding, E_emu the error of the restatement that rounds to fp16 at every
    tensor the engine stores (exact accumulation, exact softmax); the kernels add fp32 accumulation order, fp16 probabilities and the
    deferred maximum, each of the size of one more store rounding per layer."""
    from scaledreamer_amd.clip_eval import ClipVisionTower

    cfg, sd, frames, pixels = _tower_case(layers, size, seed=80 + layers)
    n = lambda t: t / t.norm(dim=-1, keepdim=True)
    ref = n(U.vision_ref64(sd, cfg, pixels))
    e_emu = float((n(U.vision_ref64(sd, cfg, pixels, fp16_stores=True)) - ref).abs().max())
    tower = ClipVisionTower(sd, cfg)
    assert (tower.L, tower.Lpad) == ((size // 14) ** 2 + 1, ((size // 14) ** 2 + 8) // 8 * 8)
    emb = tower(torch.from_numpy(frames).cuda())
    assert emb.dtype == torch.float32 and tuple(emb.shape) == (3, 64) and bool(torch.isfinite(emb).all())
    err = float((n(emb.double().cpu()) - ref).abs().max())
    print(f"tower {layers} layers, S {size}: E_emu {e_emu:.3e}, largest component {float(ref.abs().max()):.3f}, err {err:.3e}, err / E_emu {err / e_emu:.3f}")
    assert 1e-5 < e_emu < 1e-2
    assert err <= 3.0 * e_emu


def _score_inputs(B, P_, D, seed):
    g = torch.Generator().manual_seed(seed)
    img = torch.randn(B, D, generator=g) * 7.0
    txt = torch.randn(P_, D, generator=g)
    txt = (txt.double() / txt.double().norm(dim=-1, keepdim=True)).float()
    own = torch.randint(0, P_, (B,), generator=g).int()
    return img, txt, own


@pytest.mark.parametrize("B,P_,D,seed", [(5, 7, 64, 90), (120, 130, 768, 94), (1, 1, 768, 92)])
def test_score_similarity_and_top1(B, P_, D, seed):
    from scaledreamer_amd import clip_eval as CE

    img, txt, own = _score_inputs(B, P_, D, seed)
    ref_sim, ref_top, margin = U.score_ref64(img, txt, own)
    assert float(margin.min()) >= 1e-4, f"pick another seed: top-1 margin {float(margin.min()):.2e}"
    sim, top1 = CE.score(img.cuda(), txt.cuda(), own.cuda())
    assert top1.cpu().tolist() == ref_top.tolist()
    err = float((sim.cpu().double() - ref_sim).abs().max())
    print(f"score B{B} P{P_} D{D}: smallest margin {float(margin.min()):.2e}, worst |sim - ref| {err:.2e}")
    assert err <= 1e-5


def test_score_ties_go_to_the_lowest_index():
    """text row 130 repeats row 3 (another 64-prompt chunk, another wave); images 0-2 point at it: both logits are equal, 3 must win"""
    from scaledreamer_amd import clip_eval as CE

    img, base, own = _score_inputs(9, 130, 64, seed=93)
    img[:3] = 5.0 * base[3] + 0.05 * img[:3] / 7.0
    own[:3] = 3
    txt = torch.cat([base, base[3:4]])
    ref_sim, ref_top, margin = U.score_ref64(img, base, own)
    assert float(margin.min()) >= 1e-4 and ref_top[:3].tolist() == [3, 3, 3]
    sim, top1 = CE.score(img.cuda(), txt.cuda(), own.cuda())
    assert top1.cpu().tolist() == ref_top.tolist()
    assert float((sim.cpu().double() - ref_sim).abs().max()) <= 1e-5
    own_dup = own.clone()
    own_dup[:3] = 130
    sim_dup, top1_dup = CE.score(img.cuda(), txt.cuda(), own_dup.cuda())
    assert torch.equal(sim_dup, sim) and torch.equal(top1_dup, top1), "equal text rows must give equal values"


def test_scorer_end_to_end_over_a_directory(tmp_path):
    """3 prompts x 4 small PNGs through evaluate_dir (PIL decode, upload, resize, tower, text tower, score, files) and through add() on
    the same frames: the same values"""
    from PIL import Image

    from scaledreamer_amd import clip_eval as CE

    cfg = dict(U.TINY_VISION, num_hidden_layers=1)
    tcfg = dict(U.TINY_TEXT)
    vision = CE.ClipVisionTower(U.random_vision_state(cfg, seed=100), cfg)
    text = CE.ClipTextTower(U.random_text_state(tcfg, seed=101), tcfg)
    tokenized = []

    def tokenize(prompts):
        tokenized.extend(prompts)
        return U.text_ids(tcfg, [3 + len(p) for p in prompts], seed=102)

    names = ["a_blue_chair", "an_owl", "the_last_teapot"]
    frames = U.random_frames(12, 30, 45, seed=103).reshape(3, 4, 30, 45, 3)
    for i, name in enumerate(names):
        os.makedirs(tmp_path / name)
        for j in range(4):
            Image.fromarray(frames[i, j]).save(tmp_path / name / f"{j}.png")
    scorer = CE.ClipScorer(vision, text, tokenize)
    sim, rec = scorer.evaluate_dir(str(tmp_path), batch_size=120)
    assert tokenized == ["a blue chair", "an owl", "the last teapot"] and list(sim) == list(rec) == names
    assert all(math.isfinite(v) and -1.0 <= v <= 1.0 for v in sim.values()) and all(v in (0.0, 0.25, 0.5, 0.75, 1.0) for v in rec.values())
    for fname, d in (("similarity.txt", sim), ("recall.txt", rec)):
        assert (tmp_path / fname).read_text() == "".join(f"{k}: {v}\n" for k, v in d.items()) + f"avgerage: {sum(d.values()) / 3}\n"
    txt = scorer.txt.clone()
    assert float((txt.norm(dim=-1) - 1.0).abs().max()) <= 1e-5
    scorer.set_prompts([n.replace("_", " ") for n in names], txt, names)
    for i in range(3):
        scorer.add(torch.from_numpy(frames[i]).cuda(), i)
    sim2, rec2 = scorer.results()
    assert sim2 == sim and rec2 == rec
