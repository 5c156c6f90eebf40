"""The CLIP text encoder on the HIP path (csrc/text.hip, scaledreamer_amd/diffusion/text_hip.py) and the multi-prompt processor on top of it:
each new entry against an exact or float64 reference at the smallest shapes where it can go wrong, the tower against the golden of
transformers' CLIPTextModel (tests/golden/text_encoder_small.npz) within three times the error of the float64 restatement's own fp16-store
emulation, chunking, and the processor end to end over a three-prompt library.  Bounds are stated where they are used; none comes from
what the kernels give.  Only the npz is read: neither transformers nor the reference is needed."""
import ctypes as C
import json
import math
import os

import pytest
import torch

import text_util as T
from gemm_edge_util import SENT16, Guarded, rand16
from test_gpu_attention_edges import _ref_and_bound as attention_ref_and_bound

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _stop_after_a_device_fault():
    """a kernel fault poisons the process: end the session instead of sending more work to the device"""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"device fault, nothing more is launched: {e}", returncode=3)


def _framed(rows, cols):
    """(buffer, view): a contiguous [rows, cols] fp16 view with 8 sentinel rows in front of it and behind it"""
    buf = torch.empty(rows + 16, cols, dtype=torch.float16, device="cuda")
    buf.view(torch.int16).fill_(SENT16)
    return buf, buf[8:8 + rows]


def _frame_intact(buf, rows):
    return bool((buf[:8].view(torch.int16) == SENT16).all() & (buf[8 + rows:].view(torch.int16) == SENT16).all())


# ---- embedding ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P,L,C_", [(3, 77, 128), (1, 77, 1024), (2, 1, 128)])
def test_embed_is_the_fp16_rounding_of_the_fp32_sum(P, L, C_):
    from scaledreamer_amd.diffusion import text_hip as TH

    vocab = 97
    tok, pos = rand16(vocab, C_, seed=1), rand16(77, C_, seed=2, scale=0.5)
    ids = torch.randint(0, vocab, (P, L), generator=torch.Generator().manual_seed(3))
    ids[0, 0], ids[-1, -1] = 0, vocab - 1                                  # both ends of the table
    buf, out = _framed(P * L, C_)
    TH.embed(ids, tok, pos, out=out)
    assert _frame_intact(buf, P * L), "embed wrote outside its [P L, C] rows"
    want = (tok[ids.cuda()].float() + pos[:L].float()).half().view(P * L, C_)
    assert torch.equal(out, want)
    for bad in (-1, vocab):
        wrong = ids.clone()
        wrong[-1, 0] = bad
        with pytest.raises(ValueError, match="input_ids outside"):
            TH.embed(wrong, tok, pos)


def test_embed_kernel_clamps_an_id_outside_the_table():
    """the C entry itself (no host validation): ids one below and one past the table read rows 0 and vocab - 1"""
    from scaledreamer_amd._lib import check, i32, lib, ptr, stream

    vocab, C_ = 50, 128
    tok, pos = rand16(vocab, C_, seed=4), rand16(4, C_, seed=5)
    ids = torch.tensor([[-1, vocab, 7, vocab - 1]], dtype=torch.int32, device="cuda")
    out = torch.empty(4, C_, dtype=torch.float16, device="cuda")
    check(lib().asd_text_embed_f16(ptr(ids), i32(1), i32(4), i32(vocab), i32(C_), ptr(tok), ptr(pos), ptr(out), stream()))
    rows = torch.tensor([0, vocab - 1, 7, vocab - 1], device="cuda")
    assert torch.equal(out, (tok[rows].float() + pos.float()).half())


# ---- GELU ---------------------------------------------------------------------------------------------------------------------------------
GELU_SPECIALS = [0.0, -0.0, 65504.0, -65504.0, 1e-4, -1e-4, 12.0, -12.0]
ERF_FORMULA_ERROR = 1.5e-7          # Abramowitz & Stegun 7.1.26, the bound they give for the formula csrc/gemm_tile.h (gelu_erf) evaluates


@pytest.mark.parametrize("n", [1, 7, 8 * 1024 + 3])
@pytest.mark.parametrize("in_place", [False, True])
def test_gelu(n, in_place):
    """|err| <= 2^-10 |ref| + 2^-24 + 0.5 |x| 1.5e-7: the fp16 store (half an ulp, doubled; half the smallest subnormal) over an fp32
    evaluation, as the quick-GELU test builds its bound, plus what the erf formula itself may be off by: gelu = x (1 + erf(x / sqrt 2)) / 2,
    so an erf error of E is a result error of |x| E / 2.  That last term matters only in the negative tail, where the result is far smaller
    than x.  The special values are rotated through the short launches so every one of them is an input of every n."""
    from scaledreamer_amd.diffusion import text_hip as TH

    worst = 0.0
    for start in range(len(GELU_SPECIALS) if n < len(GELU_SPECIALS) else 1):
        sp = (GELU_SPECIALS[start:] + GELU_SPECIALS[:start])[:n]
        buf = torch.empty(n + 24, dtype=torch.float16, device="cuda")
        buf.view(torch.int16).fill_(SENT16)
        x = (rand16(n, seed=60 + start).float() * 3.0).half()
        x[:len(sp)] = torch.tensor(sp, dtype=torch.float16, device="cuda")
        xd = x.double()
        if in_place:
            y = buf[8:8 + n]
            y.copy_(x)
            TH.gelu(y, out=y)
        else:
            y = buf[8:8 + n]
            TH.gelu(x, out=y)
            assert torch.equal(x.double(), xd), "gelu changed its input"
        assert bool((buf[:8].view(torch.int16) == SENT16).all() & (buf[8 + n:].view(torch.int16) == SENT16).all()), "gelu wrote outside y"
        ref = T.gelu64(xd)
        err = (y.double() - ref).abs()
        assert bool(torch.isfinite(y).all())
        worst = max(worst, float((err / (2.0 ** -10 * ref.abs() + 2.0 ** -24 + 0.5 * ERF_FORMULA_ERROR * xd.abs())).max()))
    print(f"gelu n {n} in_place {in_place}: worst err/bound {worst:.3f}")
    assert worst <= 1.0


# ---- causal attention ---------------------------------------------------------------------------------------------------------------------
CAUSAL = [(3, 2, 77), (1, 16, 77), (2, 2, 1), (2, 2, 16), (2, 2, 17), (1, 2, 64), (1, 2, 65), (1, 2, 128)]


def _poisoned(rows, cols, seed):
    """a [rows, cols] fp16 view that ends exactly at its last row inside a buffer whose 8 following rows are NaN: a key or query row read
    beyond the view turns results into NaN (0 x NaN = NaN)"""
    buf = torch.full((rows + 8, cols), float("nan"), dtype=torch.float16, device="cuda")
    buf[:rows] = rand16(rows, cols, seed=seed)
    return buf[:rows]


def _causal_ref_and_bound(q, k, v, B, heads, L):
    """float64 masked softmax attention and the per-element bound of test_gpu_attention_edges, row by row: query t over its first t + 1 keys"""
    C_ = heads * 64
    refs, bounds = [], []
    for t in range(L):
        qt = q.reshape(B, L, C_)[:, t].contiguous()
        r, b = attention_ref_and_bound(qt, k.contiguous(), v.contiguous(), B, heads, 1, t + 1, L)
        refs.append(r)
        bounds.append(b)
    return torch.stack(refs, 1).reshape(B * L, C_), torch.stack(bounds, 1).reshape(B * L, C_)


def _causal_inputs(B, heads, L, fused, seed=70):
    C_ = heads * 64
    if fused:
        qkv = _poisoned(B * L, 3 * C_, seed)
        return qkv[:, :C_], qkv[:, C_:2 * C_], qkv[:, 2 * C_:]
    return tuple(_poisoned(B * L, C_, seed + i) for i in range(3))


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("B,heads,L", CAUSAL)
def test_causal_attention_against_float64(B, heads, L, fused):
    from scaledreamer_amd.diffusion import text_hip as TH

    C_ = heads * 64
    q, k, v = _causal_inputs(B, heads, L, fused)
    assert q.stride(0) == (3 * C_ if fused else C_)
    o = Guarded(B * L, C_)
    TH.causal_attention(q, k, v, B, heads, L, out=o.view)
    assert bool(o.intact()), "causal attention wrote outside its [B L, heads 64] output"
    ref, bound = _causal_ref_and_bound(q, k, v, B, heads, L)
    err = (o.view.double() - ref).abs()
    ratio = float(torch.nan_to_num(err / bound, nan=math.inf).max())
    print(f"causal attention B{B} h{heads} L{L} fused {fused}: worst err/bound {ratio:.3f}")
    assert ratio <= 1.0


@pytest.mark.parametrize("fused", [False, True])
def test_causality_is_bit_for_bit(fused):
    """rows > t of q, k and v overwritten with +-60000: output rows <= t keep their bits (a masked score is -inf before the maximum, its
    probability exactly 0, and 0 x 60000 adds nothing)"""
    from scaledreamer_amd.diffusion import text_hip as TH

    B, heads, L = 2, 2, 77
    C_ = heads * 64
    q, k, v = _causal_inputs(B, heads, L, fused, seed=80)
    base = TH.causal_attention(q, k, v, B, heads, L).view(B, L, C_).clone()
    sign = 1.0 - 2.0 * ((torch.arange(L, device="cuda")[:, None] + torch.arange(C_, device="cuda")[None, :]) % 2)
    big = (60000.0 * sign).half()
    for t in (0, 15, 16, 40):
        if fused:
            m = torch.cat([q, k, v], 1)                                   # a fresh [B L, 3C] matrix
            m.view(B, L, 3 * C_)[:, t + 1:] = big.repeat(1, 3)[t + 1:]
            q2, k2, v2 = m[:, :C_], m[:, C_:2 * C_], m[:, 2 * C_:]
        else:
            q2, k2, v2 = q.clone(), k.clone(), v.clone()
            for y in (q2, k2, v2):
                y.view(B, L, C_)[:, t + 1:] = big[t + 1:]
        got = TH.causal_attention(q2, k2, v2, B, heads, L).view(B, L, C_)
        assert bool(torch.isfinite(got[:, :t + 1]).all())
        assert torch.equal(got[:, :t + 1].contiguous().view(torch.int16), base[:, :t + 1].contiguous().view(torch.int16)), f"rows <= {t} changed with rows > {t}"


@pytest.mark.parametrize("L", [0, 129, -1])
def test_causal_attention_rejects_lengths_outside_1_to_128(L):
    from scaledreamer_amd._lib import f32, i32, lib, stream

    x = rand16(256, 128, seed=90)
    o = Guarded(256, 128)
    p = lambda t: C.c_void_p(t.data_ptr())
    rc = lib().asd_attention_causal_f16(p(x), i32(128), p(x), i32(128), p(x), i32(128), p(o.view), i32(o.view.stride(0)), i32(1), i32(2), i32(L),
                                        f32(0.125), stream())
    assert rc != 0 and b"[1, 128]" in lib().asd_last_error()
    assert bool(o.intact(written=False)), "an error status must not launch"


# ---- tower --------------------------------------------------------------------------------------------------------------------------------
def _emulation_error(sd, cfg, ids, ref_last):
    emu_last, _ = T.tower_ref64(sd, cfg, ids, fp16_stores=True)
    return float((emu_last - ref_last).abs().max())


def test_tower_against_the_golden_within_three_emulation_errors():
    """max |hip - golden| <= 3 E_emu on last_hidden_state and on pooled, E_emu the error against the golden of the float64 restatement that
    rounds to fp16 at every tensor the engine stores (exact accumulation, exact softmax); the kernels add fp32 accumulation order and fp16
    probabilities, each of the size of one more store rounding per layer.  pooled is the fp32 of the row at argmax, bit for bit."""
    from scaledreamer_amd.diffusion.text_hip import HipClipTextEncoder

    g = T.golden()
    cfg, sd, ids = g["config"], g["sd"], g["input_ids"]
    gold_last, gold_pool = g["last_hidden_state"].double(), g["pooler_output"].double()
    e_emu = _emulation_error(sd, cfg, ids, gold_last)
    enc = HipClipTextEncoder(sd, cfg)
    last, pooled = enc(ids)
    assert last.dtype == torch.float16 and tuple(last.shape) == (4, 77, 128) and pooled.dtype == torch.float32 and tuple(pooled.shape) == (4, 128)
    err = float((last.double().cpu() - gold_last).abs().max())
    err_pool = float((pooled.double().cpu() - gold_pool).abs().max())
    print(f"text tower (gelu): E_emu {e_emu:.3e}, largest component {float(gold_last.abs().max()):.3f}, err {err:.3e}, err / E_emu {err / e_emu:.3f}, "
          f"pooled err {err_pool:.3e}, pooled err / E_emu {err_pool / e_emu:.3f}")
    assert 1e-5 < e_emu < 1e-2
    assert err <= 3.0 * e_emu and err_pool <= 3.0 * e_emu
    rows = last[torch.arange(4, device="cuda"), ids.argmax(-1).cuda()].float()
    assert torch.equal(pooled.view(torch.int32), rows.view(torch.int32))
    # keys with the published checkpoints' prefix load to the same weights
    enc2 = HipClipTextEncoder({"text_model." + k: v for k, v in sd.items()}, cfg)
    assert torch.equal(enc2(ids)[0], last)
    enc.release()
    with pytest.raises(RuntimeError, match="released"):
        enc(ids)


def test_tower_with_quick_gelu_and_first_eos_pooling():
    """the other activation and the other pooling rule (eos_token_id != 2: the first position holding it) against the float64 restatement,
    under the same 3 E_emu rule"""
    from scaledreamer_amd.diffusion.text_hip import HipClipTextEncoder

    g = T.golden()
    cfg, sd, ids = dict(g["config"], hidden_act="quick_gelu", eos_token_id=511), g["sd"], g["input_ids"].clone()
    ids[0, 30] = 511                                                    # a second end token: the first one counts
    ref_last, ref_pool = T.tower_ref64(sd, cfg, ids)
    e_emu = _emulation_error(sd, cfg, ids, ref_last)
    last, pooled = HipClipTextEncoder(sd, cfg)(ids)
    err = float((last.double().cpu() - ref_last).abs().max())
    err_pool = float((pooled.double().cpu() - ref_pool).abs().max())
    print(f"text tower (quick_gelu): E_emu {e_emu:.3e}, err {err:.3e}, err / E_emu {err / e_emu:.3f}, pooled err / E_emu {err_pool / e_emu:.3f}")
    assert 1e-5 < e_emu < 1e-2
    assert err <= 3.0 * e_emu and err_pool <= 3.0 * e_emu
    assert torch.equal(pooled, last[torch.arange(4, device="cuda"), torch.tensor([1, 5, 40, 76], device="cuda")].float())


def test_chunks_agree_within_three_emulation_errors():
    """6 sequences in chunks of 4 + 2 and in one chunk of 6: another M may pick another GEMM tile, so the bound is the tower's, not equality"""
    from scaledreamer_amd.diffusion.text_hip import HipClipTextEncoder

    g = T.golden()
    cfg, sd = g["config"], g["sd"]
    ids = torch.cat([g["input_ids"], g["input_ids"][:2].clone()])
    ids[4, 5:40] = g["input_ids"][2, 5:40]                               # rows 4 and 5 differ from rows 0 .. 3
    ids[5, 1:5] = g["input_ids"][3, 1:5]
    ref_last, _ = T.tower_ref64(sd, cfg, ids)
    e_emu = _emulation_error(sd, cfg, ids, ref_last)
    a_last, a_pool = HipClipTextEncoder(sd, cfg, chunk=4)(ids)
    b_last, b_pool = HipClipTextEncoder(sd, cfg, chunk=6)(ids)
    assert tuple(a_last.shape) == tuple(b_last.shape) == (6, 77, 128)
    d = float((a_last.double() - b_last.double()).abs().max())
    d_pool = float((a_pool.double() - b_pool.double()).abs().max())
    err = float((a_last.double().cpu() - ref_last).abs().max())
    print(f"chunk 4 vs chunk 6: E_emu {e_emu:.3e}, difference {d:.3e} ({d / e_emu:.3f} E_emu), chunked err / E_emu {err / e_emu:.3f}")
    assert 1e-5 < e_emu < 1e-2
    assert d <= 3.0 * e_emu and d_pool <= 3.0 * e_emu and err <= 3.0 * e_emu


# ---- processor end to end -----------------------------------------------------------------------------------------------------------------
PROMPTS = ["a red car, shiny.", "an owl carved from wood", "a brass teapot"]


def _processor(tmp_path, log, **over):
    import scaledreamer_amd.plugins  # noqa: F401
    from scaledreamer_amd.registry import find

    g = T.golden()
    model = T.write_model_dir(tmp_path / "tiny-sd", g["sd"], g["config"])
    os.makedirs(tmp_path / "load", exist_ok=True)
    with open(tmp_path / "load" / "three.json", "w") as f:
        json.dump({"train": PROMPTS, "val": PROMPTS[:1]}, f)
    cfg = dict(prompt_library="three", prompt_library_dir=str(tmp_path / "load"), pretrained_model_name_or_path=model, cache_dir=str(tmp_path / "cache"),
               negative_prompt="ugly, blurry", use_perp_neg=True, front_threshold=30.0, back_threshold=30.0, **over)
    return cfg, find("stable-diffusion-multi-prompt-processor")(cfg, tokenize_fn=T.stub_tokenizer(512, log=log), rank=0, n_ranks=1)


def test_processor_end_to_end_and_one_system_step(tmp_path, monkeypatch):
    """3 prompts + 12 view-dependent strings + the negative prompt = 16 distinct strings, 32 cache files.  (The reference's directions map a
    negative prompt to itself, base.py:105,210-212, so its four direction strings are the negative prompt again and add no file.)"""
    import random

    from test_gpu_latent import _LatentRenderer, _StandInBackend

    from scaledreamer_amd import presets
    from scaledreamer_amd.multiprompt_processors import hash_prompt
    from scaledreamer_amd.registry import find

    log = []
    pcfg, pp = _processor(tmp_path, log)
    strings = pp.all_strings()
    assert len(strings) == 16 and len(set(log)) == len(log) == 16 and pp.encode_calls == 1
    cache = tmp_path / "cache"
    assert len(os.listdir(cache)) == 32
    log2 = []
    _, pp2 = _processor(tmp_path, log2)
    assert log2 == [] and pp2.encode_calls == 0, "a second configure must encode nothing"
    # values: device tensors equal to the files, which hold the encoder's output for the stub tokenizer's ids
    model = pcfg["pretrained_model_name_or_path"]
    load = lambda s, t: torch.load(cache / f"{hash_prompt(model, s, t)}.pt")
    pu = pp2(PROMPTS[1:])
    assert all(t.is_cuda and t.dtype == torch.float32 for t in pu.global_text_embeddings + pu.local_text_embeddings + pu.text_embeddings_vd)
    assert pu.uncond_text_embeddings.is_cuda and pu.uncond_text_embeddings_vd.is_cuda
    for i, p in enumerate(PROMPTS[1:]):
        assert torch.equal(pu.global_text_embeddings[i].cpu(), load(p, "global")) and torch.equal(pu.local_text_embeddings[i].cpu(), load(p, "local"))
        assert torch.equal(pu.text_embeddings_vd[i].cpu(), torch.stack([load(f"{p}, {d} view", "local") for d in ("side", "front", "back", "overhead")]))
    assert torch.equal(pu.uncond_text_embeddings_vd.cpu(), torch.stack([load("ugly, blurry", "local")] * 4))
    assert tuple(torch.stack(pu.text_embeddings_vd).shape) == (2, 4, 77, 128) and tuple(pu.uncond_text_embeddings_vd.shape) == (4, 77, 128)
    from scaledreamer_amd.diffusion.text_hip import HipClipTextEncoder

    g = T.golden()
    last, pooled = HipClipTextEncoder(g["sd"], g["config"])(T.stub_tokenizer(512)([PROMPTS[2], "ugly, blurry"]))
    assert torch.equal(load(PROMPTS[2], "local"), last[0].float().cpu()) and torch.equal(load(PROMPTS[2], "global"), pooled[0].cpu())
    assert torch.equal(load("ugly, blurry", "local"), last[1].float().cpu())

    # one training step of the multi-prompt system with this processor, built from the system's own config through the registry (every
    # string is cached by now, so no tokenizer is asked for), at the sizes test_gpu_latent.py uses for the same system
    torch.manual_seed(0)
    random.seed(0)
    monkeypatch.setenv("WORLD_SIZE", "1")                                # one process: the processor keeps the whole library, as the datamodule below
    dev = torch.device("cuda", 0)
    cfg = presets.asd_sd_hyper_ingp(PROMPTS)
    cfg["system"].update(rgb_as_latents=True, validation_via_video=False, prompt_processor=pcfg)
    cfg["system"]["guidance"] = {"guidance_scale": 7.5}
    for k in list(cfg["system"]["loss"]):
        if k != "lambda_asd":
            cfg["system"]["loss"][k] = 0.0
    cfg["data"].update(prompt_library={"train": PROMPTS, "val": PROMPTS[:1], "test": PROMPTS[:1]})
    system = find(cfg["system_type"])(cfg["system"], guidance_backend=_StandInBackend(context_dim=128))
    assert system.prompt_processor is None
    system.renderer = _LatentRenderer().to(dev)
    system.train()
    system.on_train_batch_start()
    dm = find(cfg["data_type"])(cfg["data"], rank=0, n_ranks=1)
    batch = system._batch_to_device(dm.collate())
    loss = system.training_step(batch)["loss"]
    assert type(system.prompt_processor).__name__ == "StableDiffusionMultiPromptProcessor" and system.prompt_processor.encode_calls == 0
    assert tuple(system.prompt_utils.get_global_text_embeddings().shape) == (len(batch["prompt"]), 128) and bool(torch.isfinite(loss))
    loss.backward()
    grad = system.renderer.gain.grad
    assert grad is not None and bool(torch.isfinite(grad)) and float(grad.abs()) > 0
