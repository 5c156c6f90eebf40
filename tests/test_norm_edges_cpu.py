"""The references and bounds of test_gpu_norm_edges.py (norm_edge_util.py) on the CPU, at every shape the GPU test uses:
  1. each float64 reference agrees with torch's own float64 operation (F.group_norm, F.layer_norm, torch.softmax, autograd) to 1e-12;
  2. an fp32 emulation of the kernel's arithmetic - one-pass sums in two different orders, the folded scale and shift, one rounding to
     fp16 - stays within the per-element bound: honest arithmetic alone does not use it up;
  3. every mutation of that emulation exceeds the bound on at least one element, at every shape it applies to: statistics without the
     image's last row, without the last row of one chunk, without one 8-channel slot; a slot that straddles groups using the group of its
     first channel; an element count of hw (C / 32 +- 1); LayerNorm / softmax sums without the row's last 8-column vector; the softmax
     maximum without it; records summed without the last one.  A shape at which one of them hid would be too large to test it."""
import pytest
import torch
import torch.nn.functional as F

import norm_edge_util as NU
from gemm_edge_util import worst_ratio

EPS = 1e-5
SINGLE = NU.GN_CASES + NU.GN_ORDERED_EXTRA + [(2, 5, c1 + c2) for c1, c2 in NU.GN_PAIR_CASES]


def _same(got, want, what):
    err, ref = float((got - want).abs().max()), max(float(want.abs().max()), 1.0)
    assert got.shape == want.shape and err <= 1e-12 * ref, f"{what}: max abs difference {err:.3e} at reference max {ref:.3e}"


def _r(got, ref, bound):
    return float(worst_ratio(got, ref, bound)[0])


def _gn(case, offset=False):
    B, hw, Cn = case
    return NU.gn_inputs(B, hw, Cn, seed=hw + Cn, offset_group=offset)


def _gn_cases():
    return [(c, False) for c in SINGLE] + [(NU.GN_OFFSET_CASE, True)]


# ---- 1. the references ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,offset", _gn_cases())
@pytest.mark.parametrize("silu", [0, 1])
def test_groupnorm_reference_matches_torch(case, offset, silu):
    x, ga, be = _gn(case, offset)
    s, q, ds, dq, n = NU.gn_sums(x)
    ref, _ = NU.gn_forward_ref(x, ga, be, EPS, silu, NU.gn_moments(s, q, ds, dq, n, EPS))
    want = F.group_norm(x.double().permute(0, 2, 1), 32, ga.double(), be.double(), NU.f32(EPS)).permute(0, 2, 1)
    _same(ref, F.silu(want) if silu else want, f"group_norm {case}")


@pytest.mark.parametrize("c1,c2", NU.GN_PAIR_CASES)
def test_two_tensor_groupnorm_is_the_groupnorm_of_the_concatenation(c1, c2):
    x, ga, be = _gn((2, 5, c1 + c2))
    x1, x2 = x[..., :c1].contiguous(), x[..., c1:].contiguous()
    assert torch.equal(torch.cat([x1, x2], 2), x)
    s, q, ds, dq, n = NU.gn_sums(torch.cat([x1, x2], 2))
    ref, _ = NU.gn_forward_ref(torch.cat([x1, x2], 2), ga, be, EPS, 1, NU.gn_moments(s, q, ds, dq, n, EPS))
    want = F.silu(F.group_norm(torch.cat([x1, x2], 2).double().permute(0, 2, 1), 32, ga.double(), be.double(), NU.f32(EPS))).permute(0, 2, 1)
    _same(ref, want, f"group_norm of cat({c1}, {c2})")


BWD_CPU = NU.GN_CASES + NU.GN_BWD_WIDE[:2] + [(2, 256, 1024)]


@pytest.mark.parametrize("case", BWD_CPU)
@pytest.mark.parametrize("silu,add", [(0, 0), (1, 1)])
def test_groupnorm_backward_reference_matches_autograd(case, silu, add):
    """(32, 256, 1024) of the GPU test is checked here at batch 2: the reference has no code that depends on the batch size"""
    B, hw, Cn = case
    x, ga, be = _gn(case, case == NU.GN_OFFSET_CASE)
    g = torch.Generator().manual_seed(7)
    dy, dx_add = torch.randn(B, hw, Cn, generator=g).half(), torch.randn(B, hw, Cn, generator=g).half()
    s, q, _, _, _ = NU.gn_sums(x)
    fstats = torch.stack([s, q], 2).reshape(-1)                      # exact statistics: the definition
    ref, _, _ = NU.gn_backward_ref(x, dy, ga, be, EPS, silu, fstats, dx_add if add else None)
    xa = x.double().requires_grad_(True)
    y = F.group_norm(xa.permute(0, 2, 1), 32, ga.double(), be.double(), NU.f32(EPS)).permute(0, 2, 1)
    (F.silu(y) if silu else y).backward(dy.double())
    _same(ref, xa.grad + (dx_add.double() if add else 0), f"group_norm backward {case}")


def _ln(rows, Cn):
    g = torch.Generator().manual_seed(rows * 10007 + Cn)
    return (torch.randn(rows, Cn, generator=g) * 1.5 + 0.3).half(), torch.randn(Cn, generator=g).half(), (0.5 * torch.randn(Cn, generator=g)).half()


LN_CASES = [(r, c) for c in NU.LN_CS for r in NU.LN_ROWS] + [(8193, 8)]
SM_CASES = [(r, c) for c in NU.SM_COLS for r in NU.SM_ROWS]


@pytest.mark.parametrize("rows,Cn", LN_CASES)
def test_layernorm_reference_emulation_and_mutation(rows, Cn):
    x, ga, be = _ln(rows, Cn)
    ref, bound = NU.layernorm_ref(x, ga, be, EPS)
    _same(ref, F.layer_norm(x.double(), (Cn,), ga.double(), be.double(), NU.f32(EPS)), "layer_norm")
    for order in (0, 1):
        assert _r(NU.emulate_layernorm(x, ga, be, EPS, order), ref, bound) <= 1.0
        assert _r(NU.emulate_layernorm(x, ga, be, EPS, order, "last_vector"), ref, bound) > 1.0


@pytest.mark.parametrize("rows,cols", SM_CASES)
def test_softmax_reference_emulation_and_mutations(rows, cols):
    x = NU.softmax_rows(rows, cols, NU.SM_SCALE, seed=cols + rows)
    assert float((x[0, -8:].float() * NU.SM_SCALE).max()) == 60 and float((x[0].float() * NU.SM_SCALE).topk(2).values[1]) <= -29.5
    assert rows == 1 or (int(x[1].argmax()) >= cols - 8 and bool((x[2] == x[2, 0]).all()))
    ref, bound = NU.softmax_ref(x, NU.SM_SCALE)
    _same(ref, torch.softmax(x.double() * NU.f32(NU.SM_SCALE), 1), "softmax")
    for order in (0, 1):
        p = NU.emulate_softmax(x, NU.SM_SCALE, order)
        assert _r(p, ref, bound) <= 1.0
        assert bool(((p.double().sum(1) - 1).abs() <= bound[0].sum(1)).all())            # per row, as the GPU test checks it
        for m in ("sum_last_vector", "max_last_vector"):
            assert _r(NU.emulate_softmax(x, NU.SM_SCALE, order, m), ref, bound) > 1.0, m


@pytest.mark.parametrize("rows,cols", [(3, 8), (3, 2056), (3, 8192)])
def test_softmax_backward_reference_matches_autograd(rows, cols):
    x = NU.softmax_rows(rows, cols, NU.SM_SCALE, seed=cols)
    dp = torch.randn(rows, cols, generator=torch.Generator().manual_seed(1)).half()
    xa = x.double().requires_grad_(True)
    p = torch.softmax(xa * NU.f32(NU.SM_SCALE), 1)
    p.backward(dp.double())
    _same(NU.softmax_bwd_ref(p.detach(), dp, NU.SM_SCALE)[0], xa.grad, "softmax backward")


def test_elementwise_references_match_torch():
    g = torch.Generator().manual_seed(3)
    h = (2 * torch.randn(5, 32, generator=g)).half()
    _same(NU.geglu_ref(h)[0], h[:, :16].double() * F.gelu(h[:, 16:].double()), "geglu")
    _same(NU.silu_ref(h)[0], F.silu(h.double()), "silu")
    t = torch.tensor([0.0, 0.5, 999.0])
    ref, _ = NU.timestep_ref(t, 6)
    k = torch.arange(3, dtype=torch.float64)
    a = t.double()[:, None] * torch.pow(torch.tensor(10000.0, dtype=torch.float64), -k / 3)[None]
    _same(ref, torch.cat([a.cos(), a.sin()], 1), "timestep embedding")


# ---- 2. and 3. GroupNorm: honest arithmetic inside, mutations outside -------------------------------------------------------------------------
def _chunkings(case):
    """rows per statistics block of asd_groupnorm_f16 and, where the ordered entry takes the shape, of asd_groupnorm_ordered_f16"""
    B, hw, Cn = case
    out = [NU.gn_stats_chunks(B, hw)[1]]
    if Cn <= 2048 and NU.gn_ordered_chunks(hw)[1] != out[0]:
        out.append(NU.gn_ordered_chunks(hw)[1])
    return out


def _mutations(case):
    B, hw, Cn = case
    cg = Cn // 32
    stat = (["last_row_image", "last_row_chunk"] if hw > 1 else []) + ["slot"]
    apply = (["frozen_group"] if cg % 8 else []) + ["cnt_plus"] + (["cnt_minus"] if cg > 1 else [])
    return stat, apply


@pytest.mark.parametrize("case,offset", _gn_cases())
def test_groupnorm_emulation_inside_every_mutation_outside(case, offset):
    x, ga, be = _gn(case, offset)
    s, q, ds, dq, n = NU.gn_sums(x)
    stat_mut, apply_mut = _mutations(case)
    eps32 = NU.f32(EPS)
    for silu in (0, 1):
        ref, bound = NU.gn_forward_ref(x, ga, be, EPS, silu, NU.gn_moments(s, q, ds, dq, n, EPS))
        for order in (0, 1):
            for rpb in _chunkings(case):
                s32, q32 = NU.emulate_gn_sums(x, rpb, order)
                assert bool(((s32.double() - s).abs() <= ds).all() and ((q32.double() - q).abs() <= dq).all())
                assert _r(NU.emulate_gn_apply(x, ga, be, eps32, silu, s32, q32), ref, bound) <= 1.0, (silu, order, rpb)
                for m in stat_mut:
                    sm, qm = NU.emulate_gn_sums(x, rpb, order, m)
                    assert _r(NU.emulate_gn_apply(x, ga, be, eps32, silu, sm, qm), ref, bound) > 1.0, (m, silu, order, rpb)
                    assert not bool(((sm.double() - s).abs() <= ds).all() and ((qm.double() - q).abs() <= dq).all()), m
            for m in apply_mut:
                assert _r(NU.emulate_gn_apply(x, ga, be, eps32, silu, s32, q32, m), ref, bound) > 1.0, (m, silu, order)


@pytest.mark.parametrize("shape", NU.GN_RECORD_SHAPES)
@pytest.mark.parametrize("n", NU.GN_RECORD_COUNTS)
def test_record_sums_inside_and_the_last_record_missed(shape, n):
    x, ga, be = _gn(shape)
    s, q, _, _, cnt = NU.gn_sums(x)
    rec = NU.split_records(torch.stack([s, q], 2).reshape(shape[0], 64), n, seed=n)
    assert rec.shape == (shape[0], n, 64) and (n < 31 or bool((rec[:, :, 1::2] < 0).any()))     # parts of a sum of squares below zero
    tot, dtot = NU.record_sums(rec)
    s, q = NU.stats_pairs(tot, shape[0])
    ds, dq = NU.stats_pairs(dtot, shape[0])
    ref, bound = NU.gn_forward_ref(x, ga, be, EPS, 1, NU.gn_moments(s, q, ds, dq, cnt, EPS))
    for order in (0, 1):
        got = NU.emulate_record_sum(rec, order)
        assert bool(((got.double() - tot).abs() <= dtot).all())
        s32, q32 = (t.float() for t in NU.stats_pairs(got, shape[0]))
        assert _r(NU.emulate_gn_apply(x, ga, be, NU.f32(EPS), 1, s32, q32), ref, bound) <= 1.0
        bad = NU.emulate_record_sum(rec, order, "last_record")
        s32, q32 = (t.float() for t in NU.stats_pairs(bad, shape[0]))
        assert _r(NU.emulate_gn_apply(x, ga, be, NU.f32(EPS), 1, s32, q32), ref, bound) > 1.0


def test_wide_rule_and_slices():
    """the shapes meant to reach the 512-thread backward statistics kernel do, the others do not; the record slices fit their area"""
    assert all(NU.gn_bwd_is_wide(*c) for c in NU.GN_BWD_WIDE) and not any(NU.gn_bwd_is_wide(*c) for c in NU.GN_CASES)
    assert NU.gn_stats_chunks(7, 1000) == (37, 28) and 36 * 28 >= 1000               # the last block owns no row
    assert NU.gn_stats_chunks(1, 4097) == (256, 17) and NU.gn_ordered_chunks(2049) == (32, 65)
    assert [NU.gn_record_slices(n, 2) for n in (96, 97, 129, 511, 513, 8192)] == [0, 4, 5, 16, 16, 16]
    assert NU.gn_record_slices(513, 34) == 16 and NU.gn_record_slices(513, 35) == 15 and NU.gn_record_slices(513, 600) == 1
    for b in (1, 34, 35, 36, 100, 512, 513, 4000):
        assert 64 * b * NU.gn_record_slices(8192, b) <= NU.gn_stats_floats(b) - 64 * b
