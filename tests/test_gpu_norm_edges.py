"""Every entry of csrc/nn_ops.hip at the shapes where its code takes another path: the five GroupNorm entries (slots that do not divide
the block, channels per group that straddle slots, the second slot pass, rows around one apply trip, capped chunk grids with blocks
that own no row, the 512-thread backward statistics kernel, record counts on both sides of the fold limit and of the reducer's trips),
LayerNorm and softmax around their vector counts, the grid-stride loops of GEGLU, SiLU and the row gather on their second trip, the
timestep embedding, concat, transpose and pad-cast.  The entries are called through ctypes on buffers the test owns: operands inside
NaN-filled allocations (a read outside makes the output non-finite), outputs and the statistics workspaces - exactly the documented
sizes - inside sentinel bands that must stay bit-identical.  Every output element is held to the bound norm_edge_util.py derives against
its float64 reference (both checked on the CPU by test_norm_edges_cpu.py, with the mutations that must exceed the bound).  Each test prints
the worst err / bound it met and asserts its launch and refusal counts against its own lists."""
import pytest
import torch
import torch.nn.functional as F

import gemm_edge_util as U
import norm_edge_util as NU
from conv_edge_util import poisoned
from gemm_edge_util import Guarded, GuardedFlat, Report, rand16, worst_ratio
from norm_edge_util import Flat16, fl, i32, i64

pytestmark = pytest.mark.gpu

MARGIN = 64


def _dev(t):
    return poisoned(t.cuda(), MARGIN)


def _poisoned32(t):
    """fp32 tensor inside a NaN-filled allocation"""
    buf = torch.full((t.numel() + 2 * MARGIN,), float("nan"), dtype=torch.float32, device="cuda")
    view = buf[MARGIN:MARGIN + t.numel()].view(t.shape)
    view.copy_(t)
    return view


def _untouched(band):
    if isinstance(band, Guarded):
        return bool(band.intact(written=False))
    if isinstance(band, GuardedFlat):
        return bool(band.intact() & (band.view.view(torch.int32) == U.SENT32).all())
    return band.untouched()


def _refused(result, word, *bands):
    rc, msg = result
    assert rc != 0 and word in msg, f"expected a refusal naming '{word}', got status {rc} '{msg}'"
    assert all(_untouched(b) for b in bands), f"a refused call ({msg}) wrote to its output"
    return 1


def _exact(got, want):
    """the ratio pair of a bit-exact comparison: 0 or inf"""
    same = (got.contiguous().view(torch.int16) == want.contiguous().view(torch.int16)).all() if got.shape == want.shape else torch.tensor(False, device="cuda")
    return torch.where(same, 0.0, float("inf")).double().expand(2)


def _stats_ratio(stats, B, s, q, ds, dq):
    gs, gq = NU.stats_pairs(stats[:B * 64], B)
    return worst_ratio(torch.stack([gs, gq]), torch.stack([s, q]), torch.stack([ds, dq]))


def _gn(case, offset=False):
    B, hw, Cn = case
    return [_dev(t) for t in NU.gn_inputs(B, hw, Cn, seed=hw + Cn, offset_group=offset)]


def _forward_case(rep, label, x, ga, be, launch):
    """every (eps, SiLU) setting of one problem; x: the whole [B, hw, C] tensor the launch normalises; returns the launches made"""
    B, hw, Cn = x.shape
    s, q, ds, dq, n = NU.gn_sums(x)
    made = 0
    for eps in (1e-5, 1e-6):
        for silu in (0, 1):
            ref, bound = NU.gn_forward_ref(x, ga, be, eps, silu, NU.gn_moments(s, q, ds, dq, n, eps))
            y, st = Flat16(B, hw, Cn), GuardedFlat(NU.gn_stats_floats(B))
            rc, msg = launch(eps, silu, y.view, st.view)
            assert rc == 0, f"{label}: {msg}"
            tag = f"{label} eps={eps} silu={silu}"
            rep.add(tag, worst_ratio(y.view, ref, bound), y.intact(), st.intact())
            rep.add(tag + " statistics", _stats_ratio(st.view, B, s, q, ds, dq), st.intact())
            made += 1
    return made


def _single_cases(max_c):
    return [(c, False) for c in NU.GN_CASES if c[2] <= max_c] + [(NU.GN_OFFSET_CASE, True)]


def test_groupnorm_forward():
    """asd_groupnorm_f16, one and two tensors.  x2 given with c2 = 0 is HANDLED, not refused: the entry takes x1 alone and never reads x2
    (every slot's channel is below c1) - shown with an x2 that is all NaN."""
    rep, made = Report(), 0
    for case, offset in _single_cases(4096):
        B, hw, Cn = case
        x, ga, be = _gn(case, offset)
        made += _forward_case(rep, f"{case}{' offset' if offset else ''}", x, ga, be,
                              lambda eps, silu, y, st: NU.groupnorm(x, None, Cn, 0, B, hw, ga, be, eps, silu, y, st))
    for c1, c2 in NU.GN_PAIR_CASES:
        B, hw = 2, 5
        xc, ga, be = _gn((B, hw, c1 + c2))
        x1, x2 = poisoned(xc[..., :c1].contiguous(), MARGIN), poisoned(xc[..., c1:].contiguous(), MARGIN)
        made += _forward_case(rep, f"pair ({c1}, {c2})", xc, ga, be,
                              lambda eps, silu, y, st: NU.groupnorm(x1, x2, c1, c2, B, hw, ga, be, eps, silu, y, st))
    B, hw, Cn = 3, 77, 96
    x, ga, be = _gn((B, hw, Cn))
    nan = torch.full((64,), float("nan"), dtype=torch.float16, device="cuda")
    made += _forward_case(rep, "x2 with c2 = 0", x, ga, be, lambda eps, silu, y, st: NU.groupnorm(x, nan, Cn, 0, B, hw, ga, be, eps, silu, y, st))
    rep.finish("groupnorm forward")
    assert made == 4 * (len(NU.GN_CASES) + 1 + len(NU.GN_PAIR_CASES) + 1)

    refusals = 0
    for c1, c2, word in ((4128, 0, "at most 4096"), (2048, 2080, "at most 4096"), (48, 0, "multiple of 32"), (36, 28, "multiple of 32")):
        Cn = c1 + c2
        x, ga, be = _gn((1, 1, max(Cn, 64)))
        y, st = Flat16(1, 1, max(Cn, 64)), GuardedFlat(NU.gn_stats_floats(1))
        refusals += _refused(NU.groupnorm(x, x if c2 else None, c1, c2, 1, 1, ga, be, 1e-5, 1, y.view, st.view), word, y, st)
    assert refusals == 4


def test_groupnorm_ordered():
    rep, made = Report(), 0
    cases = _single_cases(2048) + [(c, False) for c in NU.GN_ORDERED_EXTRA]
    for case, offset in cases:
        B, hw, Cn = case
        assert B * NU.gn_ordered_chunks(hw)[0] <= 512
        x, ga, be = _gn(case, offset)
        made += _forward_case(rep, f"{case}{' offset' if offset else ''}", x, ga, be,
                              lambda eps, silu, y, st: NU.groupnorm_ordered(x, Cn, B, hw, ga, be, eps, silu, y, st))
    rep.finish("groupnorm ordered")
    assert made == 4 * len(cases) and len(cases) == 12 + 1 + 4

    refusals = 0
    for (B, hw, Cn), word in (((1, 9, 2080), "at most 2048"), ((17, 2049, 32), "at most 16 images")):
        assert Cn > 2048 or B * NU.gn_ordered_chunks(hw)[0] > 512
        x, ga, be = _gn((B, hw, Cn))
        y, st = Flat16(B, hw, Cn), GuardedFlat(NU.gn_stats_floats(B))
        refusals += _refused(NU.groupnorm_ordered(x, Cn, B, hw, ga, be, 1e-5, 0, y.view, st.view), word, y, st)
    assert refusals == 2


# (B, hw, C, records): the record counts at both shapes, then the scratch boundary - 16 slices of 64 floats per batch element fit the
# 64 (512 + batch) floats up to batch 34; from 35 the entries take fewer slices
RECORD_CASES = [(B, hw, Cn, n) for B, hw, Cn in NU.GN_RECORD_SHAPES for n in NU.GN_RECORD_COUNTS] + [(34, 2, 32, 513), (35, 2, 32, 513)]


def test_groupnorm_apply_from_records():
    rep = Report()
    for B, hw, Cn, n in RECORD_CASES:
        x, ga, be = _gn((B, hw, Cn))
        s, q, _, _, cnt = NU.gn_sums(x)
        rec = _poisoned32(NU.split_records(torch.stack([s, q], 2).reshape(B, 64), n, seed=n))
        tot, dtot = NU.record_sums(rec)
        (s, q), (ds, dq) = NU.stats_pairs(tot, B), NU.stats_pairs(dtot, B)
        silu, eps = n % 2, 1e-5
        ref, bound = NU.gn_forward_ref(x, ga, be, eps, silu, NU.gn_moments(s, q, ds, dq, cnt, eps))
        y, st = Flat16(B, hw, Cn), GuardedFlat(NU.gn_stats_floats(B))
        rc, msg = NU.groupnorm_apply(x, Cn, B, hw, ga, be, eps, silu, rec, n, y.view, st.view)
        label = f"({B}, {hw}, {Cn}) records={n} slices={NU.gn_record_slices(n, B)}"
        assert rc == 0, f"{label}: {msg}"
        rep.add(label, worst_ratio(y.view, ref, bound), y.intact(), st.intact())
        rep.add(label + " statistics", _stats_ratio(st.view, B, s, q, ds, dq), st.intact())
    rep.finish("groupnorm apply from records")
    assert len(rep.labels) == 2 * (2 * 13 + 2)
    assert NU.gn_record_slices(513, 34) == 16 and NU.gn_record_slices(513, 35) == 15

    x, ga, be = _gn((1, 1, 4128))
    rec, y, st = _poisoned32(torch.zeros(1, 1, 64)), Flat16(1, 1, 4128), GuardedFlat(NU.gn_stats_floats(1))
    assert _refused(NU.groupnorm_apply(x, 4128, 1, 1, ga, be, 1e-5, 0, rec, 1, y.view, st.view), "at most 4096", y, st) == 1


def _bwd_inputs(case, seed):
    B, hw, Cn = case
    g = torch.Generator().manual_seed(seed)
    return _dev(torch.randn(B, hw, Cn, generator=g).half()), _dev(torch.randn(B, hw, Cn, generator=g).half())


def test_groupnorm_backward_apply_from_records():
    rep = Report()
    for B, hw, Cn, n in RECORD_CASES:
        x, ga, be = _gn((B, hw, Cn))
        dy, add = _bwd_inputs((B, hw, Cn), n)
        s, q, _, _, _ = NU.gn_sums(x)
        fstats = _poisoned32(torch.stack([s, q], 2).reshape(-1).float())
        silu, eps, add = n % 2, 1e-5, (add if n % 3 == 0 else None)
        _, _, (S1, S2) = NU.gn_backward_ref(x, dy, ga, be, eps, silu, fstats)
        rec = _poisoned32(NU.split_records(torch.stack([S1, S2], 2).reshape(B, 64), n, seed=n + 1))
        tot, dtot = NU.record_sums(rec)
        ref, bound, _ = NU.gn_backward_ref(x, dy, ga, be, eps, silu, fstats, add, sums=NU.stats_pairs(tot, B) + NU.stats_pairs(dtot, B))
        dx, scratch = Flat16(B, hw, Cn), GuardedFlat(NU.gn_stats_floats(B) - 64 * B)
        rc, msg = NU.groupnorm_bwd_apply(x, dy, Cn, B, hw, ga, be, eps, silu, fstats, rec, n, add, dx.view, scratch.view)
        label = f"({B}, {hw}, {Cn}) records={n} silu={silu} add={add is not None}"
        assert rc == 0, f"{label}: {msg}"
        rep.add(label, worst_ratio(dx.view, ref, bound), dx.intact(), scratch.intact())
    rep.finish("groupnorm backward apply from records")
    assert len(rep.labels) == 2 * 13 + 2

    x, ga, be = _gn((1, 1, 4128))
    rec, dx, scratch = _poisoned32(torch.zeros(1, 1, 64)), Flat16(1, 1, 4128), GuardedFlat(NU.gn_stats_floats(1) - 64)
    assert _refused(NU.groupnorm_bwd_apply(x, x, 4128, 1, 1, ga, be, 1e-5, 0, rec, rec, 1, None, dx.view, scratch.view), "at most 4096", dx, scratch) == 1


def test_groupnorm_backward():
    """asd_groupnorm_bwd_f16 from the statistics asd_groupnorm_f16 left (checked against the float64 sums first); the last three shapes
    reach the 512-thread statistics kernel, the others do not"""
    rep, made = Report(), 0
    cases = _single_cases(4096) + [(c, False) for c in NU.GN_BWD_WIDE]
    for i, (case, offset) in enumerate(cases):
        B, hw, Cn = case
        assert NU.gn_bwd_is_wide(*case) == (i >= len(cases) - 3)
        x, ga, be = _gn(case, offset)
        dy, add = _bwd_inputs(case, hw + Cn + 1)
        eps = 1e-6
        s, q, ds, dq, n = NU.gn_sums(x)
        y, st = Flat16(B, hw, Cn), GuardedFlat(NU.gn_stats_floats(B))
        rc, msg = NU.groupnorm(x, None, Cn, 0, B, hw, ga, be, eps, 0, y.view, st.view)
        assert rc == 0, msg
        rep.add(f"{case} forward statistics", _stats_ratio(st.view, B, s, q, ds, dq), st.intact())
        fstats = _poisoned32(st.view[:B * 64])
        for silu in (0, 1):
            for a in (None, add):
                ref, bound, _ = NU.gn_backward_ref(x, dy, ga, be, eps, silu, fstats, a)
                dx, bst = Flat16(B, hw, Cn), GuardedFlat(NU.gn_stats_floats(B) - 64 * B)
                rc, msg = NU.groupnorm_bwd(x, dy, Cn, B, hw, ga, be, eps, silu, fstats, a, dx.view, bst.view)
                label = f"{case}{' offset' if offset else ''} silu={silu} add={a is not None}"
                assert rc == 0, f"{label}: {msg}"
                rep.add(label, worst_ratio(dx.view, ref, bound), dx.intact(), bst.intact())
                made += 1
                del ref, bound
    rep.finish("groupnorm backward")
    assert made == 4 * (len(NU.GN_CASES) + 1 + 3)

    x, ga, be = _gn((1, 1, 4128))
    dx, bst = Flat16(1, 1, 4128), GuardedFlat(NU.gn_stats_floats(1) - 64)
    fstats = _poisoned32(torch.zeros(64))
    assert _refused(NU.groupnorm_bwd(x, x, 4128, 1, 1, ga, be, 1e-5, 0, fstats, None, dx.view, bst.view), "at most 4096", dx, bst) == 1


def _ln_inputs(rows, Cn):
    g = torch.Generator().manual_seed(rows * 10007 + Cn)
    return [_dev(t.half()) for t in (torch.randn(rows, Cn, generator=g) * 1.5 + 0.3, torch.randn(Cn, generator=g), 0.5 * torch.randn(Cn, generator=g))]


def test_layernorm():
    rep = Report()
    cases = [(r, c) for c in NU.LN_CS for r in NU.LN_ROWS] + [(8193, 8)]          # 8193 rows: a second grid-stride trip of the 2048 x 4 waves
    for rows, Cn in cases:
        x, ga, be = _ln_inputs(rows, Cn)
        ref, bound = NU.layernorm_ref(x, ga, be, 1e-5)
        y = Flat16(rows, Cn)
        rc, msg = NU.call("asd_layernorm_f16", x, i32(rows), i32(Cn), ga, be, fl(1e-5), y.view)
        assert rc == 0, msg
        rep.add(f"rows={rows} C={Cn}", worst_ratio(y.view, ref, bound), y.intact())
    rep.finish("layernorm")
    assert len(rep.labels) == 41
    refusals = 0
    for Cn in (12, 2056):
        x, ga, be = _ln_inputs(2, Cn)
        y = Flat16(2, Cn)
        refusals += _refused(NU.call("asd_layernorm_f16", x, i32(2), i32(Cn), ga, be, fl(1e-5), y.view), "multiple of 8 and <= 2048", y)
    assert refusals == 2


def test_softmax_and_its_gradient():
    rep, scale = Report(), NU.SM_SCALE
    for cols in NU.SM_COLS:
        for rows in NU.SM_ROWS:
            x = NU.poisoned_rows(NU.softmax_rows(rows, cols, scale, seed=cols + rows).cuda(), cols + 8)
            ref, bound = NU.softmax_ref(x, scale)
            y = Guarded(rows, cols)
            ld = y.view.stride(0)
            assert x.stride(0) == cols + 8 and ld == cols + 16
            rc, msg = NU.call("asd_softmax_f16", x, i32(cols + 8), i32(rows), i32(cols), fl(scale), y.view, i32(ld))
            assert rc == 0, msg
            label = f"rows={rows} cols={cols}"
            rep.add(label, worst_ratio(y.view, ref, bound), y.intact())
            rep.add(label + " row sums", worst_ratio(y.view.double().sum(1), torch.ones(rows, dtype=torch.float64, device="cuda"), bound[0].sum(1)), y.intact())
            p = NU.poisoned_rows(y.view, ld)                     # the kernel's own fp16 p
            dp = NU.poisoned_rows(rand16(rows, cols, seed=cols), ld)
            ref, bound = NU.softmax_bwd_ref(p, dp, scale)
            ds = Guarded(rows, cols)
            rc, msg = NU.call("asd_softmax_bwd_f16", p, dp, i32(ld), i32(rows), i32(cols), fl(scale), ds.view)
            assert rc == 0, msg
            rep.add(label + " gradient", worst_ratio(ds.view, ref, bound), ds.intact())
    rep.finish("softmax")
    assert len(rep.labels) == 3 * 16
    refusals = 0
    for cols, ldx in ((8200, 8208), (12, 16), (2048, 2052)):
        x, y = NU.poisoned_rows(rand16(1, cols, seed=1), (ldx + 7) // 8 * 8), Guarded(1, cols)
        refusals += _refused(NU.call("asd_softmax_f16", x, i32(ldx), i32(1), i32(cols), fl(scale), y.view, i32(y.view.stride(0))), "multiple of 8", y)
        if ldx % 8 == 0:
            refusals += _refused(NU.call("asd_softmax_bwd_f16", x, x, i32(ldx), i32(1), i32(cols), fl(scale), y.view), "multiple of 8", y)
    assert refusals == 5


def test_geglu_silu_timestep():
    rep = Report()
    for rows, c in ((1, 8), (8193, 512)):                       # 8193 x 64 slots: one more than the 2048 x 256 threads of the grid
        h = _dev(rand16(rows, 2 * c, seed=c, scale=2.0))
        ref, bound = NU.geglu_ref(h)
        y = Flat16(rows, c)
        rc, msg = NU.call("asd_geglu_f16", h, i32(rows), i32(c), y.view)
        assert rc == 0, msg
        rep.add(f"geglu ({rows}, {c})", worst_ratio(y.view, ref, bound), y.intact())
    for n in (8, 8 * (524288 + 1)):
        x = _dev(rand16(n, seed=n % 1000, scale=3.0))
        ref, bound = NU.silu_ref(x)
        y = Flat16(n)
        rc, msg = NU.call("asd_silu_f16", x, i64(n), y.view)
        assert rc == 0, msg
        rep.add(f"silu n={n}", worst_ratio(y.view, ref, bound), y.intact())
    for dim in (2, 6, 320, 1280):
        for n in (1, 5, 257):
            t = _poisoned32(torch.tensor([0.0, 0.5, 999.0]).repeat(n)[:n].contiguous())
            ref, bound = NU.timestep_ref(t, dim)
            y = Flat16(n, dim)
            rc, msg = NU.call("asd_timestep_embedding_f16", t, i32(n), i32(dim), y.view)
            assert rc == 0, msg
            rep.add(f"timestep n={n} dim={dim}", worst_ratio(y.view, ref, bound), y.intact())
    rep.finish("geglu, silu, timestep embedding")
    assert len(rep.labels) == 2 + 2 + 12


def test_concat_transpose_padcast_gather_are_bit_exact():
    rep = Report()
    for c1, c2 in ((8, 8), (8, 1272), (1272, 8)):
        for rows in (1, 300):
            x1, x2 = _dev(rand16(rows, c1, seed=c1)), _dev(rand16(rows, c2, seed=c2 + 1))
            y = Flat16(rows, c1 + c2)
            rc, msg = NU.call("asd_concat_f16", x1, i32(c1), x2, i32(c2), i64(rows), y.view)
            assert rc == 0, msg
            rep.add(f"concat ({c1}, {c2}) rows={rows}", _exact(y.view, torch.cat([x1, x2], 1)), y.intact())
    sizes = (1, 63, 64, 65, 130)
    for rows in sizes:
        for cols in sizes:
            ldx = (cols + 7) // 8 * 8 + 8
            x, y = NU.poisoned_rows(rand16(rows, cols, seed=rows * 131 + cols), ldx), Guarded(cols, rows)
            assert ldx > cols and y.view.stride(0) > rows
            rc, msg = NU.call("asd_transpose_f16", x, i32(rows), i32(cols), i32(ldx), y.view, i32(y.view.stride(0)))
            assert rc == 0, msg
            rep.add(f"transpose {rows}x{cols}", _exact(y.view, x.t()), y.intact())
    for c, c_pad in ((8, 32), (3, 8), (32, 32)):
        rows = 37
        x = _poisoned32(torch.randn(rows, c, generator=torch.Generator().manual_seed(c)) * 3)
        y = Flat16(rows, c_pad)
        rc, msg = NU.call("asd_pad_cast_f16", x, i32(rows), i32(c), y.view, i32(c_pad))
        assert rc == 0, msg
        rep.add(f"pad-cast ({c}, {c_pad})", _exact(y.view, F.pad(x, (0, c_pad - c)).half()), y.intact())
    for row_halfs in (8, 8 * 65537):                             # 65537 16-byte words per row: more than the 65 x 256 threads that copy a row
        src = _dev(rand16(5, row_halfs, seed=5))
        idx = torch.tensor([4, 0, 4, 2, 2, 4], dtype=torch.int32, device="cuda")       # repeats, and the last source row
        dst = Flat16(6, row_halfs)
        rc, msg = NU.call("asd_gather_rows_f16", src, idx, i32(6), i64(row_halfs), dst.view)
        assert rc == 0, msg
        rep.add(f"gather row_halfs={row_halfs}", _exact(dst.view, src[idx.long()]), dst.intact())
    rep.finish("concat, transpose, pad-cast, gather")
    assert len(rep.labels) == 6 + 25 + 3 + 2
