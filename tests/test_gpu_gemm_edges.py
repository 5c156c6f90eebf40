"""Every PLAIN row of the GEMM tile table (csrc/gemm.hip: asd_gemm_tiles) on the linear-GEMM shapes at which its kernel takes another
path — row clamp and store guard, ragged last k-step, a ring prologue longer than the reduction, k-groups and split-K slices without a
k-step, both epilogues — with the plan pinned (tile_cfg = row + 1, explicit split_k), every output element held to a bound derived for
that element against a float64 reference, and the output inside a sentinel-filled buffer that must stay bit-identical around it.
The bounds are derived in gemm_edge_util.py; each test prints the worst err / bound it met and asserts how many launches it made."""
import pytest
import torch

import gemm_edge_util as U
from gemm_edge_util import Guarded, GuardedFlat, Report, geometry, launch

pytestmark = pytest.mark.gpu


def _shapes(tile):
    bm, bn, nst, kg, _ = geometry(tile)
    Ms = [1, 15, bm - 1, bm, bm + 1, 2 * bm + 17]
    Ns = [4, 60, 64, 68, bn + 4, 2 * bn] if bn in (64, 128) else [bn, 2 * bn]
    Ks = sorted({8, 56, 64, 72, 64 * (nst - 1) - 8, 64 * (nst - 1), 64 * nst + 8, 64 * kg - 8, 64 * kg, 64 * (2 * kg + 1) + 24})
    Ns = sorted(set(Ns))          # bn + 4 = 68 on the 64-wide tiles
    assert len(set(Ms)) == 6 and len(Ns) == (5 if bn == 64 else 6 if bn == 128 else 2) and all(k > 0 and k % 8 == 0 for k in Ks)
    return Ms, Ns, Ks


class _Pool:
    """one A [max M, max K] and one W [max N, max K] per tile; the float64 products of their leading K columns are formed once per K and
    sliced per (M, N) (the operands of a launch are contiguous copies of the same slices: lda = ldw = K)"""

    def __init__(self, M, N, K, seed):
        self.A, self.W = U.rand16(M, K, seed=seed), U.rand16(N, K, seed=seed + 1, scale=0.125)
        self._k = None

    def ref(self, K):
        if self._k != K:
            a, w = self.A[:, :K].double(), self.W[:, :K].double()
            self._k, self._lin, self._S = K, a @ w.T, a.abs() @ w.abs().T
        return self._lin, self._S

    def operands(self, M, N, K):
        return self.A[:M, :K].contiguous(), self.W[:N, :K].contiguous()


def _assert_refused(rc, msg, word, guard, label):
    assert rc != 0 and word in msg, f"{label}: expected a refusal naming '{word}', got status {rc} '{msg}'"
    assert bool(guard.intact(written=False)), f"{label}: a refused launch wrote to C"


@pytest.mark.parametrize("tile", U.PLAIN)
def test_every_edge_shape_at_split_1(tile):
    Ms, Ns, Ks = _shapes(tile)
    pool, rep = _Pool(max(Ms), max(Ns), max(Ks), seed=100 + tile), Report()
    refused = 0
    for K in Ks:
        lin, S = pool.ref(K)
        for N in Ns:
            for M in Ms:
                a, w = pool.operands(M, N, K)
                c, label = Guarded(M, N), f"M{M} N{N} K{K}"
                rc, msg = launch(a, w, c.view, tile, 1)
                if U.refuses_n(tile, N):
                    _assert_refused(rc, msg, "does not divide N", c, label)
                    refused += 1
                    continue
                assert rc == 0, f"{label}: {msg}"
                ref, s = lin[:M, :N], S[:M, :N]
                rep.add(label, U.worst_ratio(c.view, ref, U.gemm_bound(ref, s, ref.abs(), K)), c.intact())
    rep.finish(f"tile {tile} {geometry(tile)} split_k 1")
    want_refused = sum(U.refuses_n(tile, N) for N in Ns) * len(Ms) * len(Ks)
    assert refused == want_refused and len(rep.labels) == len(Ms) * len(Ns) * len(Ks) - want_refused


@pytest.mark.parametrize("tile", U.PLAIN)
def test_split_k_slices_including_empty_ones(tile):
    """split_k 2 and 3 on four M tails x two N x four K (K = 8 has one k-step: split 2 already leaves a slice empty), split_k 5 on K = 72
    (two k-steps, three empty slices), and one partials_only launch whose fp32 slabs are summed in float64 here.  The slabs live in a
    workspace with sentinels on either side."""
    bm, bn, nst, kg, _ = geometry(tile)
    Ms = [1, bm - 1, bm + 1, 2 * bm + 17]
    Ns = [68 if bn in (64, 128) else bn, 2 * bn]
    Ks = sorted({8, 72, 64 * nst + 8, 64 * (2 * kg + 1) + 24})
    assert len(Ks) == 4
    pool, rep = _Pool(max(Ms), max(Ns), max(max(Ks), 192), seed=200 + tile), Report()
    plans = [(K, sk) for K in Ks for sk in (2, 3)] + [(72, 5)]
    for K, sk in plans:
        lin, S = pool.ref(K)
        for N in Ns:
            for M in Ms:
                a, w = pool.operands(M, N, K)
                c, ws, label = Guarded(M, N), GuardedFlat(sk * M * N), f"M{M} N{N} K{K} split{sk}"
                rc, msg = launch(a, w, c.view, tile, sk, ws=ws.view)
                assert rc == 0, f"{label}: {msg}"
                ref, s = lin[:M, :N], S[:M, :N]
                rep.add(label, U.worst_ratio(c.view, ref, U.gemm_bound(ref, s, ref.abs(), K)), c.intact(), ws.intact())
    # partials_only (K % 64 == 0 is part of its contract): C is not written, the slabs carry no fp16 rounding
    M, N, K, sk = bm + 1, Ns[0], 192, 2
    lin, S = pool.ref(K)
    a, w = pool.operands(M, N, K)
    c, ws = Guarded(M, N), GuardedFlat(sk * M * N)
    rc, msg = launch(a, w, c.view, tile, sk, ws=ws.view, partials_only=True)
    assert rc == 0, msg
    ref, s = lin[:M, :N], S[:M, :N]
    total = ws.view.view(sk, M, N).double().sum(0)
    rep.add(f"M{M} N{N} K{K} split{sk} partials_only", U.worst_ratio(total, ref, U.gemm_bound(ref, s, ref.abs(), K, out_f32=True)),
            c.intact(written=False), ws.intact())
    rep.finish(f"tile {tile} {geometry(tile)} split-K")
    assert len(rep.labels) == (4 * 2 + 1) * 2 * 4 + 1


def _epilogue_items():
    """what differs from the plain launch, one name per launch; 'all' = every compatible item at once"""
    return ["bias", "row_bias", "row_bias_slice", "residual_view", "silu", "out_f32", "lda", "ldc4", "c_plus8", "bias_plus8", "all", "all_narrow"]


@pytest.mark.parametrize("tile", U.PLAIN)
def test_epilogue_matrix_on_a_tail_tile(tile):
    """bias, row_bias (7 rows per group: groups straddle the 16-row fragments; also as a column slice of a wider matrix), a strided residual,
    SiLU, fp32 output, lda > K — each alone and all together — at M = bm + 1 (the next multiple of 7 where row_bias is involved), K = 72,
    N = 68 (narrow epilogue: N % 8 != 0) and N = bn (bn alone on the 256- / 320-wide tiles).  At N = bn the output view, the bias and the
    leading dimensions are 16-byte aligned, which selects the wide epilogue on tiles with whole 32-column groups per wave; 'ldc4' (ldc % 8
    == 4), 'c_plus8' (C 8 bytes past a 16-byte boundary) and 'bias_plus8' (bias 8 bytes past one) each break one condition and force the
    narrow one on the same shape ('all_narrow': all items on the narrow one).  Both must meet the bound; they need not be equal."""
    bm, bn, nst, kg, _ = geometry(tile)
    K, M1 = 72, bm + 1
    M7 = (M1 + 6) // 7 * 7
    Ns = [68, bn] if bn in (64, 128) else [bn]
    Nmax = max(Ns)
    pool = _Pool(M7, Nmax, K, seed=300 + tile)
    lin, S = pool.ref(K)
    a_wide = torch.cat([U.rand16(M7, 8, seed=5), pool.A, U.rand16(M7, 16, seed=6)], 1)          # lda = K + 24, A 16 bytes into the row
    bias_buf = U.rand16(Nmax + 8, seed=400 + tile)
    Nw = (Nmax + 7) // 8 * 8 + 24                                                               # leading dimensions % 8 == 0
    rb_wide = U.rand16(M7 // 7, Nw, seed=401 + tile)
    res_wide = U.rand16(M7, Nw, seed=402 + tile)
    rep = Report()
    for N in Ns:
        w = pool.W[:N].contiguous()
        for item in _epilogue_items():
            every = item in ("all", "all_narrow")
            rb_item = every or item.startswith("row_bias")
            M = M7 if rb_item else M1
            a = a_wide[:M, 8:8 + K] if (every or item == "lda") else pool.A[:M].contiguous()
            kw = {}
            if every or item == "bias":
                kw["bias"] = bias_buf[:N]
            if item == "bias_plus8" or item == "all_narrow":
                kw["bias"] = bias_buf[4:4 + N]
            if item == "row_bias":
                kw.update(row_bias=rb_wide[:, :N].contiguous(), rows_per_group=7)
            if every or item == "row_bias_slice":
                kw.update(row_bias=rb_wide[:, 8:8 + N], rows_per_group=7)
            if every or item == "residual_view":
                kw["residual"] = res_wide[:M, 16:16 + N]
            if every or item == "silu":
                kw["act"] = 1
            f32 = every or item == "out_f32"
            c = Guarded(M, N, f32=f32, col0=12 if item == "c_plus8" else U.GUARD, ld_extra=4 if item in ("ldc4", "all_narrow") else 0)
            label = f"M{M} N{N} K{K} {item}"
            rc, msg = launch(a, w, c.view, tile, 1, out_f32=f32, **kw)
            assert rc == 0, f"{label}: {msg}"
            ref, s, act_abs = U.epilogue_ref(lin[:M, :N], S[:M, :N], kw.get("bias"), kw.get("row_bias"), 7, kw.get("residual"), kw.get("act", 0))
            rep.add(label, U.worst_ratio(c.view, ref, U.gemm_bound(ref, s, act_abs, K, kw.get("act", 0), f32)), c.intact())
    rep.finish(f"tile {tile} {geometry(tile)} epilogues")
    assert len(rep.labels) == len(Ns) * len(_epilogue_items())


@pytest.mark.parametrize("tile", U.PLAIN)
def test_geglu_epilogue(tile):
    """act = 2 on weights packed by pack_geglu_weight: out = value * gelu(gate), N / 2 columns.  Tiles without whole 32-column groups per
    wave must refuse it, and every tile must refuse it under split-K.  The kernel evaluates x Phi(x) with the erf of Abramowitz & Stegun
    7.1.26; against the exact erf form that formula is off by at most E = 2.11e-7 on [-10, 10] (float64 grid of 2e6 + 1 points, measured
    by gelu_formula_error, which this test calls again and holds to that figure); e_act = 2 E |value|.
    A product of a small value and a small gelu(gate) lands in fp16's subnormal range, where the output rounding is half the spacing 2^-24
    whatever |ref| is, and unlike in the linear GEMM no accumulation term is left to cover it: the rounding term is max(2^-11 |ref|, 2^-25)."""
    from scaledreamer_amd.diffusion import hip_ops as H

    bm, bn, nst, kg, wave_n = geometry(tile)
    E = U.gelu_formula_error()
    print(f"GELU formula (A&S 7.1.26) max abs error on [-10, 10]: {E:.3e}")
    assert E <= 2.2e-7
    Ms, Ns, Ks = [1, bm + 1], [64, 2 * bn], [8, 72]
    rep, refused = Report(), 0
    A = U.rand16(max(Ms), max(Ks), seed=500 + tile)
    W, B = U.rand16(max(Ns), max(Ks), seed=501 + tile, scale=0.25), U.rand16(max(Ns), seed=502 + tile)
    for K in Ks:
        for N in Ns:
            half = N // 2
            w, b = W[:N, :K].contiguous(), B[:N].contiguous()
            wp, bp = H.pack_geglu_weight(w, b)
            h = A[:, :K].double() @ w.double().T + b.double()
            Sh = A[:, :K].double().abs() @ w.double().abs().T + b.double().abs()
            for M in Ms:
                a, label = A[:M, :K].contiguous(), f"M{M} N{N} K{K} geglu"
                c = Guarded(M, half)
                rc, msg = launch(a, wp, c.view, tile, 1, bias=bp, act=2)
                if U.refuses_geglu(tile) or U.refuses_n(tile, N):
                    _assert_refused(rc, msg, "GEGLU" if U.refuses_geglu(tile) else "does not divide N", c, label)
                    refused += 1
                    continue
                assert rc == 0, f"{label}: {msg}"
                val, gate = h[:M, :half], h[:M, half:]
                g = U.gelu64(gate)
                ref = val * g
                ev, eg = (K + 8) * U.U24 * Sh[:M, :half], (K + 8) * U.U24 * Sh[:M, half:]
                bound = ev * g.abs() + 1.13 * eg * val.abs() + 1.13 * ev * eg + 2 * E * val.abs() + 2.0 ** -20 * ref.abs()
                rnd = (U.U11 * ref.abs()).clamp_min(2.0 ** -25)      # fp16 output: half an ulp, half the subnormal spacing 2^-24 below 2^-14
                rep.add(label, U.worst_ratio(c.view, ref, (bound + rnd, rnd)), c.intact())
            # GEGLU needs the whole K in one block: refused under split-K on every tile
            a, c, ws = A[:Ms[1], :K].contiguous(), Guarded(Ms[1], half), GuardedFlat(2 * Ms[1] * N)
            rc, msg = launch(a, wp, c.view, tile, 2, bias=bp, act=2, ws=ws.view)
            _assert_refused(rc, msg, "GEGLU", c, f"M{Ms[1]} N{N} K{K} geglu split2")
    want_refused = sum(U.refuses_geglu(tile) or U.refuses_n(tile, N) for N in Ns) * len(Ms) * len(Ks)
    assert refused == want_refused and len(rep.labels) == len(Ms) * len(Ns) * len(Ks) - want_refused
    assert (len(rep.labels) > 0) == (wave_n % 32 == 0)
    if rep.labels:
        rep.finish(f"tile {tile} {geometry(tile)} GEGLU")


@pytest.mark.parametrize("tile", U.PLAIN)
def test_tiles_that_cannot_divide_n_refuse_it(tile):
    """N = 68 and N = bn + 64: accepted by the 64-wide tiles (any N % 4 == 0) and the 128-wide ones (N % 4 == 0), refused by the 256- and
    320-wide ones, before anything is launched."""
    bm, bn, nst, kg, _ = geometry(tile)
    M, K = 15, 72
    pool, rep, refused = _Pool(M, bn + 64, K, seed=600 + tile), Report(), 0
    lin, S = pool.ref(K)
    for N in (68, bn + 64):
        a, w = pool.operands(M, N, K)
        c, label = Guarded(M, N), f"M{M} N{N} K{K}"
        rc, msg = launch(a, w, c.view, tile, 1)
        if U.refuses_n(tile, N):
            _assert_refused(rc, msg, "does not divide N", c, label)
            refused += 1
            continue
        assert rc == 0, f"{label}: {msg}"
        rep.add(label, U.worst_ratio(c.view, lin[:, :N], U.gemm_bound(lin[:, :N], S[:, :N], lin[:, :N].abs(), K)), c.intact())
    assert refused == (2 if bn in (256, 320) else 0) and len(rep.labels) == 2 - refused
    if rep.labels:
        rep.finish(f"tile {tile} {geometry(tile)} N not a multiple of bn")


@pytest.mark.parametrize("tile", U.PLAIN)
def test_layernorm_fold_on_tail_shapes(tile):
    """ln_mode 1 with the row statistics returned, M in {1, bm + 1} x K in {64, 72, 320} x N in {bn + 4 (64- / 128-wide tiles: narrow
    epilogue), 2 bn}, against LayerNorm + matmul + bias in float64.  The fold's cancellation term (x W'^T - mean rowsum(W')) has no bound that
    can be derived in advance, so the yardstick is the unfused route on the same inputs and the same plan (hip_ops.layernorm, then the GEMM):
    the fold's max error may be at most twice that route's on each case.  Measured on an MI355X over the 17 tiles and all their cases: fold / unfused
    between 0.61 and 1.53 (largest at M = 1, where the maximum runs over 64 - 256 elements; both routes are dominated by the fp16 rounding
    of the output there), the statistics at 0.05 of their bounds or less.
    The statistics: mean within (K + 1) u24 mean|x|; rstd within the first-order image of the variance's error, (K + 4) u24 (E[x^2] + 2 mean^2)
    (fp32 sums of exact squares, then E[x^2] - mean^2), times 0.5 rstd / (var + eps), 1 % slack for the second order, plus 4 ulp for rsqrt."""
    from scaledreamer_amd.diffusion import hip_ops as H
    from scaledreamer_amd.diffusion.weights import _ln_fold

    bm, bn, nst, kg, _ = geometry(tile)
    Ms, Ks = [1, bm + 1], [64, 72, 320]
    Ns = [bn + 4, 2 * bn] if bn in (64, 128) else [2 * bn]
    eps, rep, rels = 1e-5, Report(), []
    for K in Ks:
        x_all = (U.rand16(max(Ms), K, seed=700 + tile).float() * 1.5 + U.rand16(max(Ms), 1, seed=701 + tile).float() * 2.0 + 0.7).half()
        gamma, beta = (U.rand16(K, seed=702).float() * 0.2 + 1.0).half(), (U.rand16(K, seed=703).float() * 0.3).half()
        for N in Ns:
            w, bias = U.rand16(N, K, seed=704 + tile, scale=K ** -0.5), U.rand16(N, seed=705 + tile)
            w2, sc = _ln_fold(w, gamma, beta)
            w2, sc32 = w2.contiguous(), sc.view(torch.float32).view(2, N).contiguous()
            for M in Ms:
                x = x_all[:M].contiguous()
                xd = x.double()
                mean, var = xd.mean(1), xd.var(1, unbiased=False)
                rstd = (var + eps).rsqrt()
                ref = ((xd - mean[:, None]) * rstd[:, None] * gamma.double() + beta.double()) @ w.double().T + bias.double()
                label = f"M{M} N{N} K{K} ln"
                c, st = Guarded(M, N), GuardedFlat(2 * M)
                stats = st.view.view(M, 2)
                rc, msg = launch(x, w2, c.view, tile, 1, bias=bias, ln=dict(eps=eps, sc=sc32, stats=stats))
                assert rc == 0, f"{label}: {msg}"
                c2 = Guarded(M, N)
                rc, msg = launch(H.layernorm(x, gamma, beta, eps), w, c2.view, tile, 1, bias=bias)
                assert rc == 0, f"{label} (unfused): {msg}"
                e_fold, e_unf = (c.view.double() - ref).abs().max(), (c2.view.double() - ref).abs().max()
                rels.append(e_fold / e_unf)
                d_mean = (K + 1) * U.U24 * xd.abs().mean(1)
                d_var = (K + 4) * U.U24 * ((xd * xd).mean(1) + 2 * mean * mean)
                d_rstd = 1.01 * 0.5 * rstd * d_var / (var + eps) + 4 * 2.0 ** -24 * rstd
                r_stats = torch.maximum(((stats[:, 0].double() - mean).abs() / d_mean).max(), ((stats[:, 1].double() - rstd).abs() / d_rstd).max())
                r = torch.nan_to_num(torch.maximum(e_fold / (2 * e_unf), r_stats), nan=float("inf"))
                rep.add(label, torch.stack([r, r_stats]), c.intact(), c2.intact(), st.intact())
    rels = torch.stack(rels).cpu()
    print(f"tile {tile} LayerNorm fold: max error fold / unfused in [{float(rels.min()):.3f}, {float(rels.max()):.3f}]")
    rep.finish(f"tile {tile} {geometry(tile)} LayerNorm fold (max of fold / (2 unfused) and statistics err/bound; second figure: statistics alone)")
    assert len(rep.labels) == len(Ms) * len(Ks) * len(Ns)
