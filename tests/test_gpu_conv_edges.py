"""Every row of the GEMM tile table (csrc/gemm.hip: asd_gemm_tiles) as a 3x3 convolution, at the shapes where its addressing takes
another path: non-square and odd images, M below the block, tiles that straddle an image boundary, stride 2 with both paddings, the
generic path with a tap boundary inside a k-step, the fused and the parity-form upsampling, the stride-2 input gradient with and
without its tap skip, split-K slices without a k-step, and the window / ping-pong / weight-streaming kernels on non-square images.
The plan is pinned (tile_cfg = row + 1, explicit split_k).  Every output element is held to the bound of gemm_edge_util.py against the
float64 reference of conv_edge_util.py (checked against torch on the CPU by test_conv_edges_cpu.py); input and weights lie inside
NaN-filled allocations, the output and the split-K workspace inside sentinel bands that must stay bit-identical, and every case stores
once into a 16-byte aligned view (wide epilogue where the tile has one) and once into a view 8 bytes past one with ldc % 8 == 4 (narrow).
Each test prints the worst err / bound it met and asserts its launch and refusal counts against its own lists."""
import pytest
import torch

import conv_edge_util as CU
import gemm_edge_util as U
from gemm_edge_util import Guarded, Report, geometry
from scaledreamer_amd.diffusion import hip_ops as H

pytestmark = pytest.mark.gpu

PLACEMENTS = (dict(col0=U.GUARD, ld_extra=0), dict(col0=12, ld_extra=4))


def _ceil8(n):
    return (n + 7) // 8 * 8


class _Problem:
    """an image batch inside a NaN-filled allocation (two image rows and more on either side), its float64 operand, and its form"""

    def __init__(self, B, Hh, Ww, Cin, stride=1, pad=1, upsample=0, out_hw=None, seed=0):
        self.B, self.H, self.W, self.Cin, self.stride, self.pad, self.upsample = B, Hh, Ww, Cin, stride, pad, upsample
        self.hout, self.wout = out_hw if out_hw is not None else CU.conv_out_hw(Hh, Ww, stride, pad, upsample)
        self.x = CU.poisoned(U.rand16(B, Hh, Ww, Cin, seed=seed), _ceil8(2 * (Ww + 2) * Cin))
        self.A = CU.conv_operand(self.x, stride, pad, upsample, None if upsample == 3 else (self.hout, self.wout))
        self.rows = CU.parity_output_rows(B, Hh, Ww, device=self.x.device) if upsample == 3 else None
        self.M, self.K = B * self.hout * self.wout, self.A.shape[1]
        assert self.A.shape[0] == self.M and self.K == (4 if upsample == 3 else 9) * Cin and bool(torch.isfinite(self.A).all())
        self.label = f"{B}x{Hh}x{Ww}x{Cin}->{self.hout}x{self.wout} s{stride} p{pad} u{upsample}"

    def weights(self, N, seed):
        """the packed fp16 operand as the kernel receives it, inside a NaN-filled allocation (two rows on either side)"""
        if self.upsample == 3:
            w = H.pack_upsample_conv3x3_weight(U.rand16(N, self.Cin, 3, 3, seed=seed, scale=0.125))
            assert w.shape == (4 * N, self.K)
        else:
            w = U.rand16(N, self.K, seed=seed, scale=0.125)
        return CU.poisoned(w, _ceil8(2 * self.K))

    def products(self, w):
        return CU.conv_products(self.A, w, self.upsample, self.rows)

    def epilogue(self, N, seed):
        """bias, one row_bias row per image, residual"""
        return dict(bias=U.rand16(N, seed=seed), row_bias=U.rand16(self.B, N, seed=seed + 1), rows_per_group=self.hout * self.wout,
                    residual=U.rand16(self.M, N, seed=seed + 2))

    def launch(self, w, c, tile, split_k, ws, **kw):
        return CU.launch_conv(self.x, w, c, tile, split_k, self.hout, self.wout, self.stride, self.pad, self.upsample,
                              ws=None if ws is None else ws.view, **kw)


def _run(rep, tile, prob, w, prods, split_k, epi=None, act=0, f32=False, tag=""):
    """one case in both output placements; returns the launches made"""
    lin, S = prods
    N = lin.shape[1]
    kw = dict(epi or {})
    ref, s, act_abs = U.epilogue_ref(lin, S, kw.get("bias"), kw.get("row_bias"), kw.get("rows_per_group", 1), kw.get("residual"), act)
    bound = U.gemm_bound(ref, s, act_abs, prob.K, act, f32)
    for pl in PLACEMENTS:
        c, ws = Guarded(prob.M, N, f32=f32, **pl), CU.workspace(prob.M, N, split_k)
        label = f"{prob.label} N{N} split{split_k}{tag} col0={pl['col0']}"
        rc, msg = prob.launch(w, c.view, tile, split_k, ws, act=act, out_f32=f32, **kw)
        assert rc == 0, f"tile {tile} {label}: {msg}"
        rep.add(label, U.worst_ratio(c.view, ref, bound), c.intact(), *([ws.intact()] if ws is not None else []))
    return len(PLACEMENTS)


def _run_epilogues(rep, tile, prob, w, prods, splits, seed):
    """bias, then row_bias with one group per image, then SiLU, then residual: fp16 and fp32 output on every split of `splits`"""
    epi, n = prob.epilogue(prods[0].shape[1], seed), 0
    for sk in splits:
        for f32 in (False, True):
            n += _run(rep, tile, prob, w, prods, sk, epi=epi, act=1, f32=f32, tag=" epilogue" + (" f32" if f32 else ""))
    return n


def _refused(tile, prob, w, N, split_k, word):
    c, ws, label = Guarded(prob.M, N), CU.workspace(prob.M, N, split_k), f"tile {tile} {prob.label} N{N} split{split_k}"
    rc, msg = prob.launch(w, c.view, tile, split_k, ws)
    assert rc != 0 and word in msg, f"{label}: expected a refusal naming '{word}', got status {rc} '{msg}'"
    assert bool(c.intact(written=False)), f"{label}: a refused launch wrote to C"
    assert ws is None or bool(ws.intact() & (ws.view.view(torch.int32) == U.SENT32).all()), f"{label}: a refused launch wrote to the workspace"
    return 1


# ---- (a) the plain rows ----------------------------------------------------------------------------------------------------------------
def _tap_skip_problems(bm, seed):
    """input gradients (forward: stride 2; pad 0, then the first two again for pad 1) whose rows are at least one block wide: dX 4 x BM (every tile in one image row),
    4 x 1.5 BM (single-row and straddling tiles in one launch), two images of 3 x BM (odd Hout: the second image starts at an odd
    global row).  Wout >= BM and Cin % 64 == 0 is what the kernel's live_ky_parity shortcut asks for (NST == 2, KG == 1 rows take it, the
    others run every k-step and must agree)."""
    ps = [_Problem(1, 2, bm // 2, 64, pad=0, upsample=2, out_hw=(4, bm), seed=seed),
          _Problem(1, 2, 3 * bm // 4, 64, pad=0, upsample=2, out_hw=(4, 3 * bm // 2), seed=seed + 1),
          _Problem(2, 1, bm // 2, 64, pad=0, upsample=2, out_hw=(3, bm), seed=seed + 2)]
    # the first two sizes are also what a pad-1 forward convolution maps onto dY: the other parity of the live taps
    ps += [_Problem(1, 2, bm // 2, 64, pad=1, upsample=2, out_hw=(4, bm), seed=seed + 3),
           _Problem(1, 2, 3 * bm // 4, 64, pad=1, upsample=2, out_hw=(4, 3 * bm // 2), seed=seed + 4)]
    for p in ps:
        assert p.wout >= bm and p.Cin % 64 == 0 and p.wout == 2 * p.W and p.hout in (2 * p.H, 2 * p.H + 1)
    assert ps[0].wout % bm == 0 and ps[1].wout % bm != 0 and ps[2].hout % 2 == 1 and ps[2].pad == 0 and len(ps) == 5
    return ps


def _plain_problems(bm, seed):
    ps = [_Problem(2, 5, 7, 64, seed=seed), _Problem(1, 16, 24, 128, seed=seed), _Problem(3, 3, 3, 64, seed=seed)]          # fast path
    ps += [_Problem(1, 9, 6, 64, stride=2, seed=seed), _Problem(2, 8, 10, 64, stride=2, pad=0, out_hw=(4, 5), seed=seed),
           _Problem(1, 7, 9, 64, stride=2, pad=0, out_hw=(3, 4), seed=seed)]
    for cin in (8, 40, 96):                                                                                               # generic path
        ps += [_Problem(2, 5, 7, cin, seed=seed), _Problem(1, 9, 6, cin, stride=2, seed=seed)]
    ps += [_Problem(2, 3, 5, 64, upsample=1, seed=seed), _Problem(1, 4, 3, 40, upsample=1, seed=seed)]
    ps += [_Problem(2, 3, 5, 64, upsample=3, seed=seed), _Problem(1, 4, 4, 32, upsample=3, seed=seed)]
    for c in (64, 40):
        ps += [_Problem(1, 3, 4, c, pad=1, upsample=2, out_hw=(6, 8), seed=seed), _Problem(1, 3, 4, c, pad=0, upsample=2, out_hw=(7, 9), seed=seed)]
    assert ps[2].M < 64 <= bm and ps[0].M < 128 and len(ps) == 20      # M below the block: 27 rows on every tile, 70 on all but the 64-row ones
    assert all((p.M // 4) % bm for p in ps if p.upsample == 3), "a parity's rows are not a multiple of BM"
    return ps + _tap_skip_problems(bm, seed + 10)


@pytest.mark.parametrize("tile", U.PLAIN)
def test_plain_rows_on_every_convolution_form(tile):
    bm, bn, nst, kg, _ = geometry(tile)
    probs, Ns, rep, refused = _plain_problems(bm, 1000 + tile), [4, 68, 2 * bn], Report(), 0
    for prob in probs:
        for N in Ns:
            w = prob.weights(N, seed=2000 + tile)
            if U.refuses_n(tile, N):
                refused += _refused(tile, prob, w, N, 1, "does not divide N")
                continue
            _run(rep, tile, prob, w, prob.products(w), 1)
    rep.finish(f"tile {tile} {geometry(tile)} convolution forms")
    n_ref = sum(U.refuses_n(tile, N) for N in Ns)
    print(f"tile {tile}: {len(rep.labels)} launches, {refused} refusals")
    assert len(probs) == 25 and refused == len(probs) * n_ref and len(rep.labels) == len(probs) * (len(Ns) - n_ref) * len(PLACEMENTS)


@pytest.mark.parametrize("tile", U.PLAIN)
def test_plain_rows_split_k_and_epilogue(tile):
    """2x5x7x64 (nine k-steps) and the tap-skip gradient with single-row and straddling tiles: split_k 1, 2, 3 and 6 (ceil(9 / 6) = 2
    k-steps per slice: the last slice has none), and the full epilogue at split 1 and 2, fp16 and fp32 output"""
    bm, bn, nst, kg, _ = geometry(tile)
    probs = [_Problem(2, 5, 7, 64, seed=3000 + tile), _tap_skip_problems(bm, 3100 + tile)[1]]
    splits, N = [1, 2, 3, 6], next(n for n in (68, 2 * bn) if not U.refuses_n(tile, n))
    rep = Report()
    for prob in probs:
        k_steps = prob.K // 64
        assert k_steps == 9 and (splits[-1] - 1) * -(-k_steps // splits[-1]) >= k_steps
        w = prob.weights(N, seed=3200 + tile)
        prods = prob.products(w)
        for sk in splits:
            _run(rep, tile, prob, w, prods, sk)
        _run_epilogues(rep, tile, prob, w, prods, (1, 2), seed=3300 + tile)
    rep.finish(f"tile {tile} {geometry(tile)} convolution split-K and epilogue")
    assert len(rep.labels) == len(probs) * (len(splits) + 2 * 2) * len(PLACEMENTS)


# ---- (b) the window rows ---------------------------------------------------------------------------------------------------------------
def _window_refusal(tile, Hh, Ww, Cin, N, split_k):
    """asd_gemm_f16's argument checks for a window row, in its order: N against the tile, the kind's shape conditions (ping-pong: 32-channel
    chunks, image rows in whole patches of bm / 16 rows, whole N tiles), split_k against the 64-channel chunks"""
    kind, bm, bn = H.TILES[tile][:3]
    if U.refuses_n(tile, N):
        return "does not divide N"
    shape_ok = Hh % 16 == 0 and Ww % 16 == 0
    kind_ok = (Cin % 32 == 0 and Hh % (bm // 16) == 0 and N % bn == 0) if kind == H.KIND_PP else Cin % 64 == 0
    if not (shape_ok and kind_ok):
        return "window convolution needs"
    if split_k != 1 and split_k > Cin // 64:
        return "split_k exceeds"
    return None


def _window_lists(tile):
    kind, bm, bn = H.TILES[tile][:3]
    pp = kind == H.KIND_PP
    images = [(1, 32, 16), (2, 32, 48), (1, 64, 16)] if bm == 512 else [(1, 16, 16), (2, 16, 32), (1, 32, 16), (1, 48, 32)]
    cins = [64, 128, 192] + ([32, 96] if pp else [])
    couts = [bn, 2 * bn] + ([8, 72] if bn == 64 else []) + ([72] if pp else [])
    return images, cins, couts


def _window_splits(Cin):
    """1, 2, Cin / 64 and one beyond the channel chunks"""
    return sorted({1, 2, max(Cin // 64, 1), max(Cin // 64, 1) + 1})


@pytest.mark.parametrize("tile", H.WINDOW_TILES)
def test_window_rows_on_non_square_images(tile):
    kind, bm, bn = H.TILES[tile][:3]
    images, cins, couts = _window_lists(tile)
    assert any(h != w for _, h, w in images) and (kind != H.KIND_PP or (72 in couts and bn != 64))
    rep, refused, odd_grids = Report(), 0, 0
    for (B, Hh, Ww) in images:
        for Cin in cins:
            prob = _Problem(B, Hh, Ww, Cin, seed=4000 + tile)
            for N in couts:
                w = prob.weights(N, seed=4100 + tile)
                prods = None
                for sk in _window_splits(Cin):
                    word = _window_refusal(tile, Hh, Ww, Cin, N, sk)
                    if word is not None:
                        refused += _refused(tile, prob, w, N, sk, word)
                        continue
                    prods = prods if prods is not None else prob.products(w)
                    _run(rep, tile, prob, w, prods, sk)
                    odd_grids += (prob.M // bm * -(-N // bn) * sk) % 8 != 0
    # the full epilogue on one non-square geometry, and an image that is no whole number of patches
    B, Hh, Ww = images[1]
    prob = _Problem(B, Hh, Ww, 128, seed=4200 + tile)
    w = prob.weights(bn, seed=4300 + tile)
    n_epi = _run_epilogues(rep, tile, prob, w, prob.products(w), (1, 2), seed=4400 + tile)
    prob = _Problem(1, 16, 24, 64, seed=4500 + tile)
    assert _window_refusal(tile, 16, 24, 64, bn, 1) == "window convolution needs"
    refused += _refused(tile, prob, prob.weights(bn, seed=4600 + tile), bn, 1, "window convolution needs")
    rep.finish(f"tile {tile} {H.TILES[tile]} window convolution")
    cases = [(Hh, Ww, Cin, N, sk) for (_, Hh, Ww) in images for Cin in cins for N in couts for sk in _window_splits(Cin)]
    n_ref = sum(_window_refusal(tile, *c) is not None for c in cases)
    print(f"tile {tile}: {len(rep.labels)} launches, {refused} refusals, {odd_grids} cases whose block count is no multiple of 8")
    assert n_ref > 0 and refused == n_ref + 1 and len(rep.labels) == (len(cases) - n_ref) * len(PLACEMENTS) + n_epi and n_epi == 4 * len(PLACEMENTS)
    assert any(_window_refusal(tile, *c) == "split_k exceeds" for c in cases) and odd_grids > 0
    if kind == H.KIND_PP:
        assert sum(c[3] == 72 for c in cases) == sum(c[3] == 72 and _window_refusal(tile, *c) is not None for c in cases) > 0


# ---- (c) the weight-streaming row ------------------------------------------------------------------------------------------------------
def _ws_refusal(B, Cin, N, split_k):
    """asd_gemm_f16: 'weight-streaming convolution: ... <= 5 images of 8x8, N % 64 == 0, split_k >= 2, Cin % (32 split_k) == 0'"""
    ok = B <= 5 and N % 64 == 0 and split_k >= 2 and Cin % (32 * split_k) == 0
    return None if ok else "weight-streaming"


@pytest.mark.parametrize("tile", [H.WS_TILE])
def test_weight_streaming_row(tile):
    assert tile is not None and H.TILES[tile][0] == H.KIND_WS and not U.refuses_n(tile, 72)
    plans, couts, rep, refused = [(64, 2), (128, 2), (128, 4), (320, 2), (320, 5)], [64, 128], Report(), 0
    for B in range(1, 6):
        probs = {Cin: _Problem(B, 8, 8, Cin, seed=5000 + B) for Cin in sorted({c for c, _ in plans})}
        for Cin, sk in plans:
            prob = probs[Cin]
            for N in couts:
                assert _ws_refusal(B, Cin, N, sk) is None
                w = prob.weights(N, seed=5100 + B)
                prods = prob.products(w)
                _run(rep, tile, prob, w, prods, sk)
                epi = prob.epilogue(N, seed=5200 + B)
                assert epi["rows_per_group"] == 64
                _run(rep, tile, prob, w, prods, sk, epi=epi, tag=" bias row_bias residual")
    bad = [(6, 64, 64, 2), (1, 64, 64, 1), (1, 64, 64, 4), (1, 64, 72, 2)]       # B = 6; split_k = 1; Cin % (32 split_k); Cout = 72
    for B, Cin, N, sk in bad:
        assert _ws_refusal(B, Cin, N, sk) is not None
        prob = _Problem(B, 8, 8, Cin, seed=5300)
        refused += _refused(tile, prob, prob.weights(N, seed=5400), N, sk, "weight-streaming")
    rep.finish(f"tile {tile} {H.TILES[tile]} weight-streaming convolution")
    print(f"tile {tile}: {len(rep.labels)} launches, {refused} refusals")
    assert refused == len(bad) and len(rep.labels) == 5 * len(plans) * len(couts) * 2 * len(PLACEMENTS)
