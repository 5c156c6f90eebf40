"""Helpers of test_gpu_gemm_edges.py / test_gpu_attention_edges.py: launches of asd_gemm_f16 with a pinned plan, outputs inside
sentinel-filled buffers, float64 references and per-element error bounds.

Bounds (u11 = 2^-11: half an fp16 ulp, relative; u24 = 2^-24: the same for fp32):
  linear GEMM   |got - ref| <= [fp16 output] u11 |ref| + (K + 8) u24 S + e_act,
                S = |a| |w|^T + |bias| + |row_bias| + |residual| element by element.  The products of fp16 numbers are exact in fp32, a sum of
                K of them in ANY order (MFMA blocks, k-groups, split-K slabs) is off by at most (K - 1) u24 sum|terms| to first order, and the
                epilogue adds at most four more roundings: K + 8 leaves the second-order terms room.
  SiLU          the pre-activation error grows by at most the Lipschitz constant of SiLU (1.0998 < 1.1); v_exp_f32 and v_rcp_f32 are 1-ulp
                operations: e_act = 2^-20 |silu(z)| is a 16-ulp margin for exp2 argument, exp2, add, rcp and the product.
  GEGLU         out = val * gelu(gate): (K + 8) u24 (S_val |gelu(gate)| + 1.13 S_gate |val|) (1.13 > max |gelu'| = 1.1290) plus their product,
                plus e_act = 2 E |val| for the kernel's erf formula (E measured by gelu_formula_error) and 2^-20 |ref| for its fp32 evaluation;
                its fp16 output term is max(u11 |ref|, 2^-25): products of two small factors reach the subnormal range."""
import ctypes as C
import math

import numpy as np
import torch

from scaledreamer_amd._lib import GemmArgs, lib, stream
from scaledreamer_amd.diffusion import hip_ops as H

U11, U24 = 2.0 ** -11, 2.0 ** -24
SENT16, SENT32 = 0x5BCD, 0x4B3C614E      # finite fp16 (~249.6) / fp32 (~1.2e7) bit patterns no result of these tests takes
GUARD = 8                                 # rows above / below and columns left / right of every output view

PLAIN = tuple(i for i, r in enumerate(H.TILES) if r[0] == H.KIND_PLAIN)


def geometry(tile):
    """(bm, bn, stages, k-groups, columns per wave) of a row of the library's tile table"""
    _, bm, bn, _, wn, nst, kg = H.TILES[tile]
    return bm, bn, nst, kg, bn // wn


def refuses_n(tile, N):
    """asd_gemm_f16: 'tile configuration does not divide N'"""
    bn = geometry(tile)[1]
    return bn != 64 and N % bn != 0 and not (bn == 128 and N % 4 == 0)


def refuses_geglu(tile, split_k=1):
    """asd_gemm_f16: the GEGLU epilogue needs whole 32-column groups per wave and the whole K in one block"""
    return geometry(tile)[4] % 32 != 0 or split_k != 1


def rand16(*shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).half().cuda()


class Guarded:
    """[M, N] output view with GUARD sentinel rows / columns on every side.  col0 = 8, ld % 8 == 0: the view starts on a 16-byte boundary
    with 16-byte row strides (what the wide epilogue asks for); col0 = 12 starts it 8 bytes past one (fp16); ld_extra = 4 makes ld % 8 == 4."""

    def __init__(self, M, N, f32=False, col0=GUARD, ld_extra=0):
        self.M, self.N, self.col0 = M, N, col0
        self.itype, self.bits = (torch.int32, SENT32) if f32 else (torch.int16, SENT16)
        ld = (col0 + N + GUARD + 7) // 8 * 8 + ld_extra
        self.buf = torch.empty(M + 2 * GUARD, ld, dtype=torch.float32 if f32 else torch.float16, device="cuda")
        self.buf.view(self.itype).fill_(self.bits)
        self.view = self.buf[GUARD:GUARD + M, col0:col0 + N]
        assert self.buf.data_ptr() % 256 == 0 and col0 >= GUARD and ld - col0 - N >= GUARD

    def intact(self, written=True):
        """device bool: every sentinel (written: outside the view; else everywhere) is bit-identical"""
        t = self.buf.view(self.itype)
        if written:
            t = t.clone()
            t[GUARD:GUARD + self.M, self.col0:self.col0 + self.N] = self.bits
        return (t == self.bits).all()


class GuardedFlat:
    """n fp32 values (a split-K workspace) with 64 sentinel values on either side"""

    def __init__(self, n):
        self.n = n
        self.buf = torch.empty(n + 128, dtype=torch.float32, device="cuda")
        self.buf.view(torch.int32).fill_(SENT32)
        self.view = self.buf[64:64 + n]

    def intact(self):
        t = self.buf.view(torch.int32)
        return (t[:64] == SENT32).all() & (t[64 + self.n:] == SENT32).all()


def launch(a, w, c, tile, split_k, bias=None, row_bias=None, rows_per_group=1, residual=None, act=0, out_f32=False, ln=None, ws=None,
           partials_only=False):
    """asd_gemm_f16 on the plan (tile, split_k); returns (status, error text).  Nothing is chosen by a table, a cost model or a timing."""
    g = GemmArgs()
    g.A, g.W, g.C = a.data_ptr(), w.data_ptr(), c.data_ptr()
    g.M, g.N, g.K = a.shape[0], w.shape[0], w.shape[1]
    g.lda, g.ldw, g.ldc = a.stride(0), w.stride(0), c.stride(0)
    if bias is not None:
        g.bias = bias.data_ptr()
    g.rows_per_group = 1
    if row_bias is not None:
        g.row_bias, g.ld_row_bias, g.rows_per_group = row_bias.data_ptr(), row_bias.stride(0), rows_per_group
    if residual is not None:
        g.residual, g.ldr = residual.data_ptr(), residual.stride(0)
    g.act, g.out_f32 = act, int(out_f32)
    g.zero_page = H.zero_page(a.device).data_ptr()
    g.tile_cfg, g.split_k, g.partials_only = tile + 1, split_k, int(partials_only)
    if ws is not None:
        g.workspace = ws.data_ptr()
    if ln is not None:
        g.ln_mode, g.ln_eps, g.ln_sc = 1, ln["eps"], ln["sc"].data_ptr()
        g.ln_stats = ln["stats"].data_ptr()
    rc = lib().asd_gemm_f16(C.byref(g), stream())
    return rc, (lib().asd_last_error().decode() if rc else "")


def epilogue_ref(lin, S, bias=None, row_bias=None, rows_per_group=1, residual=None, act=0):
    """float64 (ref, S, |activation value|) of the epilogue on top of lin = a w^T and S = |a| |w|^T"""
    z = lin
    if bias is not None:
        z, S = z + bias.double(), S + bias.double().abs()
    if row_bias is not None:
        rb = row_bias.double().repeat_interleave(rows_per_group, 0)[:lin.shape[0]]
        z, S = z + rb, S + rb.abs()
    y = z * torch.sigmoid(z) if act == 1 else z
    ref = y
    if residual is not None:
        ref, S = y + residual.double(), S + residual.double().abs()
    return ref, S, y.abs()


def gemm_bound(ref, S, act_abs, K, act=0, out_f32=False):
    """(bound, its output-rounding term)"""
    acc = (K + 8) * U24 * S
    b = 1.1 * acc + 2.0 ** -20 * act_abs if act == 1 else acc
    rnd = torch.zeros_like(ref) if out_f32 else U11 * ref.abs()
    return b + rnd, rnd


def _ratio(num, den):
    r = torch.where(den > 0, num / den, torch.where(num > 0, torch.full_like(num, math.inf), torch.zeros_like(num)))
    return torch.nan_to_num(r, nan=math.inf).max()


def worst_ratio(got, ref, bound):
    """device [2]: max err / bound (inf where a positive error meets a zero bound or the result is not finite), and the same with the
    output-rounding term taken off both sides.  Round-to-nearest reaches its half ulp, so over thousands of fp16 outputs the first figure
    approaches 1 whenever that term dominates (small K); the second shows how much of the arithmetic's own allowance is used."""
    bound, rnd = bound if isinstance(bound, tuple) else (bound, torch.zeros_like(bound))
    err = (got.double() - ref).abs()
    return torch.stack([_ratio(err, bound), _ratio((err - rnd).clamp_min(0), bound - rnd)])


class Report:
    """collects (label, worst ratio, guard band intact) per launch on the device and is read back once"""

    def __init__(self):
        self.labels, self.ratios, self.guards = [], [], []

    def add(self, label, ratio, *guards):
        self.labels.append(label)
        self.ratios.append(ratio)
        self.guards.append(torch.stack([g for g in guards]).all())

    def finish(self, what):
        ratios, guards = torch.stack(self.ratios).cpu(), torch.stack(self.guards).cpu()
        ratios, excess = ratios[:, 0], float(ratios[:, 1].max())
        worst = int(ratios.argmax())
        print(f"{what}: {len(self.labels)} launches, worst err/bound {float(ratios[worst]):.3f} at {self.labels[worst]}; beyond the output rounding {excess:.3f}")
        bad_guard = [self.labels[i] for i in range(len(self.labels)) if not bool(guards[i])]
        assert not bad_guard, f"{what}: memory around the output changed: {bad_guard[:8]}"
        bad = [(self.labels[i], float(ratios[i])) for i in range(len(self.labels)) if not float(ratios[i]) <= 1.0]
        assert not bad, f"{what}: err/bound > 1: {bad[:8]}"
        return float(ratios[worst])


_gelu_err = []


def gelu_formula_error():
    """max |x Phi_AS(x) - x Phi(x)| over a dense grid on [-10, 10] in float64 on the CPU, Phi_AS with the erf of Abramowitz & Stegun
    7.1.26 as csrc/gemm_tile.h (gelu_erf) evaluates it"""
    if not _gelu_err:
        x = np.linspace(-10.0, 10.0, 2_000_001)
        z = np.abs(x) * 0.70710678118654752440
        t = 1.0 / (1.0 + 0.3275911 * z)
        poly = ((((1.061405429 * t - 1.453152027) * t + 1.421413741) * t - 0.284496736) * t + 0.254829592) * t
        tail = poly * np.exp(-z * z)
        phi = np.where(x >= 0, 1.0 - 0.5 * tail, 0.5 * tail)
        exact = 0.5 * x * (1.0 + torch.erf(torch.from_numpy(x / math.sqrt(2.0))).numpy())
        _gelu_err.append(float(np.abs(x * phi - exact).max()))
    return _gelu_err[0]


def gelu64(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))
