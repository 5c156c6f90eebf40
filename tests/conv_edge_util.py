"""Helpers of test_conv_edges_cpu.py / test_gpu_conv_edges.py: the im2col operand of every 3x3 convolution form of asd_gemm_f16 in
float64, launches of those forms with a pinned plan, and operands placed inside NaN-filled allocations.

The operand is built from the DEFINITIONS of the forms (include/asd_hip.h: asd_gemm_args.conv / upsample, hip_ops.conv3x3,
weights._pack_conv3x3 / _pack_upsample_conv3x3), by integer index arithmetic over whole index tensors - not from the kernels' address code:
  output pixel (b, Y, X), tap (ky, kx), k = (ky, kx, cin):
    upsample 0   reads x[b, Y stride + ky - pad, X stride + kx - pad]; pad 1: zeros on every side; pad 0: the VAE Downsample convention
                 F.pad(x, (0, 1, 0, 1)), zeros below and right only (coordinates never go negative)
    upsample 1   nearest 2x, then 3x3 / stride 1 / pad 1: u = Y + ky - pad in the UPSAMPLED frame [0, 2 Hin), reads x[b, u // 2, ...]
    upsample 2   input gradient of a stride-2 convolution with forward padding `pad`: x is dY, the output dX;
                 dX[Y, X] += dY[(Y + pad - ky) / 2, (X + pad - kx) / 2] W[ky, kx] where both numerators are even, >= 0 and in range
    upsample 3   the parity form of upsample 1: rows ordered [parity (a, b)][batch][y][x] over LOW-resolution positions, row -> output
                 pixel (batch, 2 y + a, 2 x + b); four taps (dy, dx) reading x[y - 1 + a + dy, x - 1 + b + dx], k = (dy, dx, cin); the weight
                 operand holds one [N, 4 Cin] matrix of pre-summed fp16 taps per parity
With Wp the packed fp16 operand as the kernel receives it, ref = A Wp^T and S = |A| |Wp|^T, and a convolution is the fp16-product,
fp32-sum arithmetic of the linear GEMM with K = taps * Cin: the bound gemm_bound(ref, S, ..., K) of gemm_edge_util.py applies unchanged
(for the parity form too: its reference uses the pre-summed fp16 taps, so the rounding of those sums is not part of the error)."""
import ctypes as C

import torch


def conv_out_hw(H, W, stride=1, pad=1, upsample=0):
    """output size of a form whose size follows from the input's (upsample 2 needs an explicit one: two input sizes share a dY size)"""
    if upsample in (1, 3):
        return 2 * H, 2 * W
    assert upsample == 0
    extra = 2 if pad == 1 else 1          # pad 0: one zero row below, one zero column right
    return (H + extra - 3) // stride + 1, (W + extra - 3) // stride + 1


def _grid(*sizes, device):
    return [g.reshape(-1) for g in torch.meshgrid(*[torch.arange(n, device=device) for n in sizes], indexing="ij")]


def conv_operand(x, stride=1, pad=1, upsample=0, out_hw=None):
    """x: NHWC [B, Hin, Win, Cin] -> float64 A [M, taps * Cin] (M = B Hout Wout; parity form: 4 B Hin Win rows in parity-major order)"""
    B, Hin, Win, Cin = x.shape
    xd, dev = x.double(), x.device
    assert pad in (0, 1) and stride in (1, 2) and (upsample == 0 or stride == 1)
    if upsample == 3:
        a, b, bi, y, xx = _grid(2, 2, B, Hin, Win, device=dev)
        taps = [(dy, dx) for dy in (0, 1) for dx in (0, 1)]
    else:
        Hout, Wout = out_hw if out_hw is not None else conv_out_hw(Hin, Win, stride, pad, upsample)
        bi, Y, X = _grid(B, Hout, Wout, device=dev)
        taps = [(ky, kx) for ky in range(3) for kx in range(3)]

    def source(o, k, par, n_in):
        """(input coordinate, valid) along one axis of output coordinate o under tap offset k"""
        if upsample == 3:
            i = o - 1 + par + k
            return i, (i >= 0) & (i < n_in)
        if upsample == 0:
            i = o * stride + k - pad
            return i, (i >= 0) & (i < n_in)
        if upsample == 1:
            u = o + k - pad
            return u // 2, (u >= 0) & (u < 2 * n_in)
        n = o + pad - k
        return n // 2, (n >= 0) & (n % 2 == 0) & (n // 2 < n_in)

    cols = []
    for ty, tx in taps:
        yi, oky = source(y if upsample == 3 else Y, ty, a if upsample == 3 else 0, Hin)
        xi, okx = source(xx if upsample == 3 else X, tx, b if upsample == 3 else 0, Win)
        v = xd[bi, yi.clamp(0, Hin - 1), xi.clamp(0, Win - 1)]
        cols.append(torch.where((oky & okx)[:, None], v, torch.zeros_like(v)))
    return torch.cat(cols, 1)


def parity_output_rows(B, Hin, Win, device="cpu"):
    """row of the NHWC output [B, 2 Hin, 2 Win] that each parity-major row of conv_operand(upsample=3) computes"""
    a, b, bi, y, xx = _grid(2, 2, B, Hin, Win, device=device)
    return (bi * 2 * Hin + 2 * y + a) * 2 * Win + 2 * xx + b


def conv_products(A, wp, upsample=0, rows=None):
    """float64 (A Wp^T, |A| |Wp|^T) in the row order of the OUTPUT; parity form: wp = [4 N, 4 Cin], one matrix per parity, rows =
    parity_output_rows(...)"""
    wd = wp.double()
    if upsample != 3:
        return A @ wd.T, A.abs() @ wd.abs().T
    w4, a4 = wd.view(4, wd.shape[0] // 4, wd.shape[1]), A.view(4, A.shape[0] // 4, A.shape[1])
    lin, S = torch.bmm(a4, w4.transpose(1, 2)).reshape(A.shape[0], -1), torch.bmm(a4.abs(), w4.abs().transpose(1, 2)).reshape(A.shape[0], -1)
    out_lin, out_S = torch.empty_like(lin), torch.empty_like(S)
    out_lin[rows], out_S[rows] = lin, S
    return out_lin, out_S


# ---- GPU side -----------------------------------------------------------------------------------------------------------------------
def poisoned(t, margin):
    """a contiguous copy of the fp16 tensor t inside a larger allocation whose other halfs, `margin` in front and behind, are NaN: a
    read outside the operand makes the output non-finite.  margin % 8 == 0 keeps the copy 16-byte aligned as the kernels require."""
    assert t.dtype == torch.float16 and margin % 8 == 0 and margin > 0
    buf = torch.full((t.numel() + 2 * margin,), float("nan"), dtype=torch.float16, device=t.device)
    view = buf[margin:margin + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == 0
    return view


def workspace(M, N, split_k):
    """the split-K workspace of a launch, sized by the library, with sentinels on either side (None at split_k <= 1)"""
    from gemm_edge_util import GuardedFlat
    from scaledreamer_amd._lib import GemmArgs, lib

    if split_k <= 1:
        return None
    g = GemmArgs()
    g.M, g.N, g.K, g.split_k = M, N, 8, split_k
    nbytes = lib().asd_gemm_workspace_bytes(C.byref(g))
    assert nbytes == split_k * M * N * 4, "asd_gemm_workspace_bytes: split_k fp32 slabs [M, N]"
    return GuardedFlat(nbytes // 4)


def launch_conv(x, w, c, tile, split_k, hout, wout, stride=1, pad=1, upsample=0, bias=None, row_bias=None, rows_per_group=1, residual=None,
                act=0, out_f32=False, ws=None):
    """asd_gemm_f16 as a 3x3 convolution of the NHWC image batch x on the plan (tile, split_k); returns (status, error text).  w: the
    packed operand [N, 9 Cin] (parity form: [4 N, 4 Cin]).  Nothing is chosen by a plan file, a cost model or a timing."""
    from scaledreamer_amd._lib import GemmArgs, lib, stream
    from scaledreamer_amd.diffusion import hip_ops as H

    B, Hin, Win, Cin = x.shape
    assert x.is_contiguous() and w.stride(1) == 1
    g = GemmArgs()
    g.A, g.W, g.C = x.data_ptr(), w.data_ptr(), c.data_ptr()
    g.M, g.N, g.K = B * hout * wout, (w.shape[0] // 4 if upsample == 3 else w.shape[0]), w.shape[1]
    g.lda, g.ldw, g.ldc = 0, w.stride(0), c.stride(0)
    g.conv, g.Hin, g.Win, g.Cin, g.Hout, g.Wout, g.stride, g.pad, g.upsample = 1, Hin, Win, Cin, hout, wout, stride, pad, upsample
    if bias is not None:
        g.bias = bias.data_ptr()
    g.rows_per_group = 1
    if row_bias is not None:
        g.row_bias, g.ld_row_bias, g.rows_per_group = row_bias.data_ptr(), row_bias.stride(0), rows_per_group
    if residual is not None:
        g.residual, g.ldr = residual.data_ptr(), residual.stride(0)
    g.act, g.out_f32 = act, int(out_f32)
    g.zero_page = H.zero_page(x.device).data_ptr()
    g.tile_cfg, g.split_k = tile + 1, split_k
    if ws is not None:
        g.workspace = ws.data_ptr()
    rc = lib().asd_gemm_f16(C.byref(g), stream())
    return rc, (lib().asd_last_error().decode() if rc else "")
