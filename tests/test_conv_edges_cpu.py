"""The float64 reference of test_gpu_conv_edges.py (conv_edge_util.conv_operand) against torch's own float64 operations on the CPU, at
the odd and non-square sizes the GPU tests use: the GPU tests then rest on a reference that shares no index code with the kernels.
Every comparison is max |A Wp^T - torch| <= 1e-12 max |torch| (two float64 sums of at most 576 terms in different orders)."""
import pytest
import torch
import torch.nn.functional as F

import conv_edge_util as CU
from scaledreamer_amd.diffusion.weights import _pack_conv3x3, _pack_upsample_conv3x3

COUT = 12


def _rand(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def _same(got, want, what):
    assert got.shape == want.shape, f"{what}: shape {tuple(got.shape)} vs {tuple(want.shape)}"
    err, ref = float((got - want).abs().max()), float(want.abs().max())
    assert ref > 0 and err <= 1e-12 * ref, f"{what}: max abs difference {err:.3e} at reference max {ref:.3e}"


def _nhwc_rows(y_nchw):
    return y_nchw.permute(0, 2, 3, 1).reshape(-1, y_nchw.shape[1])


def _forward(x_nchw, w, stride, pad):
    """the convolution the library documents: pad 1 on every side, or the VAE Downsample padding (zeros below and right only)"""
    if pad == 1:
        return F.conv2d(x_nchw, w, stride=stride, padding=1)
    return F.conv2d(F.pad(x_nchw, (0, 1, 0, 1)), w, stride=stride)


# B, H, W, Cin, stride, pad: the fast-path, stride-2 and generic-path geometries of the GPU tests
PLAIN_FORMS = [(2, 5, 7, 64, 1, 1), (1, 16, 24, 128, 1, 1), (3, 3, 3, 64, 1, 1), (1, 9, 6, 64, 2, 1), (2, 8, 10, 64, 2, 0), (1, 7, 9, 64, 2, 0),
               (2, 5, 7, 8, 1, 1), (2, 5, 7, 40, 1, 1), (2, 5, 7, 96, 1, 1), (1, 9, 6, 8, 2, 1), (1, 9, 6, 40, 2, 1), (1, 9, 6, 96, 2, 1),
               (1, 16, 32, 64, 1, 1), (1, 32, 16, 64, 1, 1), (2, 8, 8, 64, 1, 1)]


@pytest.mark.parametrize("B,H,W,Cin,stride,pad", PLAIN_FORMS)
def test_plain_forms_match_conv2d(B, H, W, Cin, stride, pad):
    x, w = _rand(B, Cin, H, W, seed=1), _rand(COUT, Cin, 3, 3, seed=2)
    want = _forward(x, w, stride, pad)
    assert tuple(want.shape[2:]) == CU.conv_out_hw(H, W, stride, pad)
    A = CU.conv_operand(x.permute(0, 2, 3, 1), stride=stride, pad=pad)
    assert A.dtype == torch.float64 and A.shape == (B * want.shape[2] * want.shape[3], 9 * Cin)
    lin, S = CU.conv_products(A, _pack_conv3x3(w, cin_pad=Cin))
    _same(lin, _nhwc_rows(want), "conv2d")
    _same(S, _nhwc_rows(_forward(x.abs(), w.abs(), stride, pad)), "conv2d of the magnitudes")


@pytest.mark.parametrize("B,H,W,Cin", [(2, 3, 5, 64), (1, 4, 3, 40), (1, 4, 4, 32)])
def test_fused_upsample_matches_interpolate_then_conv2d(B, H, W, Cin):
    x, w = _rand(B, Cin, H, W, seed=3), _rand(COUT, Cin, 3, 3, seed=4)
    want = F.conv2d(F.interpolate(x, scale_factor=2, mode="nearest"), w, padding=1)
    assert tuple(want.shape[2:]) == CU.conv_out_hw(H, W, upsample=1)
    A = CU.conv_operand(x.permute(0, 2, 3, 1), upsample=1)
    _same(CU.conv_products(A, _pack_conv3x3(w, cin_pad=Cin))[0], _nhwc_rows(want), "interpolate + conv2d")


# B, dY size, dX size, channels of dY, forward pad: the small and the tap-skip geometries (BM = 64) of the GPU tests, and odd sizes
DGRAD_FORMS = [(1, (3, 4), (6, 8), 64, 1), (1, (3, 4), (7, 9), 64, 0), (1, (3, 4), (6, 8), 40, 1), (1, (3, 4), (7, 9), 40, 0),
               (1, (3, 4), (5, 7), 8, 1), (2, (2, 3), (4, 6), 8, 0), (1, (2, 32), (4, 64), 64, 0), (1, (2, 48), (4, 96), 64, 0),
               (2, (1, 32), (3, 64), 64, 0), (1, (2, 32), (4, 64), 64, 1), (1, (2, 48), (4, 96), 64, 1)]


@pytest.mark.parametrize("B,dy_hw,dx_hw,C,pad", DGRAD_FORMS)
def test_stride2_input_gradient_matches_autograd(B, dy_hw, dx_hw, C, pad):
    """forward: x [B, COUT, dX size] -> y [B, C, dY size]; the gather form reads dY with the weight [COUT, 9 C] of the swapped channel roles"""
    x = _rand(B, COUT, *dx_hw, seed=5).requires_grad_(True)
    w, dy = _rand(C, COUT, 3, 3, seed=6), _rand(B, C, *dy_hw, seed=7)
    y = _forward(x, w, 2, pad)
    assert tuple(y.shape[2:]) == dy_hw
    y.backward(dy)
    A = CU.conv_operand(dy.permute(0, 2, 3, 1), pad=pad, upsample=2, out_hw=dx_hw)
    assert A.shape == (B * dx_hw[0] * dx_hw[1], 9 * C)
    _same(CU.conv_products(A, _pack_conv3x3(w.permute(1, 0, 2, 3), cin_pad=C))[0], _nhwc_rows(x.grad), "autograd input gradient")


@pytest.mark.parametrize("B,H,W,Cin", [(2, 3, 5, 64), (1, 4, 4, 32), (1, 5, 3, 64)])
def test_parity_form_matches_the_nine_tap_form(B, H, W, Cin):
    """weights that fp16 holds exactly: the packer sums at most four of them per slot in fp32, which is then exact too, so the parity
    form with the packed sums and the nine-tap form with the un-summed weights are the same float64 sums in another order"""
    x = _rand(B, Cin, H, W, seed=8)
    w = _rand(COUT, Cin, 3, 3, seed=9).half().double()
    xn = x.permute(0, 2, 3, 1)
    nine = CU.conv_products(CU.conv_operand(xn, upsample=1), _pack_conv3x3(w, cin_pad=Cin))[0]
    A = CU.conv_operand(xn, upsample=3)
    assert A.shape == (4 * B * H * W, 4 * Cin)
    rows = CU.parity_output_rows(B, H, W)
    assert sorted(rows.tolist()) == list(range(4 * B * H * W))
    wp = _pack_upsample_conv3x3(w)
    assert wp.shape == (4 * COUT, 4 * Cin) and wp.dtype == torch.float64
    _same(CU.conv_products(A, wp, upsample=3, rows=rows)[0], nine, "nine-tap form")
    _same(nine, _nhwc_rows(F.conv2d(F.interpolate(x, scale_factor=2, mode="nearest"), w, padding=1)), "interpolate + conv2d")
