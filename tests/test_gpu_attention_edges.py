"""asd_attention_f16 at the edges of its two forms — the wide one (256 queries per block, lq and lk >= 2048) at the smallest sizes that
dispatch it, with a masked last key tile, a ragged last query block and keys beyond lk_stride; the narrow one below one key tile and
below one query fragment — every output element against float64 softmax attention over the first lk keys of each batch element:

    |got - ref| <= 4 * 2^-11 * (P |v|) + 2^-24 * (sum_j |v_j|) / L,      P the float64 probabilities, L = sum_j exp(s_j - max s)

(fp16 rounding of each probability, the normaliser summed from the same rounded values, the output rounding and fp32 accumulation over
<= 4096 keys; the second term is for probabilities that fall into fp16's subnormal range when the maximum arrives late).  Rows lk ..
lk_stride of K and the matching columns of V^T hold +-60000 alternating: the mask must remove them entirely."""
import ctypes as C
import math

import pytest
import torch

from gemm_edge_util import Guarded, rand16

pytestmark = pytest.mark.gpu

WIDE = [(1, 2, 2048, 2048, 2048), (1, 2, 2049, 2048, 2048), (1, 2, 2148, 2112, 2112), (1, 2, 2048, 2049, 2056), (1, 2, 2304, 2088, 2088),
        (1, 2, 2100, 2111, 2112), (2, 2, 2049, 2049, 2056)]
NARROW = [(2, 3, lq, lk, lks) for lq in (1, 15, 16, 129) for lk, lks in ((1, 8), (8, 8), (63, 64), (64, 64), (65, 72), (77, 80))]


def _inputs(B, heads, lq, lk, lks, seed):
    """q [B lq, C], k [B lks, C], v [B lks, C] fp16; the padding rows lk .. lks of k and v are +-60000 alternating"""
    C_ = heads * 64
    q, k, v = rand16(B * lq, C_, seed=seed), rand16(B * lks, C_, seed=seed + 1), rand16(B * lks, C_, seed=seed + 2)
    if lks > lk:
        sign = 1.0 - 2.0 * ((torch.arange(lks - lk, device="cuda")[:, None] + torch.arange(C_, device="cuda")[None, :]) % 2)
        pad = (60000.0 * sign).half()
        k.view(B, lks, C_)[:, lk:] = pad
        v.view(B, lks, C_)[:, lk:] = pad
    return q, k, v


def _ref_and_bound(q, k, v, B, heads, lq, lk, lks):
    qd = q.double().view(B, lq, heads, 64).transpose(1, 2)
    kd = k.double().view(B, lks, heads, 64)[:, :lk].transpose(1, 2)
    vd = v.double().view(B, lks, heads, 64)[:, :lk].transpose(1, 2)
    s = qd @ kd.transpose(-1, -2) * 64 ** -0.5
    e = torch.exp(s - s.amax(-1, keepdim=True))
    L = e.sum(-1, keepdim=True)
    P = e / L
    ref = P @ vd
    bound = 4 * 2.0 ** -11 * (P @ vd.abs()) + 2.0 ** -24 * vd.abs().sum(-2, keepdim=True) / L
    back = lambda t: t.transpose(1, 2).reshape(B * lq, heads * 64)
    return back(ref), back(bound)


def _check(got, ref, bound, what):
    err = (got.double() - ref).abs()
    ratio = float(torch.nan_to_num(err / bound, nan=math.inf).max())
    print(f"attention {what}: worst err/bound {ratio:.3f}")
    assert ratio <= 1.0, f"attention {what}: err/bound {ratio}"


@pytest.mark.parametrize("B,heads,lq,lk,lks", WIDE + NARROW)
def test_attention_edge_shapes(B, heads, lq, lk, lks):
    from scaledreamer_amd.diffusion import hip_ops as H

    q, k, v = _inputs(B, heads, lq, lk, lks, seed=40)
    got = H.attention(q, k, v.t().contiguous(), B, heads, lq, lk, lks)
    ref, bound = _ref_and_bound(q, k, v, B, heads, lq, lk, lks)
    _check(got, ref, bound, f"B{B} h{heads} lq{lq} lk{lk} stride{lks}")


@pytest.mark.parametrize("B,heads,lq,lk,lks", [(1, 2, 2100, 2111, 2112), (2, 3, 129, 77, 80)])
def test_attention_strided_operands_and_output_guard(B, heads, lq, lk, lks):
    """one case per form through the C entry: q and k are column slices of wider matrices (ldq, ldk > heads * 64), o lies inside a
    sentinel-filled buffer with ldo > heads * 64: the ragged last query block writes nothing beyond row B lq - 1, nothing beside the rows"""
    from scaledreamer_amd._lib import check, f32, i32, lib, stream
    from scaledreamer_amd.diffusion import hip_ops as H

    C_ = heads * 64
    q, k, v = _inputs(B, heads, lq, lk, lks, seed=50)
    qw, kw = rand16(B * lq, 3 * C_, seed=53), rand16(B * lks, 2 * C_ + 8, seed=54)
    qw[:, C_:2 * C_] = q
    kw[:, 8:8 + C_] = k
    qs, ks, vT = qw[:, C_:2 * C_], kw[:, 8:8 + C_], v.t().contiguous()
    o = Guarded(B * lq, C_)
    assert o.view.stride(0) > C_
    check(lib().asd_attention_f16(C.c_void_p(qs.data_ptr()), i32(qs.stride(0)), C.c_void_p(ks.data_ptr()), i32(ks.stride(0)),
                                  C.c_void_p(vT.data_ptr()), i32(vT.stride(0)), C.c_void_p(o.view.data_ptr()), i32(o.view.stride(0)), i32(B), i32(heads),
                                  i32(lq), i32(lk), i32(lks), f32(64 ** -0.5), C.c_void_p(H.zero_page(q.device).data_ptr()), stream()))
    assert bool(o.intact()), "attention wrote outside its [B lq, heads 64] output"
    ref, bound = _ref_and_bound(q, k, v, B, heads, lq, lk, lks)
    _check(o.view, ref, bound, f"strided B{B} h{heads} lq{lq} lk{lk} stride{lks}")
