"""Helpers of test_norm_edges_cpu.py / test_gpu_norm_edges.py: float64 references of the kernels of csrc/nn_ops.hip computed from the
operations' definitions on the fp16-rounded inputs, per-element error bounds, fp32 emulations of the kernels' arithmetic with their
mutations (CPU), and launches of the entries through ctypes on buffers the test owns (GPU).

Bounds.  u11 = 2^-11 (half an fp16 ulp, relative), u = u24 = 2^-24 (the same for fp32).  Every bound is  arith (1 + 2^-10) + rnd  with
rnd = max(u11 |ref|, 2^-25) the one rounding of the output to fp16 (2^-25: half a subnormal step) - the pair worst_ratio expects.

  sums         a sum of n fp32 terms in ANY order (threads, LDS atomics, partials, records, slices) is off by at most (n - 1) u sum|terms|
               to first order - adding a zero does not round.  |ds| <= n u sum|x|, |dq| <= (n + 1) u sum x^2 (the squares of fp16 numbers
               and the FMA that adds them are exact before the one rounding).
  moments      gn_moments: mu = s / n, m2 = q / n with inv_cnt = fl(1 / fl(hw cg)):  dmu = ds / n + 4 u |mu|;
               dvar = dq / n + 4 u m2 + [2 |mu| dmu + dmu^2 + 2 u (m2 + mu^2)]  - the bracket is the cancellation of the one-pass variance:
               the error of mu enters through mu^2, and mu^2 and the difference are rounded at the size of m2 and mu^2, not of var;
               v = var + eps: dv = dvar + u (v + dvar);  r = rsqrt(v): since max(var, 0) + eps >= eps in the kernel too,
               dr = [rsqrt(max(v - dv, eps (1 - 2 u))) - r] (1 + 2^-22) + 2^-22 r  (rsqrt is convex and decreasing: the lower end is the
               worse one; 2^-22 = 2 fp32 ulp for the hardware rsqrt; exact, not first order: dv may be a large part of v).
  GroupNorm    z = (x - mu) r gamma + beta as fma(x, a, b), a = fl(r gamma), b = fl(beta - fl(mu a)):
               dz = |gamma| dr |x - mu| + (|a| + da) dmu + 6 u (|a| |x| + |a| |mu| + |beta|), da = |gamma| dr + u |a|
               (six roundings at the size of the TERMS: a, mu a, the difference, the FMA, and for the SiLU argument the second folded pair
               -log2(e) a, -log2(e) b).  SiLU as gemm_bound's act == 1: 1.1 dz + 2^-20 |y| (1.0998 bounds sigma + |z| sigma' too, so the
               separately rounded exponent argument is covered).
  GN backward  with mu, r from the kernel's own fp32 statistics (ds = dq = 0, the roundings above remain): xh = fma(x, r, -mu r):
               dxh = |x - mu| dr + (r + dr) dmu + 3 u r (|x| + |mu|);  z = fma(xh, gamma, beta): dzz = |gamma| dxh + 2 u (|xh gamma| + |beta|);
               silu'(z) = s + z (s - s^2) in two FMAs (|silu''| <= 1/2): e_sg = dzz / 2 + 2^-21 (2 + |z|);  g = dy gamma silu'(z):
               dg = |dy gamma| e_sg + 2 u |g|;  S1 = sum g, S2 = sum g xh over the group:  d1 = sum dg + n u (sum|g| + sum dg),
               d2 = sum te + (n + 1) u (sum|g xh| + sum te), te = dg |xh| + |g| dxh + dg dxh;  m_i = S_i / n: dm_i = d_i / n + 4 u |m_i|;
               c_i = -m_i r: dc_i = r dm_i + |m_i| dr + dm_i dr + 2 u |c_i|;  G = gamma r: dG = |gamma| dr + u |G|;
               lin = fma(xh, c2, c1): dlin = |xh| dc2 + |c2| dxh + dxh dc2 + dc1 + 2 u (|xh c2| + |c1|);
               dx = fma(dy G, silu', lin) [+ dx_add, exact in fp32 before its one rounding u |dx|]:
               arith = |dy| dG |silu'| + (|dy G| + |dy| dG) e_sg + dlin + 2 u (|dy G silu'| + |lin|) + u |ref|.
  LayerNorm    two passes, no cancellation term: dmu = u sum|x| + 2 u |mu| (C terms / C);  d = x - mu, q = sum d^2:
               dq = 2 e sum|d| + C e^2 + (C + 3) u sum d^2 with e = dmu + u max|d|;  v = q / C + eps: dv = dq / C + 4 u v;  dr as above;
               arith = |gamma| (|d| dr + (r + dr) dmu) + 4 u (|d r gamma| + |beta|).
  softmax      p = e / sum e, e = __expf(fma(x, scale, -m)): the rounding of m is a common factor and cancels;  relative error of e_i:
               eps_i = (|x_i scale - m| + 2) 2^-22 (the argument's rounding grows with its size; two ulp for the exponential);  the sum
               over cols terms, the division and the product:  arith = p_i (eps_i + sum_j p_j eps_j + (cols + 3) u).
  softmax bwd  from the kernel's own fp16 p:  s = sum p dp (an FMA chain): dsum = (cols + 1) u sum|p dp|;
               arith = |scale p| (dsum + 4 u (|dp| + |s|)).
  GEGLU        y = a gelu(g), gelu(g) = g (1 + erf(g / sqrt 2)) / 2 with libm's erff (a few fp32 ulp: 2^-20 absolute on 1 + erf covers
               eight of them at |erf| <= 1 and the rounding of its argument):  arith = |a| (2^-21 |g| + 4 u |gelu(g)|).
  SiLU         arith = (2^-20 + 2^-23 |x|) |y|  (v_exp, v_rcp as above; the exponent argument -log2(e) x is rounded at its own size).
  timestep     a = t freq, freq = expf(-logf(10^4) k / half): |da| <= a (ln 10^4 + 4) 2^-23 (the exponent's argument carries three
               roundings at a size up to ln 10^4; expf, the product); cos and sin are 1-Lipschitz and a few ulp themselves:
               arith = da + 2^-22.
  concat, transpose, pad-cast, gather: bit-exact against torch indexing (pad-cast: torch's round-to-nearest-even fp32 -> fp16).

Mutation condition (test_norm_edges_cpu.py): at every shape of the GPU test an fp32 emulation of the kernel's arithmetic in two summation
orders stays within these bounds, and every mutation of it (a row, a chunk's last row, a slot, the last vector or the last record left out
of the statistics; a straddling slot with one group index; a wrong element count) exceeds them on at least one element."""
import ctypes as C
import math

import numpy as np
import torch

U11, U24 = 2.0 ** -11, 2.0 ** -24
RSQ = 2.0 ** -22
LN1E4 = math.log(10000.0)

GN_MAX_C, GN_FOLD_RECORDS = 4096, 96


def f32(v):
    """the value an entry receives for a float argument"""
    return float(np.float32(v))


def gn_stats_floats(batch):
    """ASD_GN_STATS_FLOATS(batch) of include/asd_hip.h"""
    return 64 * batch + 64 * (512 + batch)


def gn_stats_chunks(batch, hw):
    """(statistics blocks per batch element, rows per block) of asd_groupnorm_f16 / asd_groupnorm_bwd_f16"""
    chunks, cap = -(-hw // 16), -(-256 // batch)
    chunks = min(chunks, cap)
    return chunks, -(-hw // chunks)


def gn_ordered_chunks(hw):
    chunks = min(-(-hw // 64), 32)
    return chunks, -(-hw // chunks)


def gn_bwd_is_wide(batch, hw, c):
    """asd_groupnorm_bwd_f16's rule for its 512-thread statistics kernel: at least 64 KB of each tensor per block, slots that divide 512"""
    return gn_stats_chunks(batch, hw)[1] * c >= 32768 and c % 8 == 0 and 512 % (c // 8) == 0


def gn_record_slices(records, batch):
    """slices the apply entries sum more than GN_FOLD_RECORDS records in (0: the apply blocks sum the records themselves)"""
    return 0 if records <= GN_FOLD_RECORDS else min(-(-records // 32), 16, (512 + batch) // batch)


def _out(ref, arith):
    rnd = (U11 * ref.abs()).clamp_min(2.0 ** -25)
    return arith * (1 + 2.0 ** -10) + rnd, rnd


# ---- GroupNorm -----------------------------------------------------------------------------------------------------------------------
def gn_sums(x):
    """x [B, hw, C] -> float64 (s, q, ds, dq) [B, 32] and n: the group sums and what any fp32 summation order may be off by"""
    B, hw, Cn = x.shape
    xg = x.double().view(B, hw, 32, Cn // 32)
    n = hw * (Cn // 32)
    s, q, s1 = xg.sum((1, 3)), (xg * xg).sum((1, 3)), xg.abs().sum((1, 3))
    return s, q, n * U24 * s1, (n + 1) * U24 * q, n


def stats_pairs(stats, B):
    """the entries' [B, 64] statistics {sum, sum of squares} per group -> float64 (s, q) [B, 32]"""
    t = stats.double().view(B, 32, 2)
    return t[..., 0], t[..., 1]


def gn_moments(s, q, ds, dq, n, eps):
    """float64 (mu, r, dmu, dr) per (batch, group) from the sums and their errors"""
    eps = f32(eps)
    mu, m2 = s / n, q / n
    dmu = ds / n + 4 * U24 * mu.abs()
    dvar = dq / n + 4 * U24 * m2.abs() + 2 * mu.abs() * dmu + dmu * dmu + 2 * U24 * (m2.abs() + mu * mu)
    v = (m2 - mu * mu).clamp_min(0) + eps
    dv = dvar + U24 * (v + dvar)
    r = v.rsqrt()
    lo = torch.maximum(v - dv, torch.full_like(v, eps * (1 - 2 * U24)))
    return mu, r, dmu, (lo.rsqrt() - r) * (1 + RSQ) + RSQ * r


def _per_channel(t, cg):
    """[B, 32] -> [B, 1, C]"""
    return t.repeat_interleave(cg, 1)[:, None, :]


def silu64(z):
    return z * torch.sigmoid(z)


def silu_grad64(z):
    s = torch.sigmoid(z)
    return s * (1 + z * (1 - s))


def gn_forward_ref(x, gamma, beta, eps, silu, moments):
    """float64 reference and (bound, rnd) of GroupNorm(+SiLU) on x [B, hw, C] from moments = gn_moments(...)"""
    cg = x.shape[2] // 32
    mu, r, dmu, dr = (_per_channel(t, cg) for t in moments)
    xd, g, b = x.double(), gamma.double()[None, None], beta.double()[None, None]
    a = r * g
    z = (xd - mu) * a + b
    da = g.abs() * dr + U24 * a.abs()
    dz = g.abs() * dr * (xd - mu).abs() + (a.abs() + da) * dmu + 6 * U24 * (a.abs() * xd.abs() + a.abs() * mu.abs() + b.abs())
    if not silu:
        return z, _out(z, dz)
    y = silu64(z)
    return y, _out(y, 1.1 * dz + 2.0 ** -20 * y.abs())


def gn_backward_ref(x, dy, gamma, beta, eps, silu, fstats, dx_add=None, sums=None):
    """float64 reference, (bound, rnd) and the two reductions (S1, S2) of the GroupNorm(+SiLU) input gradient.  fstats: the forward statistics [B * 64] as the entry
    reads them (exact values: only the roundings of what follows count).  sums = (S1, S2, d1, d2) [B, 32]: the two reductions as the
    entry receives them (records) with their summation error; None: taken from x and dy."""
    B, hw, Cn = x.shape
    cg, n = Cn // 32, hw * (Cn // 32)
    s, q = stats_pairs(fstats, B)
    zero = torch.zeros_like(s)
    mu, r, dmu, dr = (_per_channel(t, cg) for t in gn_moments(s, q, zero, zero, n, eps))
    xd, dyd, g, b = x.double(), dy.double(), gamma.double()[None, None], beta.double()[None, None]
    xh = (xd - mu) * r
    dxh = (xd - mu).abs() * dr + (r + dr) * dmu + 3 * U24 * r * (xd.abs() + mu.abs())
    z = xh * g + b
    if silu:
        sg = silu_grad64(z)
        e_sg = 0.5 * (g.abs() * dxh + 2 * U24 * ((xh * g).abs() + b.abs())) + 2.0 ** -21 * (2 + z.abs())
    else:
        sg, e_sg = torch.ones_like(z), torch.zeros_like(z)
    gg = dyd * g * sg
    dg = (dyd * g).abs() * e_sg + 2 * U24 * gg.abs()
    te = dg * xh.abs() + gg.abs() * dxh + dg * dxh

    def grp(t):
        return t.view(B, hw, 32, cg).sum((1, 3))
    if sums is None:
        S1, S2 = grp(gg), grp(gg * xh)
        d1 = grp(dg) + n * U24 * (grp(gg.abs()) + grp(dg))
        d2 = grp(te) + (n + 1) * U24 * (grp((gg * xh).abs()) + grp(te))
    else:   # the element errors dg, te are the producer's, not this entry's
        S1, S2, d1, d2 = sums
    m1, m2, dm1, dm2 = S1 / n, S2 / n, d1 / n + 4 * U24 * (S1 / n).abs(), d2 / n + 4 * U24 * (S2 / n).abs()
    m1, m2, dm1, dm2 = (_per_channel(t, cg) for t in (m1, m2, dm1, dm2))
    c1, c2 = -m1 * r, -m2 * r
    dc1 = r * dm1 + m1.abs() * dr + dm1 * dr + 2 * U24 * c1.abs()
    dc2 = r * dm2 + m2.abs() * dr + dm2 * dr + 2 * U24 * c2.abs()
    G = g * r
    dG = g.abs() * dr + U24 * G.abs()
    lin = xh * c2 + c1
    dlin = xh.abs() * dc2 + c2.abs() * dxh + dxh * dc2 + dc1 + 2 * U24 * ((xh * c2).abs() + c1.abs())
    ref = dyd * G * sg + lin
    arith = dyd.abs() * dG * sg.abs() + ((dyd * G).abs() + dyd.abs() * dG) * e_sg + dlin + 2 * U24 * ((dyd * G * sg).abs() + lin.abs())
    if dx_add is not None:
        ref = ref + dx_add.double()
    return ref, _out(ref, arith + U24 * ref.abs()), (S1, S2)


def split_records(totals, n, seed):
    """[B, 64] float64 totals -> fp32 records [B, n, 64] whose float64 sum is close to the totals: random parts of either sign, with the
    first, the middle and the last record carrying a tenth each (a record left out at an edge of any trip shows)"""
    g = torch.Generator().manual_seed(seed)
    B = totals.shape[0]
    w = torch.randn(B, n, 64, generator=g, dtype=torch.float64)
    w = w - w.mean(1, keepdim=True)                       # sums to zero
    w = 0.5 * w / w.abs().sum(1, keepdim=True).clamp_min(1e-30) + (0.7 / n)
    for i in {0, n // 2, n - 1}:
        w[:, i] += 0.3 / len({0, n // 2, n - 1})
    return (totals.cpu()[:, None, :] * w).float()


def record_sums(records):
    """float64 (sum [B, 64], summation error bound [B, 64]) of fp32 records [B, n, 64]"""
    rd = records.double()
    return rd.sum(1), records.shape[1] * U24 * rd.abs().sum(1)


# ---- LayerNorm, softmax, element-wise ------------------------------------------------------------------------------------------------
def layernorm_ref(x, gamma, beta, eps):
    eps = f32(eps)
    xd, g, b = x.double(), gamma.double()[None], beta.double()[None]
    Cn = x.shape[1]
    mu = xd.mean(1, keepdim=True)
    dmu = U24 * xd.abs().sum(1, keepdim=True) + 2 * U24 * mu.abs()
    d = xd - mu
    e = dmu + U24 * d.abs().amax(1, keepdim=True)
    q = (d * d).sum(1, keepdim=True)
    dq = 2 * e * d.abs().sum(1, keepdim=True) + Cn * e * e + (Cn + 3) * U24 * q
    v = q / Cn + eps
    dv = dq / Cn + 4 * U24 * v
    r = v.rsqrt()
    lo = torch.maximum(v - dv, torch.full_like(v, eps * (1 - 2 * U24)))
    dr = (lo.rsqrt() - r) * (1 + RSQ) + RSQ * r
    ref = d * r * g + b
    arith = g.abs() * (d.abs() * dr + (r + dr) * dmu) + 4 * U24 * ((d * r * g).abs() + b.abs())
    return ref, _out(ref, arith)


def softmax_ref(x, scale):
    scale = f32(scale)
    t = x.double() * scale
    t = t - t.amax(1, keepdim=True)
    e = t.exp()
    p = e / e.sum(1, keepdim=True)
    eps_i = (t.abs() + 2) * 2.0 ** -22
    arith = p * (eps_i + (p * eps_i).sum(1, keepdim=True) + (x.shape[1] + 3) * U24)
    return p, _out(p, arith)


def softmax_bwd_ref(p, dp, scale):
    scale = f32(scale)
    pd, dd = p.double(), dp.double()
    s = (pd * dd).sum(1, keepdim=True)
    dsum = (p.shape[1] + 1) * U24 * (pd * dd).abs().sum(1, keepdim=True)
    ref = scale * pd * (dd - s)
    return ref, _out(ref, (scale * pd).abs() * (dsum + 4 * U24 * (dd.abs() + s.abs())))


def softmax_rows(rows, cols, scale, seed):
    """fp16 [rows, cols] with scale x in [-40, 40].  Row 0: everything in [-40, -30] but one element of the LAST vector at +60 - the
    other exponentials underflow, and a maximum taken without the last vector overflows (89.5 > ln of the largest float);
    row 1: the whole span with its maximum, +40, in the last vector; row 2: constant."""
    g = torch.Generator().manual_seed(seed)
    x = torch.empty(rows, cols, dtype=torch.float64)
    for r in range(rows):
        if r % 3 == 0:
            x[r] = -40 + 10 * torch.rand(cols, generator=g, dtype=torch.float64)
            x[r, cols - 3] = 60
        elif r % 3 == 1:
            x[r] = -40 + 79 * torch.rand(cols, generator=g, dtype=torch.float64)
            x[r, cols - 6] = 40
        else:
            x[r] = 17.0
    return (x / scale).half()


def geglu_ref(h):
    from_c = h.shape[1] // 2
    a, g = h[:, :from_c].double(), h[:, from_c:].double()
    gelu = 0.5 * g * (1 + torch.erf(g / math.sqrt(2.0)))
    ref = a * gelu
    return ref, _out(ref, a.abs() * (2.0 ** -21 * g.abs() + 4 * U24 * gelu.abs()))


def silu_ref(x):
    xd = x.double()
    y = silu64(xd)
    return y, _out(y, (2.0 ** -20 + 2.0 ** -23 * xd.abs()) * y.abs())


def timestep_ref(t, dim):
    """t fp32 [n] -> float64 [n, dim] (cos | sin), the bound"""
    half = dim // 2
    k = torch.arange(half, dtype=torch.float64, device=t.device)
    a = t.double()[:, None] * torch.exp(-LN1E4 * k / half)[None]
    ref = torch.cat([a.cos(), a.sin()], 1)
    da = a.abs() * (LN1E4 + 4) * 2.0 ** -23
    return ref, _out(ref, torch.cat([da, da], 1) + 2.0 ** -22)


# ---- fp32 emulations of the kernels' arithmetic and their mutations (CPU) ------------------------------------------------------------------
def _sum32(t, dim, order):
    """fp32 sum along dim: torch's blocked order, or strictly sequential from the far end"""
    return t.sum(dim) if order == 0 or t.shape[dim] == 0 else torch.cumsum(t.flip(dim), dim).select(dim, -1)


def emulate_gn_sums(x, rows_per_block, order, mutation=None):
    """fp32 [B, 32] (s, q) as the statistics pass forms them: per channel over the rows of a block, channels into groups, then blocks"""
    B, hw, Cn = x.shape
    cg, xs = Cn // 32, x.float()
    s_tot, q_tot = [], []
    for i, r0 in enumerate(range(0, hw, rows_per_block)):
        r1 = min(hw, r0 + rows_per_block)
        if mutation == "last_row_image" and r1 == hw:
            r1 -= 1
        if mutation == "last_row_chunk" and i == 0:
            r1 -= 1
        blk = xs[:, r0:r1]
        s, q = _sum32(blk, 1, order), _sum32(blk * blk, 1, order)              # [B, C]
        if mutation == "slot":
            c = (Cn // 8 // 2) * 8
            s[:, c:c + 8], q[:, c:c + 8] = 0, 0
        s_tot.append(_sum32(s.view(B, 32, cg), 2, order))
        q_tot.append(_sum32(q.view(B, 32, cg), 2, order))
    return _sum32(torch.stack(s_tot), 0, order), _sum32(torch.stack(q_tot), 0, order)


def emulate_gn_apply(x, gamma, beta, eps, silu, s, q, mutation=None):
    """fp32 apply pass from the sums: the folded scale and shift, the second folded pair of the SiLU argument, one rounding to fp16"""
    B, hw, Cn = x.shape
    cg = Cn // 32
    cnt = hw * {"cnt_plus": cg + 1, "cnt_minus": cg - 1}.get(mutation, cg)
    inv = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(cnt), dtype=torch.float32)
    mean = s * inv
    var = (q * inv - mean * mean).clamp_min(0)
    rstd = torch.rsqrt(var + torch.tensor(eps, dtype=torch.float32))
    ch = torch.arange(Cn)
    grp = (ch // 8 * 8 if mutation == "frozen_group" else ch) // cg
    xs, g, b = x.float(), gamma.float()[None, None], beta.float()[None, None]
    sa = rstd[:, grp][:, None, :] * g
    sb = b - mean[:, grp][:, None, :] * sa
    f = xs * sa + sb
    if silu:
        c = torch.tensor(-1.4426950408889634, dtype=torch.float32)
        f = f * (1 / (1 + torch.exp2(xs * (c * sa) + c * sb)))
    return f.half()


def emulate_layernorm(x, gamma, beta, eps, order, mutation=None):
    xs, Cn = x.float(), x.shape[1]
    live = xs[:, :Cn - 8] if mutation == "last_vector" else xs
    inv = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(Cn), dtype=torch.float32)
    mean = (_sum32(live, 1, order) * inv)[:, None]
    d = live - mean
    rstd = torch.rsqrt(_sum32(d * d, 1, order)[:, None] * inv + torch.tensor(eps, dtype=torch.float32))
    return ((xs - mean) * rstd * gamma.float()[None] + beta.float()[None]).half()


def emulate_softmax(x, scale, order, mutation=None):
    xs, cols = x.float(), x.shape[1]
    sc = torch.tensor(scale, dtype=torch.float32)
    seen = xs[:, :cols - 8] if mutation == "max_last_vector" else xs
    m = seen.amax(1, keepdim=True) if seen.shape[1] else torch.full((x.shape[0], 1), -math.inf)
    m = m * sc
    e = torch.exp(xs * sc - m)
    tot = _sum32(e[:, :cols - 8] if mutation == "sum_last_vector" else e, 1, order)[:, None]
    return (e * (1 / tot)).half()


def emulate_record_sum(records, order, mutation=None):
    r = records[:, :-1] if mutation == "last_record" else records
    return _sum32(r, 1, order) if r.shape[1] else torch.zeros(records.shape[0], 64)


# ---- GPU side ------------------------------------------------------------------------------------------------------------------------------
def poisoned_rows(t, ld, margin=64):
    """the fp16 matrix t with row stride ld >= its columns inside a NaN-filled allocation: the row gaps and `margin` halfs on either
    side are NaN"""
    rows, cols = t.shape
    assert t.dtype == torch.float16 and ld >= cols and ld % 8 == 0 and margin % 8 == 0
    buf = torch.full((rows * ld + 2 * margin,), float("nan"), dtype=torch.float16, device=t.device)
    view = buf[margin:margin + rows * ld].view(rows, ld)[:, :cols]
    view.copy_(t)
    assert view.data_ptr() % 16 == 0
    return view


class Flat16:
    """n fp16 values (n even) inside gemm_edge_util.GuardedFlat's sentinel band"""

    def __init__(self, *shape):
        from gemm_edge_util import GuardedFlat
        n = math.prod(shape)
        assert n % 2 == 0
        self.band = GuardedFlat(n // 2)
        self.view = self.band.view.view(torch.float16).view(*shape)

    def intact(self):
        return self.band.intact()

    def untouched(self):
        from gemm_edge_util import SENT32
        return bool(self.band.intact() & (self.band.view.view(torch.int32) == SENT32).all())


def _arg(a):
    if a is None:
        return C.c_void_p(0)
    if isinstance(a, torch.Tensor):
        return C.c_void_p(a.data_ptr())
    return a


def call(name, *args):
    """an entry of the library on the current stream (appended); tensors and None become pointers; returns (status, error text)"""
    from scaledreamer_amd._lib import lib, stream
    rc = getattr(lib(), name)(*[_arg(a) for a in args], stream())
    return rc, (lib().asd_last_error().decode() if rc else "")


i32, i64, fl = C.c_int32, C.c_int64, C.c_float


def groupnorm(x1, x2, c1, c2, B, hw, gamma, beta, eps, silu, y, stats):
    return call("asd_groupnorm_f16", x1, i32(c1), x2, i32(c2), i32(B), i32(hw), gamma, beta, fl(eps), i32(silu), y, stats)


def groupnorm_ordered(x, c, B, hw, gamma, beta, eps, silu, y, stats):
    return call("asd_groupnorm_ordered_f16", x, i32(c), i32(B), i32(hw), gamma, beta, fl(eps), i32(silu), y, stats)


def groupnorm_apply(x, c, B, hw, gamma, beta, eps, silu, records, n, y, stats):
    return call("asd_groupnorm_apply_f16", x, i32(c), i32(B), i32(hw), gamma, beta, fl(eps), i32(silu), records, i32(n), y, stats)


def groupnorm_bwd(x, dy, c, B, hw, gamma, beta, eps, silu, fstats, dx_add, dx, bstats):
    return call("asd_groupnorm_bwd_f16", x, dy, i32(c), i32(B), i32(hw), gamma, beta, fl(eps), i32(silu), fstats, dx_add, dx, bstats)


def groupnorm_bwd_apply(x, dy, c, B, hw, gamma, beta, eps, silu, fstats, records, n, dx_add, dx, scratch):
    return call("asd_groupnorm_bwd_apply_f16", x, dy, i32(c), i32(B), i32(hw), gamma, beta, fl(eps), i32(silu), fstats, records, i32(n), dx_add, dx,
                scratch)


# ---- the shapes of both tests ---------------------------------------------------------------------------------------------------------
# (B, hw, C): one row; fewer rows than rows in flight; 12 slots (256 % 12 != 0, 3 channels per group straddle slots); 5 channels per
# group; 120 slots, two rows in flight; 240 slots, one row in flight, 16 idle threads; exactly 256 slots; a second pass with 4 live slots;
# a second pass; the full second pass; hw around one apply trip of 4 x 64 rows; the chunk cap with a 1-row tail; statistics chunks capped
# at 37 of 28 rows, the last block without a row
GN_CASES = [(2, 1, 32), (1, 3, 64), (3, 77, 96), (2, 37, 160), (1, 130, 960), (2, 19, 1920), (1, 9, 2048), (1, 9, 2080), (2, 5, 2560),
            (1, 3, 4096), (1, 255, 32), (1, 256, 32), (1, 257, 32), (1, 4097, 32), (7, 1000, 32)]
GN_OFFSET_CASE = (2, 37, 160)          # batch 0, group 3 gets mean / std = 16
GN_PAIR_CASES = [(40, 24), (8, 88), (1280, 1280), (2048, 512)]     # (c1, c2) at hw = 5, batch 2
GN_ORDERED_EXTRA = [(2, 63, 64), (2, 64, 64), (2, 65, 64), (1, 2049, 32)]
GN_BWD_WIDE = [(1, 16, 2048), (1, 8, 4096), (32, 256, 1024)]
GN_RECORD_COUNTS = [1, 3, 4, 5, 31, 32, 33, 96, 97, 129, 511, 513, 8192]
GN_RECORD_SHAPES = [(2, 8, 64), (1, 5, 2560)]
LN_CS, LN_ROWS = [8, 504, 512, 520, 1024, 1032, 1536, 1544, 2040, 2048], [1, 3, 4, 5]
SM_COLS, SM_ROWS, SM_SCALE = [8, 2040, 2048, 2056, 4096, 4104, 8184, 8192], [1, 3], 0.125


def gn_inputs(B, hw, Cn, seed, offset_group=False):
    """fp16 CPU (x, gamma with mixed signs, beta)"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, hw, Cn, generator=g) * 1.5 + 0.3
    if offset_group:
        cg = Cn // 32
        x[0, :, 3 * cg:4 * cg] = 16 + torch.randn(hw, cg, generator=g)
    gamma, beta = torch.randn(Cn, generator=g), 0.5 * torch.randn(Cn, generator=g)
    return x.half(), gamma.half(), beta.half()
