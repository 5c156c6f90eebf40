"""GPU parity of every SiLU / silu' site of the diffusion side after the IEEE divisions left them: the three GroupNorm
streaming kernels at the VAE encoder's real tensor shapes, their saturation behaviour, the GEMM epilogue and the split-K reductions.
The bars are the existing ones: forward 4e-3 of max(|ref|, 1) as in test_groupnorm, input gradient 5e-3 max-relative as in
test_conv_dgrad_and_groupnorm_bwd_ops, GEMM 3e-3 as in test_gemm_bias_rowbias_residual_silu, the fused split-K GroupNorm 2e-3 absolute
against the stand-alone kernels and 4e-3 against torch as in test_groupnorm_applied_by_the_split_k_reduction."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

MAGNITUDES = (1.0, 10.0, 20.0, 90.0, 1e3, 6e4)


def _rand(*shape, scale=1.0, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).half().cuda()


def _close(got, want, tol, what=""):
    got, want = got.float(), want.float()
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite output"
    err = (got - want).abs().max().item()
    ref = want.abs().max().item()
    print(f"{what}: max abs err {err:.4g}, ref max {ref:.4g}, bar {tol * max(ref, 1.0):.4g}")
    assert err <= tol * max(ref, 1.0), f"{what}: max abs err {err} vs ref max {ref}"


def _max_rel(got, want, tol, what=""):
    got, want = got.double(), want.double()
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite output"
    rel = float((got - want).abs().max() / want.abs().max())
    print(f"{what}: max-relative err {rel:.4g}, bar {tol:.4g}")
    assert rel < tol, f"{what}: max-relative err {rel}"


def _torch_gn(x, gamma, beta, eps, silu, gy):
    """fp32 GroupNorm(32)(+SiLU) of the fp16-rounded inputs and its autograd input gradient for the upstream gradient gy"""
    xr = x.float().requires_grad_(True)
    ref = F.group_norm(xr.permute(0, 2, 1), 32, gamma.float(), beta.float(), eps).permute(0, 2, 1)
    ref = F.silu(ref) if silu else ref
    ref.backward(gy.float())
    return ref.detach(), xr.grad


@pytest.mark.parametrize("silu", [True, False])
@pytest.mark.parametrize("B,HW,C", [(1, 512 * 512, 128), (1, 256 * 256, 256), (1, 128 * 128, 512)])
def test_groupnorm_fwd_and_input_gradient_at_the_vae_shapes(B, HW, C, silu):
    from scaledreamer_amd.diffusion import hip_ops as H

    x = _rand(B, HW, C, scale=2.0, seed=31) + 0.3
    gamma, beta = _rand(C, seed=32) * 0.1 + 1, _rand(C, seed=33) * 0.1
    gy, extra = _rand(B, HW, C, seed=34), _rand(B, HW, C, seed=35)
    ref, gref = _torch_gn(x, gamma, beta, 1e-6, silu, gy)
    y, stats = H.groupnorm(x, gamma, beta, 1e-6, silu, return_stats=True)
    _close(y, ref, 4e-3, f"forward {HW}x{C} silu={silu}")
    _max_rel(H.groupnorm_bwd(x, gy, gamma, beta, 1e-6, silu, stats), gref, 5e-3, f"dx {HW}x{C} silu={silu}")
    _max_rel(H.groupnorm_bwd(x, gy, gamma, beta, 1e-6, silu, stats, dx_add=extra), gref + extra.float(), 5e-3, f"dx + dx_add {HW}x{C} silu={silu}")


def _saturating_case(B, HW, C, seed):
    """x, gamma, dy such that in group g the normalised z = xhat * gamma spans [-M, M] with M = MAGNITUDES[g % 6] (the sign of gamma
    alternates per channel), and dy ~ 4 / M so that the gradient stays inside fp16"""
    x = torch.clamp(_rand(B, HW, C, seed=seed), -2.0, 2.0)
    cg = C // 32
    xg = x.double().view(B, HW, 32, cg)
    xhat_max = ((xg - xg.mean((1, 3), keepdim=True)) / xg.std((1, 3), unbiased=False, keepdim=True)).abs().amax((0, 1, 3))   # [32]
    mag = torch.tensor([MAGNITUDES[g % len(MAGNITUDES)] for g in range(32)], device="cuda", dtype=torch.float64)
    sign = torch.tensor([1.0, -1.0], device="cuda", dtype=torch.float64).repeat(C // 2)
    gamma = ((0.98 * mag / xhat_max).repeat_interleave(cg) * sign).half()
    beta = torch.zeros(C, dtype=torch.float16, device="cuda")
    dy = (_rand(B, HW, C, seed=seed + 1).float() * (4.0 / mag.float()).repeat_interleave(cg)).half()
    return x, gamma, beta, dy, mag


def test_groupnorm_silu_saturation():
    """z from -6e4 to 6e4: exp2 overflows to +inf and rcp(inf) = 0 on the negative side, exp2 underflows to 0 on the positive side —
    outputs finite, silu -> -0 / z and silu' -> 0 / 1, every magnitude class held to the bars on its own channels"""
    from scaledreamer_amd.diffusion import hip_ops as H

    B, HW, C = 2, 1024, 256
    cg = C // 32
    x, gamma, beta, dy, mag = _saturating_case(B, HW, C, seed=41)
    extra = _rand(B, HW, C, seed=43)
    ref, gref = _torch_gn(x, gamma, beta, 1e-6, True, dy)
    z = F.group_norm(x.float().permute(0, 2, 1), 32, gamma.float(), beta.float(), 1e-6).permute(0, 2, 1)
    y, stats = H.groupnorm(x, gamma, beta, 1e-6, True, return_stats=True)
    dx = H.groupnorm_bwd(x, dy, gamma, beta, 1e-6, True, stats)
    dxa = H.groupnorm_bwd(x, dy, gamma, beta, 1e-6, True, stats, dx_add=extra)
    for i, m in enumerate(MAGNITUDES):
        ch = torch.cat([torch.arange(g * cg, (g + 1) * cg) for g in range(32) if g % len(MAGNITUDES) == i]).cuda()
        assert 0.9 * m < float(z[..., ch].abs().max()) <= m      # the class does reach its magnitude, on both sides of 0
        assert float(z[..., ch].min()) < -0.8 * m and float(z[..., ch].max()) > 0.8 * m
        _close(y[..., ch], ref[..., ch], 4e-3, f"silu(z), |z| <= {m:g}")
        _max_rel(dx[..., ch], gref[..., ch], 5e-3, f"dx, |z| <= {m:g}")
        _max_rel(dxa[..., ch], gref[..., ch] + extra[..., ch].float(), 5e-3, f"dx + dx_add, |z| <= {m:g}")
    # the element-wise kernel on the magnitudes themselves
    v = torch.tensor([s * m for m in MAGNITUDES for s in (1.0, -1.0)] * 8, device="cuda").half()
    got, want = H.silu(v).float(), F.silu(v.float())
    assert bool(torch.isfinite(got).all())
    assert bool(((got - want).abs() <= 3e-3 * want.abs().clamp(min=1.0)).all()), (got, want)
    assert bool((got[v < -20] == 0).all()) and bool((got[v > 20] == v.float()[v > 20]).all())


def test_gemm_epilogue_silu_and_split_k_reductions():
    from scaledreamer_amd.diffusion import hip_ops as H

    M, N, K = 5120, 640, 1280
    a, w = _rand(M, K, seed=1), _rand(N, K, scale=K ** -0.5, seed=2)
    bias, res, rb = _rand(N, seed=3), _rand(M, N, seed=4), _rand(5, N, seed=5)
    ref = F.silu(a.float() @ w.float().T + bias.float() + rb.float().repeat_interleave(M // 5, 0)) + res.float()
    kw = dict(bias=bias, row_bias=rb, rows_per_group=M // 5, residual=res, act=1)
    _close(H.gemm(a, w, **kw), ref, 3e-3, "gemm epilogue act=1")
    _close(H.gemm(a, w, split_k=3, **kw), ref, 3e-3, "split-K reduction act=1")
    # the reduction that applies GroupNorm + SiLU for its consumer
    B, hw, cin, cout, split = 5, 8, 128, 1280, 4
    rows = hw * hw
    bias, res, temb = _rand(cout, seed=3), _rand(B * rows, cout, seed=4), _rand(B, cout, seed=9)
    gamma, beta = (_rand(cout, seed=5) * 0.1 + 1).half(), (_rand(cout, seed=6) * 0.1).half()
    x = _rand(B, hw, hw, cin, seed=1)
    wt = H.pack_conv3x3_weight(_rand(cout, cin, 3, 3, scale=(9 * cin) ** -0.5, seed=2))
    c, y, st = H.conv3x3(x, wt, gn_rows=rows, gn_apply=dict(gamma=gamma, beta=beta, eps=1e-5, silu=True), bias=bias, residual=res,
                         row_bias=temb, rows_per_group=rows, tile_cfg=13, split_k=split)
    assert y is not None and st is not None
    cv = c.view(B, rows, cout)
    want = H.groupnorm(cv, gamma, beta, 1e-5, True)
    assert float((y.view_as(want).float() - want.float()).abs().max()) <= 2e-3
    ref = F.silu(F.group_norm(cv.float().permute(0, 2, 1), 32, gamma.float(), beta.float(), 1e-5).permute(0, 2, 1))
    _close(y.view(B, rows, cout), ref, 4e-3, "split-K GroupNorm + SiLU reduction")
