"""The guidance forward driven through the bare C ABI (include/asd_hip.h: asd_unet_*, asd_vae_enc_*) with nothing but ctypes and
device buffers — what a non-Python host would do: create -> read the weight table -> bind -> workspace -> fwd (-> bwd)."""
import ctypes as C
import os
import zlib

import numpy as np
import pytest
import torch

from golden_util import GOLDEN_DIR

pytestmark = pytest.mark.gpu


def rnd(name, shape, seed=0):
    g = torch.Generator().manual_seed((seed * 1_000_003 + zlib.crc32(name.encode())) & 0x7FFFFFFF)
    return torch.randn(shape, generator=g)


def _rel(got, ref):
    got, ref = got.double().cpu(), ref.double().cpu()
    return float((got - ref).norm() / ref.norm()), float((got - ref).abs().max() / ref.abs().max())


def _bind(lib, kind, h, packed):
    from scaledreamer_amd._lib import WeightInfo, check, i32

    n = getattr(lib, f"asd_{kind}_num_weights")(h)
    info, keep, ptrs = WeightInfo(), [], (C.c_void_p * n)()
    for i in range(n):
        check(getattr(lib, f"asd_{kind}_weight_info")(h, i32(i), C.byref(info)))
        t = packed[info.name.decode()].to(device="cuda", dtype=torch.float16).contiguous()
        assert t.numel() == info.rows * info.cols
        keep.append(t)
        ptrs[i] = t.data_ptr()
    check(getattr(lib, f"asd_{kind}_bind_weights")(h, ptrs, i32(n)))
    return keep


def test_asd_unet_fwd_through_ctypes_matches_the_reference_golden():
    from scaledreamer_amd._lib import check, i32, lib
    from scaledreamer_amd.diffusion import weights as W
    from scaledreamer_amd.diffusion.engine import unet_desc

    l = lib()
    g = dict(np.load(os.path.join(GOLDEN_DIR, "diffusion_unet_small.npz")))       # reference UNetModel, reduced width (head_dim 32 -> use the 64 one)
    cfg = W.UNetConfig(model_channels=128, num_head_channels=64, context_dim=128)
    from oracle import diffusion_ref as D

    layout = W.unet_layout(cfg)
    p = W.gen_params(layout[0], seed=21)
    B, hw, n_ctx = 3, 32, 77
    x, ctx, t = rnd("in.x", (B, 4, hw, hw), 21), rnd("in.context", (B, n_ctx, 128), 21), torch.tensor([815.0, 20.0, 999.0])
    with torch.no_grad():
        ref = D.unet_forward(p, layout, cfg, x, t, ctx)
    h = C.c_void_p()
    check(l.asd_unet_create(C.byref(unet_desc(cfg)), C.byref(h)))
    keep = _bind(l, "unet", h, W.pack_unet(p, cfg))
    ctx_stride = (n_ctx + 7) // 8 * 8
    xin = torch.zeros(B, hw, hw, 32, device="cuda", dtype=torch.float16)
    xin[..., :4] = x.permute(0, 2, 3, 1)
    cin = torch.zeros(B, ctx_stride, 128, device="cuda", dtype=torch.float16)
    cin[:, :n_ctx] = ctx
    tin, eps = t.cuda(), torch.empty(B, hw, hw, 4, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for tune in (1, 0):       # first call times the GEMM shapes that have no plan, second runs on the recorded plans
        nb = l.asd_unet_workspace_bytes(h, i32(B), i32(hw), i32(hw), i32(n_ctx), i32(1), i32(tune))
        assert nb > 0
        ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
        check(l.asd_unet_fwd(h, C.c_void_p(xin.data_ptr()), C.c_void_p(tin.data_ptr()), C.c_void_p(cin.data_ptr()), None, i32(B), i32(hw), i32(hw),
                             i32(n_ctx), i32(1), C.c_void_p(ws.data_ptr()), C.c_int64(nb), C.c_void_p(eps.data_ptr()), i32(tune), st))
        l2, mx = _rel(eps.permute(0, 3, 1, 2), ref)
        assert l2 < 1e-2 and mx < 1e-2, (tune, l2, mx)
    # error behaviour: too small a workspace, camera passed to a UNet without camera conditioning
    assert l.asd_unet_fwd(h, C.c_void_p(xin.data_ptr()), C.c_void_p(tin.data_ptr()), C.c_void_p(cin.data_ptr()), None, i32(B), i32(hw), i32(hw), i32(n_ctx),
                          i32(1), C.c_void_p(ws.data_ptr()), C.c_int64(1024), C.c_void_p(eps.data_ptr()), i32(0), st) != 0
    assert b"too small" in l.asd_last_error()
    assert l.asd_unet_fwd(h, C.c_void_p(xin.data_ptr()), C.c_void_p(tin.data_ptr()), C.c_void_p(cin.data_ptr()), C.c_void_p(cin.data_ptr()), i32(B), i32(hw),
                          i32(hw), i32(n_ctx), i32(1), C.c_void_p(ws.data_ptr()), C.c_int64(nb), C.c_void_p(eps.data_ptr()), i32(0), st) != 0
    torch.cuda.synchronize()
    l.asd_unet_destroy(h)
    del keep, g


def test_asd_vae_enc_fwd_bwd_through_ctypes_matches_the_reference_golden():
    from scaledreamer_amd._lib import check, i32, lib
    from scaledreamer_amd.diffusion import weights as W
    from scaledreamer_amd.diffusion.vae_hip import vae_desc

    l = lib()
    g = dict(np.load(os.path.join(GOLDEN_DIR, "diffusion_vae_small.npz")))
    ch, nrb, zc = (int(v) for v in g["cfg"])
    cfg = W.VAEConfig(ch=ch, num_res_blocks=nrb, z_channels=zc, ch_mult=tuple(int(v) for v in g["ch_mult"]))
    seed, B, res = int(g["seed"]), int(g["batch"]), int(g["res"])
    h = C.c_void_p()
    check(l.asd_vae_enc_create(C.byref(vae_desc(cfg)), C.byref(h)))
    keep = _bind(l, "vae_enc", h, W.pack_vae_encoder(W.gen_params(W.vae_encoder_layout(cfg)[0], seed), cfg))
    img = torch.tanh(rnd("in.img", (B, 3, res, res), seed))
    x = torch.zeros(B, res, res, 32, device="cuda", dtype=torch.float16)
    x[..., :3] = img.permute(0, 2, 3, 1)
    gm = rnd("in.gmoments", (B, 8, res // 8, res // 8), seed).permute(0, 2, 3, 1).contiguous().cuda()
    m = torch.empty(B, res // 8, res // 8, 8, device="cuda")
    dx = torch.empty(B, res, res, 32, device="cuda", dtype=torch.float16)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for tune in (1, 0):
        nb = l.asd_vae_enc_workspace_bytes(h, i32(B), i32(res), i32(res), i32(tune))
        ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
        assert l.asd_vae_enc_bwd(h, C.c_void_p(gm.data_ptr()), i32(B), i32(res), i32(res), C.c_void_p(ws.data_ptr()), C.c_int64(nb),
                                 C.c_void_p(dx.data_ptr()), i32(tune), st) != 0          # no forward has run on this workspace yet
        check(l.asd_vae_enc_fwd(h, C.c_void_p(x.data_ptr()), i32(B), i32(res), i32(res), C.c_void_p(ws.data_ptr()), C.c_int64(nb),
                                C.c_void_p(m.data_ptr()), i32(tune), st))
        check(l.asd_vae_enc_bwd(h, C.c_void_p(gm.data_ptr()), i32(B), i32(res), i32(res), C.c_void_p(ws.data_ptr()), C.c_int64(nb),
                                C.c_void_p(dx.data_ptr()), i32(tune), st))
        l2, mx = _rel(m.permute(0, 3, 1, 2), torch.from_numpy(g["moments"]))
        assert l2 < 1e-2 and mx < 1e-2, (tune, l2, mx)
        l2, mx = _rel(dx[..., :3].permute(0, 3, 1, 2), torch.from_numpy(g["grad_x_sub"]))
        assert l2 < 1e-2 and mx < 1e-2, (tune, l2, mx)
        assert float(dx[..., 3:].abs().max()) == 0.0                                      # gradient of the zero padding channels
    torch.cuda.synchronize()
    l.asd_vae_enc_destroy(h)
    del keep


class _VaeSmall:
    """The diffusion_vae_small golden's encoder behind the C ABI, with its inputs on the device and one workspace per call of ws()."""

    def __init__(self):
        from scaledreamer_amd._lib import check, lib
        from scaledreamer_amd.diffusion import weights as W
        from scaledreamer_amd.diffusion.vae_hip import vae_desc

        self.l = lib()
        g = dict(np.load(os.path.join(GOLDEN_DIR, "diffusion_vae_small.npz")))
        ch, nrb, zc = (int(v) for v in g["cfg"])
        self.cfg = W.VAEConfig(ch=ch, num_res_blocks=nrb, z_channels=zc, ch_mult=tuple(int(v) for v in g["ch_mult"]))
        seed, self.B, self.res = int(g["seed"]), int(g["batch"]), int(g["res"])
        self.h = C.c_void_p()
        check(self.l.asd_vae_enc_create(C.byref(vae_desc(self.cfg)), C.byref(self.h)))
        self.keep = _bind(self.l, "vae_enc", self.h, W.pack_vae_encoder(W.gen_params(W.vae_encoder_layout(self.cfg)[0], seed), self.cfg))
        img = torch.tanh(rnd("in.img", (self.B, 3, self.res, self.res), seed))
        self.x = torch.zeros(self.B, self.res, self.res, 32, device="cuda", dtype=torch.float16)
        self.x[..., :3] = img.permute(0, 2, 3, 1)
        self.gm = rnd("in.gmoments", (self.B, 8, self.res // 8, self.res // 8), seed).permute(0, 2, 3, 1).contiguous().cuda()
        self.moments, self.grad = torch.from_numpy(g["moments"]), torch.from_numpy(g["grad_x_sub"])
        self.st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def ws(self, B, tune=0):
        from scaledreamer_amd._lib import i32

        nb = self.l.asd_vae_enc_workspace_bytes(self.h, i32(B), i32(self.res), i32(self.res), i32(tune))
        assert nb > 0
        return torch.empty(nb, dtype=torch.uint8, device="cuda")

    def fwd(self, ws, B, tune=0):
        from scaledreamer_amd._lib import i32

        m = torch.empty(B, self.res // 8, self.res // 8, 8, device="cuda")
        st = self.l.asd_vae_enc_fwd(self.h, C.c_void_p(self.x.data_ptr()), i32(B), i32(self.res), i32(self.res), C.c_void_p(ws.data_ptr()),
                                    C.c_int64(ws.numel()), C.c_void_p(m.data_ptr()), i32(tune), self.st)
        return st, m

    def bwd(self, ws, B, tune=0, res=None, dx=None):
        from scaledreamer_amd._lib import i32

        res = self.res if res is None else res
        if dx is None:
            dx = torch.empty(B, res, res, 32, device="cuda", dtype=torch.float16)
        st = self.l.asd_vae_enc_bwd(self.h, C.c_void_p(self.gm.data_ptr()), i32(B), i32(res), i32(res), C.c_void_p(ws.data_ptr()),
                                    C.c_int64(ws.numel()), C.c_void_p(dx.data_ptr()), i32(tune), self.st)
        return st, dx

    def check(self, m, dx, B, tag):
        """the bound of the golden test above, on the first B images (a batch item's moments and gradient do not depend on the others)"""
        for got, ref, what in ((m.permute(0, 3, 1, 2), self.moments[:B], "moments"), (dx[..., :3].permute(0, 3, 1, 2), self.grad[:B], "grad")):
            l2, mx = _rel(got, ref)
            print(f"{tag} {what} B={B}: l2 {l2:.3e} max {mx:.3e}")
            assert l2 < 1e-2 and mx < 1e-2, (tag, what, l2, mx)
        assert float(dx[..., 3:].abs().max()) == 0.0                                          # gradient of the zero padding channels

    def tuned(self):
        """every GEMM shape of the golden's batch has a recorded plan (nothing is timed when an earlier test already did)"""
        ws = self.ws(self.B, 1)
        assert self.fwd(ws, self.B, 1)[0] == 0 and self.bwd(ws, self.B, 1)[0] == 0
        torch.cuda.synchronize()

    def close(self):
        torch.cuda.synchronize()
        self.l.asd_vae_enc_destroy(self.h)


def test_asd_vae_enc_two_workspaces_interleaved():
    """One handle, two workspaces with different layouts (the golden's batch, and its first image alone): fwd A, fwd B, bwd A, bwd B.
    Each backward reads the layout ITS forward recorded for its workspace."""
    v = _VaeSmall()
    wa, wb = v.ws(v.B), v.ws(1)
    sa, ma = v.fwd(wa, v.B)
    sb, mb = v.fwd(wb, 1)
    assert sa == 0 and sb == 0
    sa, da = v.bwd(wa, v.B)
    sb, db = v.bwd(wb, 1)
    assert sa == 0 and sb == 0, v.l.asd_last_error()
    v.check(ma, da, v.B, "A")
    v.check(mb, db, 1, "B")
    v.close()


def test_asd_vae_enc_bwd_after_the_plan_table_changed():
    """A plan of one of the forward's convolution shapes changes between forward and backward (another split-K: the record count a second
    walk of the forward would allocate differs, and the plan generation moves).  The backward runs on the recorded layout."""
    from scaledreamer_amd._lib import GemmArgs, check, i32

    v = _VaeSmall()
    v.tuned()
    l, B, res = v.l, v.B, v.res
    # forward-only shapes: the stride-2 Downsample convolutions (their input gradient is the parity-form launch, another plan key)
    keys, c, hw = [], v.cfg.ch, res
    for mult in v.cfg.ch_mult[:-1]:
        c = v.cfg.ch * mult
        keys.append((B * (hw // 2) ** 2, c, 9 * c, 1, hw, c, 2, 0, 0))
        hw //= 2
    plans, buf = {}, (C.c_int32 * 11)()
    for i in range(l.asd_gemm_plan_count()):
        check(l.asd_gemm_plan_entry(i32(i), buf))
        plans[tuple(buf[:9])] = (buf[9], buf[10])

    def records(key):
        a = GemmArgs()
        a.M, a.N, a.K, a.conv, a.Hin, a.Cin, a.stride, a.upsample, a.pad = key
        a.Win, a.Hout, a.Wout, a.ldw, a.ldc = a.Hin, a.Hin // 2, a.Hin // 2, a.K, a.N
        a.gn_rows, a.gn_cg = a.Hout * a.Wout, a.N // 32
        return l.asd_gemm_gn_records(C.byref(a))

    ws = v.ws(B)
    st, m = v.fwd(ws, B)
    assert st == 0
    changed = None
    for key in keys:
        assert key in plans, ("the tuning pass recorded no plan for", key)
        tile, split = plans[key]
        before, gen = records(key), l.asd_gemm_plan_generation()
        check(l.asd_gemm_plan_set(*[i32(k) for k in key], i32(tile), i32(2 if split == 1 else 1)))
        if records(key) != before and l.asd_gemm_plan_generation() != gen:
            changed = (key, tile, split)
            break
        check(l.asd_gemm_plan_set(*[i32(k) for k in key], i32(tile), i32(split)))
    assert changed is not None, "no Downsample shape whose record count depends on its split-K"
    try:
        st, dx = v.bwd(ws, B)
        assert st == 0, l.asd_last_error()
        v.check(m, dx, B, "plan changed")
    finally:
        key, tile, split = changed
        torch.cuda.synchronize()
        check(l.asd_gemm_plan_set(*[i32(k) for k in key], i32(tile), i32(split)))
    v.close()


def test_asd_vae_enc_bwd_refuses_another_shape_than_its_forward():
    v = _VaeSmall()
    l, B, res = v.l, v.B, v.res
    ws = v.ws(B)
    fresh = v.ws(B)
    st, m = v.fwd(ws, B)
    assert st == 0
    for bad_b, bad_res in ((B + 1, res), (B, res // 2)):
        dx = torch.full((bad_b, bad_res, bad_res, 32), 7.0, device="cuda", dtype=torch.float16)
        st = l.asd_vae_enc_bwd(v.h, C.c_void_p(v.gm.data_ptr()), C.c_int32(bad_b), C.c_int32(bad_res), C.c_int32(bad_res), C.c_void_p(ws.data_ptr()),
                               C.c_int64(ws.numel()), C.c_void_p(dx.data_ptr()), C.c_int32(0), v.st)
        err = l.asd_last_error()
        assert st != 0
        assert f"{bad_b} x {bad_res} x {bad_res}".encode() in err and f"{B} x {res} x {res}".encode() in err, err
        torch.cuda.synchronize()
        assert bool((dx == 7.0).all())                                                        # nothing was launched
    assert v.bwd(fresh, B)[0] != 0 and b"no forward pass" in l.asd_last_error()               # a workspace no forward has run on
    st, dx1 = v.bwd(ws, B)
    assert st == 0, l.asd_last_error()
    st, dx2 = v.bwd(ws, B)                                                                    # again, as under retain_graph
    assert st == 0, l.asd_last_error()
    v.check(m, dx1, B, "first")
    v.check(m, dx2, B, "second")
    v.close()
