"""Memory-safety and determinism evidence for the C ABI (the reference relies on compute-sanitizer / TORCH_USE_CUDA_DSA for
its third-party kernels; neither exists for gfx950 in this image).  (1) Guard bands: the entry points that own a whole pass are run on
buffers embedded in sentinel-filled allocations — every byte in front of and behind the workspace / outputs must come back untouched.
(2) Determinism: the passes WITHOUT atomics are bit-identical run to run; the atomic ones (hash-table scatter) are bounded."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
GUARD = 1 << 16


def _guarded(nbytes: int):
    buf = torch.full((nbytes + 2 * GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    return buf, buf[GUARD:GUARD + nbytes]


def _intact(buf, nbytes):
    return bool((buf[:GUARD] == 0xA5).all()) and bool((buf[GUARD + nbytes:] == 0xA5).all())


def test_render_pass_stays_inside_its_workspace_and_outputs():
    from scaledreamer_amd import _lib, presets
    from scaledreamer_amd.renderer import _RenderPass
    from scaledreamer_amd.smoke import build_smoke_system

    system, batches = build_smoke_system(0, 1)
    system.on_train_batch_start()                  # (the step hook that builds the occupancy grid from the initial field)
    ren, geo = system.renderer, system.geometry
    b = batches[0]
    rays_o = b["rays_o"].reshape(-1, 3).contiguous().float()
    rays_d = b["rays_d"].reshape(-1, 3).contiguous().float()
    n_rays = rays_o.shape[0]
    est = ren.estimator
    mcfg = est.march_cfg(ren.cfg.near_plane, ren.cfg.far_plane, ren.render_step_size)
    bits = est._bits()
    st = _RenderPass(mcfg, geo._meta, geo._fcfg, rays_o, rays_d, bits, torch.rand(n_rays, device="cuda"), 1e-4, min(0.01, est._occ_mean), 1, 1,
                     n_rays * int(mcfg.max_steps))
    total = int(st.layout.total_bytes)
    wbuf, ws = _guarded(total)
    st.ws = ws
    grid = geo.encoding.encoding.encoding.params.detach()
    w = [t.detach() for t in geo._weights()]
    bg = torch.rand(n_rays, 3, device="cuda")
    p = st.params(grid, *w, bg)
    _lib.check(_lib.lib().asd_render_fwd(C.byref(p), _lib.ptr(ws), _lib.stream()))
    torch.cuda.synchronize()
    assert _intact(wbuf, total), "asd_render_fwd wrote outside its workspace"
    n_kept = int(st.view("n_kept").item())
    assert 0 < n_kept <= st.capacity and int(st.view("kept").sum()) == n_kept
    # backward: every output embedded in its own guarded allocation
    nf = C.c_int64(0)
    _lib.check(_lib.lib().asd_render_bwd_workspace(C.byref(p), C.byref(nf)))
    outs = {k: _guarded(t.numel() * 4) for k, t in (("grid", grid), ("w1d", w[0]), ("w2d", w[1]), ("w1f", w[2]), ("w2f", w[3]), ("bg", bg))}
    bb, bws = _guarded(nf.value * 4)
    for k, (bufk, v) in outs.items():
        v.zero_()
    dcomp, dop = torch.randn(n_rays, 3, device="cuda"), torch.randn(n_rays, device="cuda")
    fp = lambda k: C.c_void_p(outs[k][1].data_ptr())
    _lib.check(_lib.lib().asd_render_bwd(C.byref(p), _lib.ptr(ws), _lib.ptr(dcomp), None, _lib.ptr(dop), None, None, fp("grid"), fp("w1d"), fp("w2d"),
                                         fp("w1f"), fp("w2f"), fp("bg"), C.c_void_p(bws.data_ptr()), _lib.stream()))
    torch.cuda.synchronize()
    assert _intact(wbuf, total) and _intact(bb, nf.value * 4)
    for k, (bufk, v) in outs.items():
        assert _intact(bufk, v.numel()), k
    dgrid = outs["grid"][1].view(torch.float32)
    assert torch.isfinite(dgrid).all() and float(dgrid.abs().sum()) > 0


# ---- the field backward passes: asd_field_bwd (hash grid: the smoke system's field), asd_voxfield_bwd (16^3 x 32 volume), asd_trifield_bwd (64^2 planes) ----
_FIELD_CASES = [(kind, wn, None) for kind in ("field", "voxfield", "trifield") for wn in (True, False)] + [("trifield", True, 1000), ("trifield", False, 1000)]
_FIELD_IDS = [f"{k}-{'normal' if wn else 'plain'}" + (f"-chunk{ch}" if ch else "") for k, wn, ch in _FIELD_CASES]


def _sdf_cfg():
    from scaledreamer_amd import _lib

    f = _lib.FieldCfg()
    for d in range(3):
        f.bbox_min[d], f.bbox_max[d] = -2.0, 2.0
    f.radius, f.bias_mode, f.bias_value = 2.0, _lib.ASD_BIAS_SPHERE, 0.8
    f.blob_scale, f.blob_std, f.activation = 0.0, 1.0, _lib.ASD_ACT_NONE
    f.fd_eps, f.n_hidden, f.n_feature_dims, f.field_mode = 0.01, 64, 3, _lib.ASD_FIELD_SDF
    return f


def _field_bwd_case(kind, with_normal):
    """One backward call of `kind` at 3001 points -> (workspace floats, {gradient output: element count}, call(workspace pointer, {output: pointer})).
    The forward pass runs here, through ops; the backward entry is called through bare ctypes."""
    from scaledreamer_amd import _lib, ops

    L, n = _lib.lib(), 3001
    g = torch.Generator().manual_seed(11)
    rnd = lambda *sh, scale=1.0: (torch.randn(*sh, generator=g) * scale).cuda()
    d_out, d_feats = rnd(n), rnd(n, 3)
    d_normal, d_fdg = (rnd(n, 3), rnd(n, 3)) if with_normal else (None, None)
    nf = C.c_int64(0)
    if kind == "field":
        from scaledreamer_amd.smoke import build_smoke_system

        geo = build_smoke_system(0, 1)[0].geometry
        meta, cfg = geo._meta, geo._fcfg
        grid = geo.encoding.encoding.encoding.params.detach()
        w = [t.detach().contiguous() for t in geo._weights()]
        pts = ((torch.rand(n, 3, generator=g) * 2 - 1) * float(cfg.radius)).cuda()
        sigma, _, _, enc = ops.field_fwd(meta, cfg, grid, *w, pts, with_normal)
        _lib.check(L.asd_field_bwd_workspace(C.byref(cfg), _lib.i32(n), _lib.i32(int(with_normal)), C.byref(nf)))
        outs = {"grid": grid.numel(), "w1d": 64 * 32, "w2d": 64, "w1f": 64 * 32, "w2f": 3 * 64}

        def call(ws, o):
            _lib.check(L.asd_field_bwd(C.byref(meta), C.byref(cfg), _lib.ptr(grid), *[_lib.ptr(t) for t in w], _lib.ptr(pts), _lib.ptr(enc), _lib.ptr(sigma),
                                       _lib.i32(n), None, _lib.ptr(d_out), _lib.ptr(d_feats), _lib.ptr(d_normal), None, o["grid"], o["w1d"], o["w2d"], o["w1f"],
                                       o["w2f"], ws, _lib.stream()))
        return nf.value, outs, call
    cfg = _sdf_cfg()
    pts = (torch.rand(n, 3, generator=g) * 4.4 - 2.2).cuda()          # some points outside the box: zero padding of the lookup
    if kind == "voxfield":
        vol = rnd(16, 16, 16, 32, scale=0.5)
        w = [rnd(64, 32, scale=0.2), rnd(1, 64, scale=0.2), rnd(64, 32, scale=0.2), rnd(3, 64, scale=0.2)]
        sdf, _, _, _, enc = ops.voxfield_fwd(vol, cfg, *w, pts, with_normal)
        _lib.check(L.asd_voxfield_bwd_workspace(C.byref(cfg), _lib.i32(n), _lib.i32(int(with_normal)), C.byref(nf)))
        outs = {"voxel": vol.numel(), "dw1_sdf": 64 * 32, "dw2_sdf": 64, "dw1_feature": 64 * 32, "dw2_feature": 3 * 64}

        def call(ws, o):
            _lib.check(L.asd_voxfield_bwd(_lib.ptr(vol), _lib.i32(16), _lib.i32(16), _lib.i32(16), _lib.i32(32), C.byref(cfg), *[_lib.ptr(t) for t in w],
                                          _lib.ptr(pts), _lib.ptr(enc), _lib.ptr(sdf), _lib.i32(n), _lib.ptr(d_out), _lib.ptr(d_feats), _lib.ptr(d_normal),
                                          _lib.ptr(d_fdg), o["voxel"], o["dw1_sdf"], o["dw2_sdf"], o["dw1_feature"], o["dw2_feature"], ws, _lib.stream()))
        return nf.value, outs, call
    planes = rnd(3, 64, 64, 32, scale=0.5)
    shapes = ((96, 64), (64, 64), (1, 64), (96, 64), (64, 64), (3, 64))
    w6 = [rnd(*sh, scale=0.2) for sh in shapes]
    sdf = ops.trifield_fwd(planes, cfg, w6, pts, with_normal)[0]
    _lib.check(L.asd_trifield_bwd_workspace(_lib.i32(64), _lib.i32(64), _lib.i32(n), _lib.i32(int(with_normal)), C.byref(nf)))
    outs = {"planes": planes.numel(), **{f"dw{j}": sh[0] * sh[1] for j, sh in enumerate(shapes)}}

    def call(ws, o):
        _lib.check(L.asd_trifield_bwd(_lib.ptr(planes), _lib.i32(64), _lib.i32(64), _lib.i32(32), C.byref(cfg), ops._ptr6(w6), _lib.ptr(pts), _lib.ptr(sdf),
                                      _lib.i32(n), _lib.ptr(d_out), _lib.ptr(d_feats), _lib.ptr(d_normal), _lib.ptr(d_fdg), o["planes"],
                                      (C.c_void_p * 6)(*[o[f"dw{j}"].value for j in range(6)]), ws, _lib.stream()))
    return nf.value, outs, call


def _run_field_bwd(case, ws_byte):
    """the call on a workspace of exactly asd_*_bwd_workspace() floats pre-filled with `ws_byte` and zeroed gradient outputs (the entries accumulate), every
    buffer inside a sentinel-filled allocation -> ({output: gradient}, all guard bytes intact)"""
    nf, outs, call = case
    wbuf, ws = _guarded(nf * 4)
    ws.fill_(ws_byte)
    bufs = {k: _guarded(ne * 4) for k, ne in outs.items()}
    for _, v in bufs.values():
        v.zero_()
    call(C.c_void_p(ws.data_ptr()), {k: C.c_void_p(v.data_ptr()) for k, (_, v) in bufs.items()})
    torch.cuda.synchronize()
    intact = _intact(wbuf, nf * 4) and all(_intact(b, outs[k] * 4) for k, (b, _) in bufs.items())
    return {k: v.view(torch.float32).clone() for k, (_, v) in bufs.items()}, intact


@pytest.mark.parametrize("kind,with_normal,chunk", _FIELD_CASES, ids=_FIELD_IDS)
def test_field_backward_passes_stay_inside_their_workspace_and_outputs(kind, with_normal, chunk, monkeypatch):
    if chunk:
        monkeypatch.setenv("ASD_TRI_CHUNK", str(chunk))         # 3001 points: four chunks
    grads, intact = _run_field_bwd(_field_bwd_case(kind, with_normal), 0xA5)
    assert intact, f"asd_{kind}_bwd wrote outside its workspace or a gradient output"
    for k, v in grads.items():
        assert torch.isfinite(v).all() and float(v.abs().sum()) > 0, k


@pytest.mark.parametrize("kind,with_normal,chunk", _FIELD_CASES, ids=_FIELD_IDS)
def test_field_backward_passes_never_read_unwritten_workspace(kind, with_normal, chunk, monkeypatch):
    """The callers hand these entries a torch.empty workspace.  Pre-filled with 0xFF bytes (a NaN as a float, -1 as an integer) and with zeros, every
    gradient must be finite and the two runs must agree: to 2e-3 of the largest entry (the bound of test_fused_sampled_field_matches_the_composed_path
    for head gradients; the scatters and the second-layer sums are fp32 atomics), bit for bit for the voxel entry's first-layer weight gradients
    (field_wgrad_kernel + slab_reduce_kernel: no atomics)."""
    if chunk:
        monkeypatch.setenv("ASD_TRI_CHUNK", str(chunk))
    case = _field_bwd_case(kind, with_normal)
    poisoned, ok1 = _run_field_bwd(case, 0xFF)
    zeroed, ok0 = _run_field_bwd(case, 0x00)
    assert ok1 and ok0
    for k in zeroed:
        assert torch.isfinite(poisoned[k]).all() and torch.isfinite(zeroed[k]).all(), k
        rel = float((poisoned[k] - zeroed[k]).abs().max() / zeroed[k].abs().max().clamp_min(1e-20))
        print(f"{kind} {k}: 0xFF-filled vs zero-filled workspace differ by {rel:.2e} of the largest entry")
        assert rel < 2e-3, k
        if kind == "voxfield" and k.startswith("dw1_"):
            assert torch.equal(poisoned[k], zeroed[k]), k


def test_conv3d_passes_stay_inside_their_buffers():
    from scaledreamer_amd import _lib
    from scaledreamer_amd import ops

    N, D, H, W, cin, cout = 1, 3, 16, 32, 64, 128
    x = torch.randn(N, D, H, W, cin, device="cuda")
    w = torch.randn(N, cout, cin, 3, 3, 3, device="cuda") * 0.02
    dy = torch.randn(N, D, H, W, cout, device="cuda")
    d = _lib.Conv3dDesc(N, D, H, W, cin, cout, None, None)
    zp = torch.zeros(64, device="cuda")
    for pss, out_elems in ((0, N * D * H * W * cout), (1, N * D * H * W * cin), (2, N * cout * cin * 27)):
        nb = _lib.lib().asd_conv3d_workspace_bytes(C.byref(d), _lib.i32(pss))
        wbuf, ws = _guarded(nb)
        obuf, out = _guarded(out_elems * 4)
        wp, op = C.c_void_p(ws.data_ptr()), C.c_void_p(out.data_ptr())
        if pss == 0:
            _lib.check(_lib.lib().asd_conv3d_fwd(C.byref(d), _lib.ptr(x), _lib.ptr(w), C.c_int64(cout * cin * 27), op, None, wp, C.c_int64(nb), _lib.stream()))
        elif pss == 1:
            _lib.check(_lib.lib().asd_conv3d_dgrad(C.byref(d), _lib.ptr(dy), _lib.ptr(w), C.c_int64(cout * cin * 27), op, wp, C.c_int64(nb), _lib.stream()))
        else:
            _lib.check(_lib.lib().asd_conv3d_wgrad(C.byref(d), _lib.ptr(x), _lib.ptr(dy), op, C.c_int64(cout * cin * 27), wp, C.c_int64(nb), _lib.ptr(zp), _lib.stream()))
        torch.cuda.synchronize()
        assert _intact(wbuf, nb) and _intact(obuf, out_elems * 4), f"pass {pss} wrote outside its buffers"
        assert torch.isfinite(out.view(torch.float32)).all()


# ---- the tri-plane transformer (csrc/tritx.hip): every workspace is exactly what its size query returns, inside a sentinel allocation; every
# output sits in a guarded allocation of its own ----
def _guarded_f32(*shape):
    n = int(np.prod(shape))
    buf, v = _guarded(n * 4)
    return buf, v.view(torch.float32).view(*shape), n * 4


def _all_intact(bufs):
    return all(_intact(b, nb) for b, _, nb in bufs)


def _tx_pack(w):
    """operand plane + scales of an nn.Linear weight [N, K]"""
    from scaledreamer_amd import _lib

    N, K = w.shape
    plane, inv = torch.empty((N, 3 * K), device="cuda", dtype=torch.float16), torch.empty(N, device="cuda")
    _lib.check(_lib.lib().asd_tx_pack_weight(_lib.ptr(w), _lib.i32(N), _lib.i32(K), _lib.ptr(plane), _lib.ptr(inv), None, None, None, _lib.stream()))
    return plane, inv


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("M,K,N", [(3072, 3072, 768), (200, 64, 128)])      # split-K 3 in the plan table / outside it
def test_tx_linear_stays_inside_its_buffers(M, K, N, mode):
    from scaledreamer_amd import _lib

    L = _lib.lib()
    g = torch.Generator(device="cuda").manual_seed(M + N)
    x = torch.randn(M, K, device="cuda", generator=g)
    plane, inv = _tx_pack(torch.randn(N, K, device="cuda", generator=g) * K ** -0.5)
    bias = torch.randn(N, device="cuda", generator=g)
    ws, y, aux = _guarded_f32(L.asd_tx_linear_workspace(_lib.i32(M), _lib.i32(N), _lib.i32(K))), _guarded_f32(M, N), _guarded_f32(M, N)
    _lib.check(L.asd_tx_linear(_lib.ptr(x), _lib.i32(M), _lib.i32(K), _lib.i32(K), _lib.ptr(plane), _lib.ptr(inv), _lib.i32(N), _lib.ptr(bias), _lib.i32(mode),
                               _lib.ptr(aux[1]) if mode else None, None, _lib.i32(N), _lib.ptr(y[1]), _lib.i32(N), _lib.ptr(ws[1]), _lib.stream()))
    torch.cuda.synchronize()
    assert _all_intact((ws, y, aux)), "asd_tx_linear wrote outside its workspace or an output"
    assert torch.isfinite(y[1]).all() and (mode == 0 or torch.isfinite(aux[1]).all())


@pytest.mark.parametrize("M,N,K", [(3072, 768, 3072), (130, 64, 128)])      # split-K 3 in the plan table / outside it
def test_tx_linear_wgrad_stays_inside_its_buffers(M, N, K):
    from scaledreamer_amd import _lib

    L = _lib.lib()
    g = torch.Generator(device="cuda").manual_seed(M + K)
    dy, x = torch.randn(M, N, device="cuda", generator=g), torch.randn(M, K, device="cuda", generator=g)
    ws, dw, db = _guarded_f32(L.asd_tx_wgrad_workspace(_lib.i32(M), _lib.i32(N), _lib.i32(K))), _guarded_f32(N, K), _guarded_f32(N)
    _lib.check(L.asd_tx_linear_wgrad(_lib.ptr(dy), _lib.i32(N), _lib.ptr(x), _lib.i32(K), _lib.i32(M), _lib.i32(N), _lib.i32(K), _lib.ptr(dw[1]), _lib.ptr(db[1]),
                                     _lib.ptr(ws[1]), _lib.stream()))
    torch.cuda.synchronize()
    assert _all_intact((ws, dw, db)), "asd_tx_linear_wgrad wrote outside its workspace or an output"
    assert torch.isfinite(dw[1]).all() and torch.isfinite(db[1]).all()


# shapes of test_gpu_tritx.py: forward, dK / dV and dQ all split | only dK / dV split (16 pieces: the largest partials) | nothing split
@pytest.mark.parametrize("Lq,Lk,H", [(3072, 3072, 16), (3072, 77, 16), (100, 50, 2)])
def test_tx_attention_passes_stay_inside_their_buffers(Lq, Lk, H):
    from scaledreamer_amd import _lib

    L = _lib.lib()
    g = torch.Generator(device="cuda").manual_seed(Lq + Lk)
    D = H * 48
    q, k, v = (torch.randn(n, D, device="cuda", generator=g) for n in (Lq, Lk, Lk))
    d_o = torch.randn(Lq, D, device="cuda", generator=g) * 1e-3
    nws = L.asd_tx_attention_workspace(_lib.i32(Lq), _lib.i32(Lk), _lib.i32(H))
    ws, o, lse = _guarded_f32(nws), _guarded_f32(Lq, D), _guarded_f32(H, Lq)
    ld = _lib.i32(D)
    _lib.check(L.asd_tx_attention_fwd(_lib.ptr(q), ld, _lib.ptr(k), ld, _lib.ptr(v), ld, _lib.i32(Lq), _lib.i32(Lk), _lib.i32(H), _lib.ptr(o[1]), ld, _lib.ptr(lse[1]),
                                      _lib.ptr(ws[1]), _lib.stream()))
    torch.cuda.synchronize()
    assert _all_intact((ws, o, lse)), "asd_tx_attention_fwd wrote outside its workspace or an output"
    assert torch.isfinite(o[1]).all() and torch.isfinite(lse[1]).all()
    ws, dq, dk, dv = _guarded_f32(nws), _guarded_f32(Lq, D), _guarded_f32(Lk, D), _guarded_f32(Lk, D)      # the same query serves the backward
    _lib.check(L.asd_tx_attention_bwd(_lib.ptr(q), ld, _lib.ptr(k), ld, _lib.ptr(v), ld, _lib.ptr(o[1]), ld, _lib.ptr(d_o), ld, _lib.ptr(lse[1]), _lib.i32(Lq),
                                      _lib.i32(Lk), _lib.i32(H), _lib.ptr(dq[1]), ld, _lib.ptr(dk[1]), ld, _lib.ptr(dv[1]), ld, _lib.ptr(ws[1]), _lib.stream()))
    torch.cuda.synchronize()
    assert _all_intact((ws, o, lse, dq, dk, dv)), "asd_tx_attention_bwd wrote outside its workspace or an output"
    assert all(torch.isfinite(t[1]).all() for t in (dq, dk, dv))


def test_tritx_generator_passes_stay_inside_their_buffers():
    """asd_tritx_pack / _fwd / _bwd at the reduced shape of test_gpu_tritx.py (TRI_HD48: 2 layers x 192 wide, 4 heads, 3 x 8^2 tokens), batch 2: the
    packed planes, the saved activations and the workspace are exactly what their queries return; the planes and each of the 38 gradients have a
    guarded allocation of their own.  (The packed buffer holds fp16 planes and bit patterns: its contents are judged through the planes they produce.)"""
    from scaledreamer_amd import _lib

    L = _lib.lib()
    nl, D, H, Dc, Tc, F, R, Cc, batch = 2, 192, 4, 128, 77, 768, 8, 32, 2
    T = 3 * R * R
    desc = _lib.TritxDesc(n_layers=nl, dim=D, heads=H, cond_dim=Dc, cond_tokens=Tc, hidden=F, low_res=R, out_channels=Cc, eps=1e-6)
    g = torch.Generator(device="cuda").manual_seed(48)
    layer = [(D,), (D,), (D, D), (D, Dc), (D, Dc), (D, D), (D,), (D,), (D,), (D, D), (D, D), (D, D), (D, D), (D,), (D,), (D,), (F, D), (F,), (D, F), (D,)]
    shapes = layer * nl + [(T, D), (D,), (D,), (D, 4 * Cc)]
    params = [torch.randn(*sh, device="cuda", generator=g) * (0.2 if len(sh) == 2 else 1.0) for sh in shapes]
    table = (C.c_void_p * len(params))(*[p.data_ptr() for p in params])
    text = torch.randn(batch, Tc, Dc, device="cuda", generator=g)
    packed = _guarded_f32(L.asd_tritx_packed_floats(C.byref(desc)))
    _lib.check(L.asd_tritx_pack(C.byref(desc), table, _lib.ptr(packed[1]), _lib.stream()))
    torch.cuda.synchronize()
    assert _all_intact((packed,)), "asd_tritx_pack wrote outside the packed buffer"
    nws = L.asd_tritx_workspace_floats(C.byref(desc))
    save, ws, planes = _guarded_f32(L.asd_tritx_save_floats(C.byref(desc), _lib.i32(batch))), _guarded_f32(nws), _guarded_f32(batch, 3, 2 * R, 2 * R, Cc)
    _lib.check(L.asd_tritx_fwd(C.byref(desc), table, _lib.ptr(packed[1]), _lib.ptr(text), _lib.i32(batch), _lib.ptr(planes[1]), _lib.ptr(save[1]), _lib.ptr(ws[1]),
                               _lib.stream()))
    torch.cuda.synchronize()
    assert _all_intact((packed, save, ws, planes)), "asd_tritx_fwd wrote outside a buffer"
    assert torch.isfinite(planes[1]).all()
    glayer = [(D,), (D,), (D, D), (2 * D, Dc), (D, D), (D,), (D,), (D,), (3 * D, D), (D, D), (D,), (D,), (D,), (F, D), (F,), (D, F), (D,)]
    grads = [_guarded_f32(*sh) for sh in glayer * nl + [(T, D), (D,), (D,), (D, 4 * Cc)]]
    gtable = (C.c_void_p * len(grads))(*[t[1].data_ptr() for t in grads])
    d_planes = torch.randn(batch, 3, 2 * R, 2 * R, Cc, device="cuda", generator=g)
    ws = _guarded_f32(nws)
    _lib.check(L.asd_tritx_bwd(C.byref(desc), table, _lib.ptr(packed[1]), _lib.ptr(text), _lib.i32(batch), _lib.ptr(d_planes), _lib.ptr(save[1]), gtable,
                               _lib.ptr(ws[1]), _lib.stream()))
    torch.cuda.synchronize()
    assert _all_intact([packed, save, ws, planes] + grads), "asd_tritx_bwd wrote outside a buffer"
    for i, t in enumerate(grads):
        assert torch.isfinite(t[1]).all(), i


def test_passes_without_atomics_are_bit_identical_and_the_scatter_is_bounded():
    from scaledreamer_amd import ops
    from scaledreamer_amd.smoke import build_smoke_system

    # split-fp16 convolution: forward, input gradient and weight gradient use no atomics on their outputs
    g = torch.Generator(device="cuda").manual_seed(3)
    x = torch.randn(1, 4, 32, 32, 64, device="cuda", generator=g)
    w = torch.randn(1, 64, 64, 3, 3, 3, device="cuda", generator=g) * 0.02
    dy = torch.randn(1, 4, 32, 32, 64, device="cuda", generator=g)
    for fn in (lambda: ops.conv3d_fwd(x, w), lambda: ops.conv3d_dgrad(dy, w, 64), lambda: ops.conv3d_wgrad(x, dy)):
        a, b = fn(), fn()
        assert torch.equal(a, b)
    # a whole training step twice from the same state: the UNet / VAE passes are deterministic, the hash-table gradient is a sum of fp32
    # atomics (order-dependent in the last bits) — bounded relative to its largest entry
    grads = []
    for _ in range(2):
        torch.manual_seed(0)
        system, batches = build_smoke_system(0, 1)
        system.train_one_step(batches[0])
        torch.cuda.synchronize()
        grads.append(system.geometry.encoding.encoding.encoding.params.grad.clone())
    diff = float((grads[0] - grads[1]).abs().max()) / float(grads[0].abs().max())
    print(f"run-to-run spread of the hash-table gradient: {diff:.2e} of its largest entry")
    assert diff < 5e-2
