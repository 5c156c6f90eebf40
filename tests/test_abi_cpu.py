"""The C-ABI library loads (no GPU needed) and exports every symbol include/asd_hip.h declares."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared_symbols():
    src = open(os.path.join(ROOT, "include", "asd_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(asd_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_every_declared_symbol():
    from scaledreamer_amd import _lib

    names = _declared_symbols()
    assert len(names) >= 20
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/asd_hip.h but not exported"
    assert sorted(_lib.SYMBOLS) == names


def test_host_side_grid_meta_matches_oracle(oracle):
    from scaledreamer_amd import _lib

    for args in [(16, 2, 19, 16, 1.447269237440378), (4, 2, 19, 4, 4.0), (16, 2, 19, 16, 1.0)]:
        a = _lib.make_grid_meta(*args)
        b = oracle.grid_meta(*args)
        assert bytes(a) == bytes(b)
    assert _lib.make_grid_meta(16, 2, 19, 16, 1.447269237440378).n_params == 12_599_920


def test_struct_layouts_match_between_binding_and_oracle(oracle):
    from scaledreamer_amd import _lib

    for a, b in [(_lib.GridMeta, oracle.GridMeta), (_lib.FieldCfg, oracle.FieldCfg), (_lib.MarchCfg, oracle.MarchCfg)]:
        assert ctypes.sizeof(a) == ctypes.sizeof(b)
        assert [(n, t) for n, t in a._fields_] == [(n, t) for n, t in b._fields_]


def test_errors_are_reported_not_swallowed():
    from scaledreamer_amd import _lib

    m = _lib.GridMeta()
    assert _lib.lib().asd_grid_meta_init(ctypes.byref(m), 17, 2, 19, 16, 1.5) == 0
    assert b"levels" in _lib.lib().asd_last_error()


def test_network_weight_tables_match_the_packers():
    """asd_unet_create / asd_vae_enc_create publish the packed weight table they read; weights.pack_unet / pack_vae_encoder must
    produce exactly those names and sizes (no device needed: handles own no device memory until weights are bound)."""
    import ctypes as C

    import torch

    from scaledreamer_amd._lib import WeightInfo, check, i32, lib
    from scaledreamer_amd.diffusion import weights as W
    from scaledreamer_amd.diffusion.engine import unet_desc
    from scaledreamer_amd.diffusion.vae_hip import vae_desc

    def table(kind, desc):
        h = C.c_void_p()
        check(getattr(lib(), f"asd_{kind}_create")(C.byref(desc), C.byref(h)))
        info, out = WeightInfo(), {}
        for i in range(getattr(lib(), f"asd_{kind}_num_weights")(h)):
            check(getattr(lib(), f"asd_{kind}_weight_info")(h, i32(i), C.byref(info)))
            out[info.name.decode()] = (info.rows, info.cols)
        assert getattr(lib(), f"asd_{kind}_weight_info")(h, i32(len(out)), C.byref(info)) != 0      # out of range -> error status
        getattr(lib(), f"asd_{kind}_destroy")(h)
        return out

    for cfg in (W.UNetConfig(), W.UNetConfig(camera_dim=16), W.UNetConfig(model_channels=64, context_dim=96, channel_mult=(1, 2), attention_resolutions=(1,))):
        packed = W.pack_unet({k: torch.empty(v, device="meta") for k, v in W.unet_layout(cfg)[0].items()}, cfg)
        t = table("unet", unet_desc(cfg))
        assert set(t) == set(packed)
        for k, (r, c) in t.items():
            assert packed[k].numel() == r * c, (k, tuple(packed[k].shape), r, c)
    t = table("unet", unet_desc(W.UNetConfig()))
    assert t["emb_all.weight"] == (sum(c for k, (r, c) in t.items() if k.endswith("in_layers.2.bias")), 1280)
    assert t["input_blocks.1.1.transformer_blocks.0.attn1.to_qk.weight"] == (640, 320) and t["input_blocks.0.0.weight"] == (320, 288)
    for cfg in (W.VAEConfig(), W.VAEConfig(ch=32)):
        packed = W.pack_vae_encoder({k: torch.zeros(v) for k, v in W.vae_encoder_layout(cfg)[0].items()}, cfg)
        t = table("vae_enc", vae_desc(cfg))
        assert set(t) == set(packed)
        for k, (r, c) in t.items():
            assert packed[k].numel() == r * c, (k, tuple(packed[k].shape), r, c)
    bad = unet_desc(W.UNetConfig())
    bad.num_head_channels = 32
    h = C.c_void_p()
    assert lib().asd_unet_create(C.byref(bad), C.byref(h)) != 0 and b"head_dim 64" in lib().asd_last_error()


_SMALL_UNET = dict(model_channels=64, context_dim=96, channel_mult=(1, 2), attention_resolutions=(1,))
# (UNetConfig arguments, (batch, hw, frames, tune, n_uniq)) -> asd_unet_workspace_bytes_shared, n_ctx 77
_UNET_WS = [
    ({}, (1, 8, 1, 0, 0), 29504512), ({}, (5, 64, 1, 0, 0), 3130461184), ({}, (5, 64, 1, 0, 1), 3033559552), ({}, (2, 16, 1, 0, 0), 102285568),
    (dict(camera_dim=16), (4, 32, 4, 0, 0), 671877888), (dict(camera_dim=16), (8, 32, 4, 1, 0), 1792818432),
    (dict(camera_dim=16), (2, 16, 1, 0, 0), 102295808),
    (_SMALL_UNET, (1, 8, 1, 0, 0), 5608192), (_SMALL_UNET, (5, 64, 1, 0, 0), 447785984), (_SMALL_UNET, (5, 64, 1, 0, 1), 428580352),
    (_SMALL_UNET, (2, 16, 1, 0, 0), 15465728),
]
# (batch, res, tune) -> asd_vae_enc_workspace_bytes for VAEConfig() / VAEConfig(ch=32)
_VAE_ENC_WS = {(1, 8, 0): (6231040, 5882112), (1, 64, 0): (34339584, 12065024), (4, 256, 0): (1566771456, 418343168),
               (1, 512, 0): (1707033344, 570565376), (1, 512, 1): (2250533888, 1097989376), (3, 40, 0): (39132672, 13039872)}
# (batch, hl) -> asd_vae_dec_workspace_bytes(.., tune 0) for VAEConfig() / VAEConfig(ch=32); None: the shape is refused (negative)
_VAE_DEC_WS = {(1, 4): (2311936, 677632), (1, 8): (8864512, 2327296), (4, 32): (559024384, 143001856), (16, 64): (8929812736, 2282889472),
               (3, 6): (None, None)}


def test_network_workspace_sizes_are_pinned():
    """asd_unet_workspace_bytes_shared / asd_vae_enc_workspace_bytes / asd_vae_dec_workspace_bytes under the committed plan table (host
    arithmetic only: no device needed).  The passes carve their workspace by the very walk that answers these queries, so a size that
    moves is an allocation sequence, a record count or a split-K scratch need that moved."""
    import ctypes as C

    import pytest

    if os.environ.get("ASD_GEMM_PLAN_FILE"):
        pytest.skip("ASD_GEMM_PLAN_FILE is set: the recorded sizes are those of the committed gemm_plans.json")
    from scaledreamer_amd._lib import check, i32, lib
    from scaledreamer_amd.diffusion import hip_ops as H  # noqa: F401  (pushes the committed plans into the library)
    from scaledreamer_amd.diffusion import weights as W
    from scaledreamer_amd.diffusion.engine import unet_desc
    from scaledreamer_amd.diffusion.vae_hip import vae_desc

    l = lib()
    assert l.asd_gemm_plan_count() >= 164

    def handle(kind, desc):
        h = C.c_void_p()
        check(getattr(l, f"asd_{kind}_create")(C.byref(desc), C.byref(h)))
        return h

    unets = {}
    for kw, (B, hw, frames, tune, n_uniq), want in _UNET_WS:
        key = tuple(sorted(kw.items()))
        if key not in unets:
            unets[key] = handle("unet", unet_desc(W.UNetConfig(**kw)))
        got = l.asd_unet_workspace_bytes_shared(unets[key], i32(B), i32(hw), i32(hw), i32(77), i32(frames), i32(tune), i32(n_uniq))
        assert got == want, (kw, (B, hw, frames, tune, n_uniq), got, want)
    for h in unets.values():
        l.asd_unet_destroy(h)
    for col, cfg in enumerate((W.VAEConfig(), W.VAEConfig(ch=32))):
        enc, dec = handle("vae_enc", vae_desc(cfg)), handle("vae_dec", vae_desc(cfg))
        for (B, res, tune), want in _VAE_ENC_WS.items():
            for _ in range(2):      # the second query of a shape may be answered from the handle's record of the first
                got = l.asd_vae_enc_workspace_bytes(enc, i32(B), i32(res), i32(res), i32(tune))
                assert got == want[col], ("vae_enc", col, (B, res, tune), got, want[col])
        for (B, hl), want in _VAE_DEC_WS.items():
            got = l.asd_vae_dec_workspace_bytes(dec, i32(B), i32(hl), i32(hl), i32(0))
            assert (got < 0) if want[col] is None else (got == want[col]), ("vae_dec", col, (B, hl), got, want[col])
        l.asd_vae_enc_destroy(enc)
        l.asd_vae_dec_destroy(dec)


def test_gemm_plan_table_round_trip():
    import ctypes as C

    from scaledreamer_amd._lib import GemmArgs, check, i32, lib

    n0 = lib().asd_gemm_plan_count()
    check(lib().asd_gemm_plan_set(i32(123456), i32(64), i32(72), i32(0), i32(72), i32(0), i32(0), i32(0), i32(0), i32(3), i32(2)))
    assert lib().asd_gemm_plan_count() == n0 + 1
    g = GemmArgs()
    g.M, g.N, g.K, g.lda = 123456, 64, 72, 72
    t, sk = C.c_int32(), C.c_int32()
    assert lib().asd_gemm_plan_get(C.byref(g), C.byref(t), C.byref(sk)) == 0 and (t.value, sk.value) == (3, 2)
    assert lib().asd_gemm_workspace_bytes(C.byref(g)) == 2 * 123456 * 64 * 4
    g.lda = 80                                   # another leading dimension is another shape: defaults, reported as un-tuned
    assert lib().asd_gemm_plan_get(C.byref(g), C.byref(t), C.byref(sk)) == 1 and t.value == 0 and sk.value >= 1
    assert lib().asd_gemm_plan_set(i32(1), i32(1), i32(1), i32(0), i32(0), i32(0), i32(0), i32(0), i32(0), i32(99), i32(1)) != 0


def test_gemm_tile_table_is_the_one_python_and_the_plans_use():
    """asd_gemm_tile_info reads the table the launches dispatch on: the tile names of hip_ops are its rows by kind, a host-side decision
    that depends on a row's tile (the GroupNorm record count of asd_gemm_gn_records) follows the numbers it reports, and every committed
    plan names a row whose kind and tile fit the plan's shape, by the conditions asd_gemm_f16 checks before it launches."""
    import ast
    import ctypes as C
    import json

    from scaledreamer_amd._lib import GemmArgs, i32, lib
    from scaledreamer_amd.diffusion import hip_ops as H

    buf = (C.c_int32 * 7)()
    rows = []
    while lib().asd_gemm_tile_info(i32(len(rows)), buf) == 0:
        rows.append(tuple(buf))
        assert len(rows) < 1000
    n = len(rows)
    assert n >= 1 and lib().asd_gemm_tile_info(i32(-1), buf) != 0 and lib().asd_gemm_tile_info(i32(n), buf) != 0 and lib().asd_gemm_tile_info(i32(n + 7), buf) != 0
    assert lib().asd_gemm_tile_info(i32(0), None) != 0
    assert rows == list(H.TILES) and len(H.TILE_BM) == len(H.TILE_BN) == n
    for i, (kind, bm, bn, wm, wn, nst, kg) in enumerate(rows):
        assert kind in (H.KIND_PLAIN, H.KIND_WIN, H.KIND_WIN2, H.KIND_PP, H.KIND_WS)
        assert (i in H.WINDOW_TILES) == (kind in (H.KIND_WIN, H.KIND_WIN2, H.KIND_PP)) and (i in H.PP_TILES) == (kind == H.KIND_PP) and (i == H.WS_TILE) == (kind == H.KIND_WS)
        assert (H.TILE_BM[i], H.TILE_BN[i]) == (bm, bn) and bm % 64 == 0 and bn % 32 == 0 and wm * wn in (4, 8, 10) and nst >= 2 and kg >= 1
        assert wm * wn * kg * 64 <= 1024, "threads of a block"
        if kind == H.KIND_PLAIN:
            assert nst * kg * (bm + bn) * 128 <= 160 * 1024, "operand ring within the CU's LDS"
        else:
            assert (nst, kg) == (2, 1)
        if kind in (H.KIND_WIN, H.KIND_WIN2):
            assert bm == 256 and bn in (64, 128)
        # the launch side reads the same row: one record per (bm x bn) tile of an image, for a 3x3 convolution every kind but WS can run
        g = GemmArgs()
        g.N, g.Cin = 640, 64
        g.M, g.K, g.conv, g.Hin, g.Win, g.Hout, g.Wout, g.stride, g.pad = 2 * 64 * 64, 9 * 64, 1, 64, 64, 64, 64, 1, 1
        g.split_k, g.tile_cfg, g.gn_cg, g.gn_rows, g.ldc = 1, i + 1, 640 // 32, 64 * 64, 640
        want = (4096 // bm) * -(-640 // bn) if 4096 % bm == 0 else 0
        assert lib().asd_gemm_gn_records(C.byref(g)) == want, (i, rows[i])
    g.tile_cfg = n + 1          # past the end: not a tile, the cost model's choice (window 256 x 128 on this shape)
    assert lib().asd_gemm_gn_records(C.byref(g)) == 16 * 5

    with open(H.PLAN_FILE if os.path.exists(H.PLAN_FILE) else os.path.join(ROOT, "scaledreamer_amd", "diffusion", "gemm_plans.json")) as f:
        plans = {ast.literal_eval(k): v for k, v in json.load(f).items()}
    assert len(plans) >= 100
    for (M, N, K, tail), (tile, split) in plans.items():
        assert 1 <= tile <= n and split >= 1, (M, N, K, tail, tile, split)
        kind, bm, bn, wm, wn, nst, kg = rows[tile - 1]
        conv = isinstance(tail, tuple)
        where = f"plan {(M, N, K, tail)} -> tile {tile} split {split}"
        assert bn == 64 or N % bn == 0 or (bn == 128 and N % 4 == 0), where
        if kind == H.KIND_PLAIN:
            if not conv and tail < 0:     # GEGLU epilogue: whole 32-column groups per wave, no split
                assert (bn // wn) % 32 == 0 and split == 1, where
            continue
        assert conv, where + ": a convolution kernel on a linear"
        hin, cin, stride, ups, pad = tail
        assert (stride, ups, pad) == (1, 0, 1) and K == 9 * cin, where
        if kind == H.KIND_WS:
            assert hin == 8 and M % 64 == 0 and M // 64 <= 5 and N % 64 == 0 and split >= 2 and cin % (32 * split) == 0, where
            continue
        assert hin % 16 == 0 and M % (hin * hin) == 0 and (split == 1 or split <= cin // 64), where + ": window kernels split over 64-channel chunks"
        if kind == H.KIND_PP:
            assert cin % 32 == 0 and N % bn == 0 and hin % (bm // 16) == 0, where
        else:
            assert cin % 64 == 0, where


def test_environment_variables_are_the_ones_integration_md_lists():
    """the names the library passes to getenv and the ASD_* names the package reads from os.environ are exactly the rows of the
    'Environment variables' table of INTEGRATION.md: a new switch is documented there or it does not exist"""
    import glob

    read = set()
    csrc = os.path.join(ROOT, "scaledreamer_amd", "csrc")
    for path in glob.glob(os.path.join(csrc, "*.hip")) + glob.glob(os.path.join(csrc, "*.h")):
        read |= set(re.findall(r'getenv\(\s*"(\w+)"', open(path).read()))
    for path in glob.glob(os.path.join(ROOT, "scaledreamer_amd", "**", "*.py"), recursive=True):
        read |= set(re.findall(r'os\.environ(?:\.get\(|\[)\s*["\'](ASD_\w+)["\']', open(path).read()))
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    table = text[text.index("Environment variables"):]
    listed = set(re.findall(r"^\|\s*`(\w+)`\s*\|", table, re.M))
    assert read and read == listed, (sorted(read - listed), sorted(listed - read))
