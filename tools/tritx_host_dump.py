"""Workspace sizes of the tri-plane transformer and conv3d entry points, dumped for an A/B of two builds of the library (no device needed).

    ASD_HIP_LIB=/path/to/libasd_hip.so python tools/tritx_host_dump.py [--out FILE]

One library per process (ASD_HIP_LIB), in the style of tools/gemm_host_dump.py.  One line per query:
  * asd_tx_linear_workspace / asd_tx_wgrad_workspace / asd_tx_attention_workspace over the product shapes of the shipped model (tx_plans[] of
    csrc/tritx.hip, as the Linear and the weight gradient that produce them), the shapes parametrised in tests/test_gpu_tritx.py and a few
    shapes outside the plan table;
  * asd_tritx_packed_floats / _save_floats / _workspace_floats for TRI_FULL and TRI_HD48 at batch 1 / 2 / 4 and for a rejected descriptor.
    Beside every workspace row: the staging reservation the layout of csrc/tritx.hip dropped,
    al64(max(F D, 3 D D, 2 D Dc, 4 C D)) + al64(max(F, 3 D)) - a build with the reservation prints a size larger by exactly that;
  * asd_conv3d_workspace_bytes for the 3D generator's layers (generators.SynthesisNetwork3D.CHANNELS) at resolutions 4 .. 128, passes 0 / 1 / 2.
A refactor of the host code leaves the dumps of two builds byte-identical.  Prints the number of rows and the SHA-256 of the dump."""
import ctypes as C
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from scaledreamer_amd._lib import Conv3dDesc, TritxDesc, lib  # noqa: E402

# (M, N, K3) of tx_plans[]: a Linear x [M, K3 / 3] -> [M, N], and the weight gradient whose product [N', K'] over tx_rp(M') rows it is
PLANS = [(3072, 768, 2304), (3072, 2304, 2304), (3072, 3072, 2304), (3072, 768, 9216), (3072, 768, 6912), (77, 1536, 3072), (3072, 128, 2304),
         (3072, 768, 384), (768, 768, 9216), (2304, 768, 9216), (768, 3072, 9216), (1536, 1024, 384), (768, 128, 9216)]
LINEAR_TESTS = [(3072, 768, 768), (3072, 768, 3072), (77, 1024, 1536), (3072, 3072, 768), (200, 64, 128)]      # (M, K, N) of test_gpu_tritx.py
WGRAD_TESTS = [(3072, 768, 768), (3072, 2304, 768), (77, 1536, 1024), (3072, 768, 3072), (130, 64, 128)]       # (M, N, K)
OTHER = [(64, 64, 64), (100, 4, 64), (1, 128, 192), (4096, 1024, 1024), (3071, 768, 768), (192, 768, 192), (5000, 2304, 768)]
ATTENTION = [(3072, 3072, 16), (3072, 77, 16), (100, 50, 2), (257, 33, 3), (192, 192, 4), (192, 77, 4), (1, 1, 1), (4096, 4096, 16), (12288, 77, 16), (513, 129, 64)]
TRI_FULL = dict(n_layers=12, dim=768, heads=16, cond_dim=1024, cond_tokens=77, hidden=3072, low_res=32, out_channels=32)
TRI_HD48 = dict(n_layers=2, dim=192, heads=4, cond_dim=128, cond_tokens=77, hidden=768, low_res=8, out_channels=32)
CHANNELS = {4: 512, 8: 512, 16: 512, 32: 256, 64: 128, 128: 64}


def al64(n):
    return (n + 63) // 64 * 64


def main(argv):
    out = open(argv[argv.index("--out") + 1], "w") if "--out" in argv else None
    L = lib()
    lines = []
    i32 = C.c_int32
    linear = sorted({(M, N, K3 // 3) for M, N, K3 in PLANS} | {(M, N, K) for M, K, N in LINEAR_TESTS} | set(OTHER))
    # a plan row (N', K', 3 Mp) is the product of the weight gradient (M', N', K') with round64(M') = Mp: 3072 and 77 -> 128 rows in the model
    wgrad = sorted({(M, N, K) for N, K, K3 in PLANS for M in ((K3 // 3, 77) if K3 == 384 else (K3 // 3,))} | set(WGRAD_TESTS) | set(OTHER))
    for M, N, K in linear:
        lines.append(f"asd_tx_linear_workspace M={M} N={N} K={K}: {L.asd_tx_linear_workspace(i32(M), i32(N), i32(K))}")
    for M, N, K in wgrad:
        lines.append(f"asd_tx_wgrad_workspace M={M} N={N} K={K}: {L.asd_tx_wgrad_workspace(i32(M), i32(N), i32(K))}")
    for Lq, Lk, H in ATTENTION:
        lines.append(f"asd_tx_attention_workspace Lq={Lq} Lk={Lk} H={H}: {L.asd_tx_attention_workspace(i32(Lq), i32(Lk), i32(H))}")
    for name, cfg in (("TRI_FULL", TRI_FULL), ("TRI_HD48", TRI_HD48), ("rejected (dim != 48 heads)", dict(TRI_HD48, dim=256))):
        desc = TritxDesc(eps=1e-6, **cfg)
        D, F, Dc, Cc = cfg["dim"], cfg["hidden"], cfg["cond_dim"], cfg["out_channels"]
        stage = al64(max(F * D, 3 * D * D, 2 * D * Dc, 4 * Cc * D)) + al64(max(F, 3 * D))
        lines.append(f"asd_tritx_packed_floats {name}: {L.asd_tritx_packed_floats(C.byref(desc))}")
        for batch in (1, 2, 4):
            lines.append(f"asd_tritx_save_floats {name} batch={batch}: {L.asd_tritx_save_floats(C.byref(desc), i32(batch))}")
        lines.append(f"asd_tritx_workspace_floats {name}: {L.asd_tritx_workspace_floats(C.byref(desc))}   (dropped staging reservation: {stage})")
    shapes = [(r, max(r, 16), max(r, 16), cin, CHANNELS[r]) for r in CHANNELS for cin in sorted({CHANNELS[max(r // 2, 4)], CHANNELS[r]})]
    for D, H, W, cin, cout in shapes + [(3, 16, 32, 64, 128), (4, 32, 32, 64, 64)]:
        d = Conv3dDesc(1, D, H, W, cin, cout, None, None)
        lines.append(f"asd_conv3d_workspace_bytes D={D} H={H} W={W} Cin={cin} Cout={cout}: "
                     + " ".join(f"pass{p}={L.asd_conv3d_workspace_bytes(C.byref(d), i32(p))}" for p in (0, 1, 2)))
    text = "\n".join(lines) + "\n"
    if out:
        out.write(text)
    print("lib", os.environ.get("ASD_HIP_LIB", "in-tree"), "rows", len(lines), "sha256", hashlib.sha256(text.encode()).hexdigest())
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
