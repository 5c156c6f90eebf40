"""Host-side decisions of the GEMM entry points, dumped for an A/B of two builds of the library (no device needed).

    ASD_HIP_LIB=/path/to/libasd_hip.so [ASD_GEMM_PLAN_FILE=none] python tools/gemm_host_dump.py [--out FILE]

One library per process (ASD_HIP_LIB).  For every shape of scaledreamer_amd/diffusion/gemm_plans.json, crossed with split_k in
{0, 1, 2, 4}, tile_cfg in 0..29, gn_rows in {0, rows of one image}, gn_bwd_x, gn_apply and ln_mode off / on, one line with what
asd_gemm_plan_get, asd_gemm_workspace_bytes, asd_gemm_gn_records and asd_gemm_gn_applies return.  Run it once with the committed plans
loaded and once with ASD_GEMM_PLAN_FILE=none (cost model and default split), on both builds: a refactor of the host code leaves the
four dumps pairwise byte-identical.  Prints the five tile names of hip_ops, the number of rows and the SHA-256 of the dump."""
import ast
import ctypes as C
import hashlib
import itertools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from scaledreamer_amd._lib import GemmArgs, lib  # noqa: E402
from scaledreamer_amd.diffusion import hip_ops as H  # noqa: E402  (loads the plans unless ASD_GEMM_PLAN_FILE=none)


def shape_args(key):
    """GemmArgs of a plan key and the rows of one image (the token rows of a linear: 4096 where they divide M, else M)"""
    M, N, K, tail = key
    g = GemmArgs()
    g.M, g.N, g.K, g.ldw, g.ldc = M, N, K, K, N
    if isinstance(tail, tuple):
        hin, cin, stride, ups, pad = tail
        hout = 2 * hin if ups else (hin + 2 * pad - 3) // stride + 1
        g.conv, g.Hin, g.Win, g.Cin, g.Hout, g.Wout, g.stride, g.pad, g.upsample = 1, hin, hin, cin, hout, hout, stride, pad, ups
        return g, hout * hout
    g.lda, g.act = abs(tail), 2 if tail < 0 else 0
    return g, 4096 if M % 4096 == 0 else M


def main(argv):
    out = open(argv[argv.index("--out") + 1], "w") if "--out" in argv else None
    print("lib", os.environ.get("ASD_HIP_LIB", "in-tree"), "plans", lib().asd_gemm_plan_count())
    for name in ("TILE_BM", "TILE_BN", "WINDOW_TILES", "PP_TILES", "WS_TILE"):
        print(name, getattr(H, name))
    with open(os.path.join(ROOT, "scaledreamer_amd", "diffusion", "gemm_plans.json")) as f:
        keys = [ast.literal_eval(k) for k in sorted(json.load(f))]
    sha, rows = hashlib.sha256(), 0
    dummy = C.c_void_p(256)      # a non-null pointer the host entries only test
    t, sk = C.c_int32(), C.c_int32()
    for key in keys:
        base, img_rows = shape_args(key)
        for split, tile, gn_rows, bwd, apply_, ln in itertools.product((0, 1, 2, 4), range(30), (0, img_rows), (0, 1), (0, 1), (0, 1)):
            g = GemmArgs.from_buffer_copy(bytes(base))
            g.split_k, g.tile_cfg, g.gn_rows, g.gn_cg, g.gn_apply, g.ln_mode = split, tile, gn_rows, key[1] // 32 if gn_rows else 0, apply_, ln
            if bwd:
                g.gn_bwd_x = g.gn_bwd_fstats = g.gn_bwd_gamma = g.gn_bwd_beta = dummy
            rc = lib().asd_gemm_plan_get(C.byref(g), C.byref(t), C.byref(sk))
            line = (f"{key} split={split} tile={tile} gn_rows={gn_rows} bwd={bwd} apply={apply_} ln={ln}: plan={rc},{t.value},{sk.value} "
                    f"ws={lib().asd_gemm_workspace_bytes(C.byref(g))} rec={lib().asd_gemm_gn_records(C.byref(g))} "
                    f"app={lib().asd_gemm_gn_applies(C.byref(g))}\n")
            sha.update(line.encode())
            rows += 1
            if out:
                out.write(line)
    print("rows", rows, "sha256", sha.hexdigest())
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
