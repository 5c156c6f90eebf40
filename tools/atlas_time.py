"""Time the textured mesh export on the MI355X: the asd_sd_nerf system of tests/test_gpu_atlas.py (seeded random weights, density blob raised
to 60, `mt-grid` at --res, default 32), exporter {uv_method: face-cells, fmt: obj-mtl, texture_format: png}.
  export()          host clock around system.export(dir) ending in a device synchronise, at every --sizes texture_size: isosurface, atlas,
                    bake, field evaluation at the owned texels, packing, and the OBJ / MTL / PNG written to a temporary directory
  asd_atlas_bake    device events around the one kernel, GB/s of the 17 bytes per texel it writes (12 gb_pos, 4 face_id, 1 covered)
One warm-up, then the median of --reps.    python tools/atlas_time.py [--res 32] [--sizes 1024 4096] [--reps 3]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=32)
    ap.add_argument("--sizes", type=int, nargs="+", default=[1024, 4096])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--bake-reps", type=int, default=20)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU: there is no fallback"
    from scaledreamer_amd import ops, plugins, presets  # noqa: F401
    from scaledreamer_amd.registry import find

    torch.manual_seed(0)
    cfg = presets.asd_sd_nerf()["system"]
    cfg.update(guidance_type="", optimizer={}, exporter={})
    cfg["geometry"].update(density_blob_scale=60.0, isosurface_method="mt-grid", isosurface_resolution=args.res, isosurface_coarse_to_fine=True,
                           isosurface_threshold=25.0)
    system = find("scaledreamer-system")(cfg).eval()
    mesh = system.geometry.isosurface()
    out = {"res": args.res, "vertices": mesh.v_pos.shape[0], "faces": mesh.t_pos_idx.shape[0], "reps": args.reps,
           "device": torch.cuda.get_device_name(0), "sizes": {}}
    for T in args.sizes:
        system.cfg.exporter = {"uv_method": "face-cells", "fmt": "obj-mtl", "texture_format": "png", "texture_size": T}
        times = []
        for rep in range(args.reps + 1):
            with tempfile.TemporaryDirectory() as d:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                paths = system.export(d)
                torch.cuda.synchronize()
                if rep > 0:     # rep 0 is the warm-up
                    times.append((time.perf_counter() - t0) * 1e3)
                files = {os.path.basename(p): os.path.getsize(p) for p in paths}
        lay = ops.atlas_layout(mesh.t_pos_idx.shape[0], T, 1)
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        bake = []
        for rep in range(args.bake_reps + 1):
            start.record()
            gb_pos, face_id, covered = ops.atlas_bake(lay, mesh.v_pos, mesh.t_pos_idx)
            stop.record()
            torch.cuda.synchronize()
            if rep > 0:
                bake.append(start.elapsed_time(stop))
            owned = int((face_id >= 0).sum())
            del gb_pos, face_id, covered
        ms = statistics.median(bake)
        out["sizes"][T] = {"export_ms": round(statistics.median(times), 1), "export_ms_all": [round(x, 1) for x in times], "files": files,
                           "cell": lay.c, "leg": lay.L, "owned_texels": owned, "bake_ms": round(ms, 4),
                           "bake_ms_min_max": [round(min(bake), 4), round(max(bake), 4)], "bake_bytes": 17 * T * T,
                           "bake_GBps": round(17 * T * T / (ms * 1e-3) / 1e9, 1)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
