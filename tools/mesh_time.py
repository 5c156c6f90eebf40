"""Time mesh extraction on the MI355X: ImplicitVolume.isosurface() of the asd_sd_nerf geometry (seeded random weights, density blob raised
to 60 so that a surface exists at threshold 25), `mt-grid` at --res (default 128).  One warm-up, then the median of --reps runs of every
stage, each ended by a device synchronise: field evaluation over the grid vertices, extraction (count, scans, one host read, emit), outlier
removal (component rounds with one host read each, counts, two scans, compaction), and isosurface() as a whole (coarse-to-fine: all three
twice).    python tools/mesh_time.py [--res 128] [--reps 5]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=128)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU: there is no fallback"
    from scaledreamer_amd import plugins, presets  # noqa: F401
    from scaledreamer_amd.geometry import scale_tensor
    from scaledreamer_amd.registry import find

    torch.manual_seed(0)
    cfg = presets.asd_sd_nerf()["system"]["geometry"]
    cfg.update(density_blob_scale=60.0, isosurface_method="mt-grid", isosurface_resolution=args.res, isosurface_threshold=25.0)
    geo = find("implicit-volume")(cfg).to("cuda").eval()
    geo._initilize_isosurface_helper()
    helper = geo.isosurface_helper
    grid = helper.grid_vertices
    rows = {"field_ms": [], "extract_ms": [], "outlier_ms": [], "isosurface_ms": []}
    mesh = clean = None
    with torch.no_grad():
        for rep in range(args.reps + 1):
            field, t_field = timed(lambda: geo.forward_field(scale_tensor(grid, helper.points_range, geo.bbox))[0])
            level = geo.forward_level(field, 25.0)
            mesh, t_extract = timed(lambda: helper(level))
            clean, t_outlier = timed(lambda: mesh.remove_outlier(0.01))
            _, t_all = timed(geo.isosurface)
            if rep > 0:     # rep 0 is the warm-up
                for k, v in zip(rows, (t_field, t_extract, t_outlier, t_all)):
                    rows[k].append(v)
    out = {k: round(statistics.median(v), 3) for k, v in rows.items()}
    out.update({k + "_all": [round(x, 3) for x in v] for k, v in rows.items()})
    out.update(res=args.res, reps=args.reps, grid_vertices=grid.shape[0], vertices=mesh.v_pos.shape[0], faces=mesh.t_pos_idx.shape[0],
               vertices_after_outlier_removal=clean.v_pos.shape[0], device=torch.cuda.get_device_name(0))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
