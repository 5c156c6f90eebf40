"""The field kernels under a level limit (asd_grid_meta.n_masked_levels, ProgressiveBandHashGrid): what a coarse-to-fine SDF step pays per
level count.  asd_field_fwd with normals and fd_grad + asd_field_bwd with d_normal and d_fd_grad (the NeuS route: four encodes per sample
each way), the shipped grid, SDF mode with the sphere bias, n = 2^18 points uniform in the bounding box, the finite-difference step of the
level count, active levels 4 / 8 / 12 / 16.  Two more sides give the all-levels comparison its context: the route without a normal gradient
(forward without normals + the matrix-pipe backward: the headline step's) and asd_field_density.

  python tools/bench_field_progressive.py [--label NAME] [--levels 4,8,12,16] [--inner 10] [--iters 5] [--warmup 3] [--rounds 3]

One process measures ONE library (ASD_HIP_LIB selects it: a build of the parent commit made with tools/build_variant.sh sits next to the
tree's own); an A/B alternates processes.  Prints one JSON line per level count: median / min ms per call (device events around --inner
calls, divided) and the bytes gathered per sample, computed from the level count: 8 corners x 8 B per level and encode, 4 encodes in the
forward pass, 3 in the backward pass (the centre's encoding is saved).
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

GRID = (16, 2, 19, 16, 1.447269237440378)
RADIUS = 1.0


def _time(fn, iters, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    out = []
    for _ in range(iters):
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) / inner)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--label", default="tree")
    ap.add_argument("--levels", default="4,8,12,16")
    ap.add_argument("--n", type=int, default=1 << 18)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_field_progressive needs a GPU: a CPU timing says nothing about this path")
    from scaledreamer_amd import _lib, ops

    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(7)
    meta = _lib.make_grid_meta(*GRID)
    n = a.n
    grid = torch.rand(meta.n_params, device=dev, generator=g) - 0.5
    w1d, w1f = (torch.randn(64, 32, device=dev, generator=g) / 32 ** 0.5 for _ in range(2))
    w2d, w2f = torch.randn(1, 64, device=dev, generator=g) / 8, torch.randn(3, 64, device=dev, generator=g) / 8
    w = (w1d, w2d, w1f, w2f)
    pts = (torch.rand(n, 3, device=dev, generator=g) * 2 - 1) * 0.95 * RADIUS
    d_sdf, d_feats, d_normal, d_fd = (torch.randn(s, device=dev, generator=g) for s in ((n,), (n, 3), (n, 3), (n, 3)))
    d_grid = torch.zeros_like(grid)
    fc = _lib.FieldCfg()
    for d in range(3):
        fc.bbox_min[d], fc.bbox_max[d] = -RADIUS, RADIUS
    fc.radius, fc.bias_mode, fc.bias_value = RADIUS, _lib.ASD_BIAS_SPHERE, 0.5
    fc.blob_scale, fc.blob_std, fc.activation = 0.0, 1.0, _lib.ASD_ACT_NONE
    fc.n_hidden, fc.n_feature_dims, fc.field_mode = 64, 3, _lib.ASD_FIELD_SDF

    def sdf_fd():
        sdf, feats, normal, fd, enc = ops.field_fwd(meta, fc, grid, *w, pts, True, want_fd_grad=True)
        ops.field_bwd(meta, fc, grid, *w, pts, enc, sdf, d_sdf, d_feats, d_normal, d_grid, d_fd_grad=d_fd)

    def plain():
        sdf, feats, _, enc = ops.field_fwd(meta, fc, grid, *w, pts, False)
        ops.field_bwd(meta, fc, grid, *w, pts, enc, sdf, d_sdf, d_feats, None, d_grid)

    def density():
        ops.field_density(meta, fc, grid, w1d, w2d, pts)

    sides = {"sdf_fd_fwd_bwd": sdf_fd, "plain_fwd_bwd": plain, "density": density}
    for levels in (int(s) for s in a.levels.split(",")):
        meta.n_masked_levels = meta.n_levels - levels          # (a build of the parent commit ignores it: give it --levels 16)
        fc.fd_eps = 2 * RADIUS / (GRID[3] * GRID[4] ** (levels - 1))
        times = {k: [] for k in sides}
        with torch.no_grad():
            for _ in range(a.warmup):
                for fn in sides.values():
                    fn()
            torch.cuda.synchronize()
            for _ in range(a.rounds):
                for k, fn in sides.items():
                    times[k] += _time(fn, a.iters, a.inner)
        print(json.dumps({
            "what": "field_progressive", "label": a.label, "gpu": torch.cuda.get_device_name(0), "n": n, "active_levels": levels, "fd_eps": fc.fd_eps,
            "gathered_bytes_per_sample": {"sdf_fd_forward": 4 * levels * 64, "sdf_fd_backward": 3 * levels * 64, "plain_forward": levels * 64,
                                          "density": levels * 64},
            "runs_per_side": a.rounds * a.iters, "calls_per_run": a.inner,
            "ms_median": {k: statistics.median(v) for k, v in times.items()}, "ms_min": {k: min(v) for k, v in times.items()},
            "ms_max": {k: max(v) for k, v in times.items()}}), flush=True)


if __name__ == "__main__":
    main()
