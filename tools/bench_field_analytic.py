"""Analytic normals (asd_field_analytic_fwd / _bwd) against the finite-difference fused route (asd_field_fwd / asd_field_bwd with normals)
on the kept samples of one asd_sd_nerf step: forward alone and forward + backward, same build, same process, alternating rounds with
warm-up.  Off the step path (the shipped step has lambda_orient = 0 and never evaluates a normal): the figures are reported,
not gated.

  python tools/bench_field_analytic.py [--steps 12] [--inner 20] [--iters 5] [--warmup 3] [--rounds 3]

The sample count is taken from a run: the system of bench.py is built and trained for --steps steps, then the renderer's sampler is asked
for the kept samples of the next batch.  Prints one JSON line: that count, median / min ms per call of the four sides (device events
around --inner calls, divided), and the ratios of the medians.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


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
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_field_analytic needs a GPU: a CPU timing says nothing about this path")
    import bench
    from scaledreamer_amd import ops

    dev = torch.device("cuda", 0)
    cfg, system, data = bench.build_system("hip", seed=10, workload="asd_sd_nerf")
    for _ in range(a.steps):
        system.train_one_step(bench.to_device(data.collate(), dev))
    batch = bench.to_device(data.collate(), dev)
    ren, geo = system.renderer, system.geometry
    with torch.no_grad():
        pts = ren._sample(batch["rays_o"].reshape(-1, 3).contiguous(), batch["rays_d"].reshape(-1, 3).contiguous())[3].contiguous()
    n = pts.shape[0]
    grid = geo.encoding.encoding.encoding.params.detach()
    w = [t.detach() for t in geo._weights()]
    meta, fc = geo._meta, geo._fcfg
    g = torch.Generator(device=dev).manual_seed(5)
    d_sigma, d_feats, d_normal = (torch.randn(s, device=dev, generator=g) for s in ((n,), (n, 3), (n, 3)))
    d_grid = torch.zeros_like(grid)

    def fd_fwd():
        return ops.field_fwd(meta, fc, grid, *w, pts, True)

    def an_fwd():
        return ops.field_analytic_fwd(meta, fc, grid, *w, pts)

    def fd_both():
        sigma, feats, normal, enc = fd_fwd()
        ops.field_bwd(meta, fc, grid, *w, pts, enc, sigma, d_sigma, d_feats, d_normal, d_grid)

    def an_both():
        sigma, feats, normal, enc = an_fwd()
        ops.field_analytic_bwd(meta, fc, grid, *w, pts, enc, sigma, d_sigma, d_feats, d_normal, d_grid)

    sides = {"fd_fwd": fd_fwd, "analytic_fwd": an_fwd, "fd_fwd_bwd": fd_both, "analytic_fwd_bwd": an_both}
    times = {k: [] for k in sides}
    with torch.no_grad():
        for _ in range(a.warmup):
            for fn in sides.values():
                fn()
        torch.cuda.synchronize()
        for _ in range(a.rounds):                  # alternate the sides: other work shares the host
            for k, fn in sides.items():
                times[k] += _time(fn, a.iters, a.inner)
        n_fd, n_an = fd_fwd()[2], an_fwd()[2]
    med = {k: statistics.median(v) for k, v in times.items()}
    result = {"what": "field_analytic_vs_finite_difference", "gpu": torch.cuda.get_device_name(0), "workload": "asd_sd_nerf", "steps_before": a.steps,
              "kept_samples": n, "runs_per_side": a.rounds * a.iters, "calls_per_run": a.inner,
              "ms_median": med, "ms_min": {k: min(v) for k, v in times.items()},
              "analytic_over_fd_fwd": med["analytic_fwd"] / med["fd_fwd"], "analytic_over_fd_fwd_bwd": med["analytic_fwd_bwd"] / med["fd_fwd_bwd"],
              # how far the two normals are apart on these samples (finite differences of step fd_eps against the derivative): context, not a check
              "mean_abs_normal_difference": float((n_fd - n_an).abs().mean())}
    print(json.dumps(result))


if __name__ == "__main__":
    main()
