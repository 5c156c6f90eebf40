"""Time the NeuS renderer's training pass on the MI355X: `implicit-sdf` shape-initialised to a sphere of radius 0.5, `no-material`,
`neural-environment-map-background`, `neus-volume-renderer` at 64x64 rays and 512 samples per ray, one occupancy update from the field, then
forward (sampling with alpha pruning, field with normals, compositing) plus backward of a loss on comp_rgb, opacity, depth and the eikonal term.
  fused      ASD_NEUS=1: asd_neus_prune_count, asd_neus_composite_fwd / _bwd
  composed   ASD_NEUS=0: tensor-op step alpha and get_alpha, asd_prune_count fed -log(1 - alpha) / dt, asd_composite_* mode 1
The two routes alternate in one process on one device (--pairs pairs, after a warm-up of each route).  One figure per route and pair: the
host clock around --reps passes ending in a device synchronise, divided by --reps (a mean over a window of a few tenths of a second, not a
median of single passes); the medians of those figures; and the device launches of one pass counted with the profiler.
    python tools/neus_time.py [--pairs 3] [--reps 100] [--init-steps 1000]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

BG_ENC = {"otype": "HashGrid", "n_features_per_level": 2, "log2_hashmap_size": 19, "n_levels": 4, "base_resolution": 4, "per_level_scale": 4.0}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--init-steps", type=int, default=1000)
    ap.add_argument("--size", type=int, default=64)
    ap.add_argument("--spp", type=int, default=512)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU: there is no fallback"
    from scaledreamer_amd import ops, plugins  # noqa: F401
    from scaledreamer_amd.registry import find

    torch.manual_seed(0)
    geo = find("implicit-sdf")({"shape_init": "sphere", "shape_init_params": 0.5})
    mat = find("no-material")({"n_output_dims": 3, "color_activation": "sigmoid"})
    bg = find("neural-environment-map-background")({"color_activation": "sigmoid", "random_aug": False, "dir_encoding_config": BG_ENC})
    ren = find("neus-volume-renderer")({"radius": 1.0, "num_samples_per_ray": args.spp}, geometry=geo, material=mat, background=bg)
    for m in (geo, mat, bg, ren):
        m.cuda().train()
    geo.SHAPE_INIT_STEPS = args.init_steps
    t0 = time.perf_counter()
    geo.initialize_shape()
    torch.cuda.synchronize()
    init_s = time.perf_counter() - t0
    geo.update_step(0, 0)
    ren.update_step(0, 0)                       # the warm-up occupancy update from the field
    H = W = args.size
    c2w = torch.tensor([[[0.0, 0.0, 1.0, 1.3], [1.0, 0.0, 0.0, 0.0], [0.0, 1.0, 0.0, 0.0], [0.0, 0.0, 0.0, 1.0]]], device="cuda")
    focal = torch.tensor([0.5 * H / 0.5774], device="cuda")          # fovy 60 degrees
    rays_o, rays_d = ops.generate_rays(c2w, focal, H, W)
    light = rays_o[:, 0, 0]
    params = [p for m in (geo, bg, ren) for p in m.parameters() if p.requires_grad]

    def one_pass():
        for p in params:
            p.grad = None
        out = ren(rays_o=rays_o, rays_d=rays_d, light_positions=light)
        eik = ((torch.linalg.norm(out["sdf_grad"], ord=2, dim=-1) - 1.0) ** 2).mean()
        loss = out["comp_rgb"].sum() + (out["opacity"] ** 2).sum() + 0.1 * out["depth"].sum() + 10.0 * eik
        loss.backward()
        return out

    def timed(route, reps):
        os.environ["ASD_NEUS"] = route
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(reps):
            one_pass()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3 / reps

    def launches(route):
        os.environ["ASD_NEUS"] = route
        with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
            one_pass()
            torch.cuda.synchronize()
        return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)

    res = {"device": torch.cuda.get_device_name(0), "rays": H * W, "spp": args.spp, "init_steps": args.init_steps, "init_s": round(init_s, 2),
           "reps": args.reps, "fused_ms": [], "composed_ms": []}
    for route in ("1", "0"):
        timed(route, 3)                         # warm-up
    os.environ["ASD_NEUS"] = "1"
    out = one_pass()
    res["kept_samples"] = int(out["weights"].shape[0])
    res["opacity_mean"] = round(float(out["opacity"].detach().mean()), 4)
    for _ in range(args.pairs):
        res["fused_ms"].append(round(timed("1", args.reps), 3))
        res["composed_ms"].append(round(timed("0", args.reps), 3))
    res["fused_ms_median"], res["composed_ms_median"] = statistics.median(res["fused_ms"]), statistics.median(res["composed_ms"])
    try:
        res["fused_launches"], res["composed_launches"] = launches("1"), launches("0")
    except Exception as e:      # the timings above stand without the profiler
        res["launches_error"] = repr(e)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
