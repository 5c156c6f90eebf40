"""Time the textured background's forward and backward on the HIP entries against the torch composition (grid_sample + sigmoid and its
autograd backward) on the same device, alternating the two routes round by round:

    python tools/background_time.py [--rounds 7] [--reps 200] [--out profiles/background_bench.txt]

Shapes: the training shape of asd_sd_nerf (batch x height x width of the preset's first resolution, the default 3 x 64 x 64 texture, the
rays of one seeded camera batch) and the contended shape of tests/test_gpu_background.py (16,384 rays of one camera's solid angle: about
2.5 k rays on one texel).  Per route and pass: device events around `reps` calls, one line per round, then median and min..max."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
import torch.nn.functional as F

import background_util as U
from scaledreamer_amd import ops, presets
from scaledreamer_amd.background import TexturedBackground


def timeit(fn, reps):
    for _ in range(10):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


def torch_color(texture, dirs):
    uv = 2 * TexturedBackground.spherical_xyz_to_uv(dirs) - 1
    c = F.grid_sample(texture, uv.reshape(1, -1, 1, 2), mode="bilinear", padding_mode="reflection", align_corners=False)
    return torch.sigmoid(c.reshape(texture.shape[1], -1).T)


def training_dirs():
    """the ray directions of one seeded camera batch of asd_sd_nerf"""
    from scaledreamer_amd.data import RandomCameraIterableDataset

    with presets.random_weights_allowed():
        cfg = presets.asd_sd_nerf()
    torch.manual_seed(cfg["seed"])
    batch = RandomCameraIterableDataset(cfg["data"]).collate()
    b, h, w = cfg["data"]["batch_size"][0], cfg["data"]["height"][0], cfg["data"]["width"][0]
    dirs = batch["rays_d"].reshape(-1, 3).float()
    assert dirs.shape[0] == b * h * w
    return dirs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "background_bench.txt"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "timing needs the GPU"
    dev = torch.device("cuda", 0)
    lines = [f"device {torch.cuda.get_device_name(0)}; us per call, device events around {a.reps} calls, {a.rounds} alternating rounds"]
    shapes = [("asd_sd_nerf training shape", training_dirs()), ("contended", U.contended_dirs(16384, 5))]
    for name, dirs in shapes:
        dirs = dirs.to(dev).contiguous()
        n = dirs.shape[0]
        g = torch.Generator().manual_seed(3)
        texture = torch.randn(1, 3, 64, 64, generator=g).to(dev).requires_grad_(True)
        d_color = torch.randn(n, 3, generator=g).to(dev)
        _, n_t = U.backward_unit(texture.detach()[0].cpu(), dirs.cpu(), d_color.cpu(), "sigmoid")
        lines.append(f"== {name}: texture 3 x 64 x 64, {n} rays, at most {int(n_t.max())} rays around one texel")
        graph = torch_color(texture, dirs)          # the torch route's backward alone: its graph is built once and kept

        def hip_both():
            c = ops.bg_texture_fwd(texture.detach(), dirs)
            return ops.bg_texture_bwd(texture.detach(), dirs, d_color), c

        def torch_both():
            return torch.autograd.grad(torch_color(texture, dirs), texture, d_color)

        routes = {
            "fwd hip": lambda: ops.bg_texture_fwd(texture.detach(), dirs),
            "fwd torch": lambda: torch_color(texture.detach(), dirs),
            "bwd hip": lambda: ops.bg_texture_bwd(texture.detach(), dirs, d_color),
            "bwd torch": lambda: torch.autograd.grad(graph, texture, d_color, retain_graph=True),
            "fwd+bwd hip": hip_both,
            "fwd+bwd torch": torch_both,
        }
        # the two routes compute the same thing at this shape
        got, want = ops.bg_texture_bwd(texture.detach(), dirs, d_color), torch_both()[0]
        lines.append(f"   max |d_texture hip - torch| = {float((got - want).abs().max()):.3e} (max |d_texture| {float(want.abs().max()):.3e})")
        times = {k: [] for k in routes}
        for r in range(a.rounds):
            for k, fn in routes.items():
                times[k].append(timeit(fn, a.reps))
            lines.append(f"   round {r}: " + "  ".join(f"{k} {times[k][-1]:.2f}" for k in routes))
        for k in routes:
            lines.append(f"   {k:<14s} median {statistics.median(times[k]):8.2f} us   min..max {min(times[k]):.2f} .. {max(times[k]):.2f}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
