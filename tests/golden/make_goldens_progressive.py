"""Golden vectors of the coarse-to-fine SDF route: the REFERENCE's own ProgressiveBandHashGrid (threestudio/models/networks.py:129-167) and
ImplicitSDF with finite_difference_normal_eps "progressive" (implicit_sdf.py:380-413), imported in place under ref_harness.py and run on the
CPU oracle (see make_goldens.py, make_goldens_neus.py).

  python tests/golden/make_goldens_progressive.py      # writes tests/golden/progressive_band.npz and neus_d_8x8x64_progressive.npz

The harness's oracle-backed tcnn.Encoding takes otype HashGrid only; ProgressiveBandHashGrid asks for otype Grid / type Hash (the same
grid by tcnn's own aliasing), so this generator registers a subclass that accepts that spelling.  The reference places its mask on
`get_rank()`, a CUDA ordinal: the imported module's get_rank is pointed at the CPU.  The .npz files are data only.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_goldens_neus as N  # noqa: E402  (installs the harness and the alpha-pruning estimator)
import ref_harness as H  # noqa: E402
from make_goldens import BG_ENC, grid_params  # noqa: E402

import threestudio.models.networks as tnet  # noqa: E402
from threestudio.models.background.neural_environment_map_background import NeuralEnvironmentMapBackground  # noqa: E402
from threestudio.models.geometry.implicit_sdf import ImplicitSDF  # noqa: E402
from threestudio.models.materials.no_material import NoMaterial  # noqa: E402
from threestudio.models.renderers.neus_volume_renderer import NeuSVolumeRenderer  # noqa: E402


class GridHashEncoding(H.OracleEncoding):
    def __init__(self, n_input_dims, encoding_config, dtype=torch.float32):
        c = dict(encoding_config)
        if c.get("otype") == "Grid":
            assert c.get("type", "Hash") == "Hash"
            c["otype"] = "HashGrid"
        super().__init__(n_input_dims, c, dtype)


sys.modules["tinycudann"].Encoding = GridHashEncoding
tnet.get_rank = lambda: torch.device("cpu")

GRID = {"n_levels": 16, "n_features_per_level": 2, "log2_hashmap_size": 19, "base_resolution": 16, "per_level_scale": 1.447269237440378}
BAND = {"otype": "ProgressiveBandHashGrid", **GRID, "start_level": 4, "start_step": 100, "update_steps": 50}
STEPS = [0, 99, 100, 149, 150, 400, 700, 5000]
ENC_LEVELS = {4: 100, 6: 200, 16: 700}          # level count -> a step at which the schedule has it
SEED, AMP = 43, 0.05


def sdf_geometry(band):
    return ImplicitSDF({"radius": 1.0, "normal_type": "finite_difference", "finite_difference_normal_eps": "progressive",
                        "pos_encoding_config": dict(band), "sdf_bias": "sphere", "sdf_bias_params": 0.5})


def make_band():
    geo = sdf_geometry(BAND)
    band = geo.encoding.encoding
    assert type(band).__name__ == "ProgressiveBandHashGrid"
    levels, masks, eps = [], [], []
    for step in STEPS:          # ascending: the reference's mask only grows
        geo.do_update_step(0, step)
        levels.append(int(band.current_level))
        masks.append(band.mask.numpy().copy())
        eps.append(float(geo.finite_difference_normal_eps))
    rng = np.random.default_rng(SEED + 3)
    x = rng.uniform(0.0, 1.0, (64, 3)).astype(np.float32)
    save = dict(steps=np.array(STEPS), current_level=np.array(levels), mask=np.stack(masks), fd_eps=np.array(eps, np.float64), seed=SEED, grid_amp=AMP,
                x=x, start_level=BAND["start_level"], start_step=BAND["start_step"], update_steps=BAND["update_steps"], radius=1.0)
    table = torch.from_numpy(grid_params(SEED, 12_599_920, AMP))
    with torch.no_grad():
        fresh = tnet.get_encoding(3, H._to_attr(dict(BAND)))
        fresh.encoding.encoding.params.copy_(table)
        save["enc_before_update"] = fresh(torch.from_numpy(x)).numpy()
        assert not save["enc_before_update"].any()
        for a, step in ENC_LEVELS.items():
            enc = tnet.get_encoding(3, H._to_attr(dict(BAND)))
            enc.encoding.encoding.params.copy_(table)
            enc.encoding.update_step(0, step)
            assert enc.encoding.current_level == a
            save[f"enc_{a}"] = enc(torch.from_numpy(x)).numpy()
    path = os.path.join(HERE, "progressive_band.npz")
    np.savez_compressed(path, **save)
    print(f"progressive_band: levels {levels}, eps {eps} -> {path} ({os.path.getsize(path) / 1e6:.3f} MB)")


STEP_D = 200            # 4 + (200 - 100) // 50 = 6 active levels


def build(spp, seed, grid_amp, ren_cfg):
    torch.manual_seed(seed)
    geo = sdf_geometry(BAND)
    mat = NoMaterial({"n_output_dims": 3, "color_activation": "sigmoid"})
    bg = NeuralEnvironmentMapBackground({"color_activation": "sigmoid", "random_aug": True, "random_aug_prob": 0.5, "dir_encoding_config": BG_ENC})
    ren = NeuSVolumeRenderer({"radius": 1.0, "num_samples_per_ray": spp, **ren_cfg}, geometry=geo, material=mat, background=bg)
    with torch.no_grad():
        geo.encoding.encoding.encoding.params.copy_(torch.from_numpy(grid_params(seed, 12_599_920, grid_amp)))
        bg.encoding.encoding.encoding.params.copy_(torch.from_numpy(grid_params(seed + 1, 1_581_184, 0.5)))
        for p in list(geo.sdf_network.parameters()) + list(geo.feature_network.parameters()):
            p.mul_(2.0)
    geo.do_update_step(0, STEP_D)           # the encoding's mask and the geometry's eps, as the system's per-step walk sets them
    assert geo.encoding.encoding.current_level == 6
    return geo, mat, bg, ren


if __name__ == "__main__":
    which = sys.argv[1:] or ["band", "d"]
    if "band" in which:
        make_band()
    if "d" in which:
        N.build = build
        geo, ren = N.make("neus_d_8x8x64_progressive", 8, 8, 64, seed=47, grid_amp=0.05, cam=(15.0, 70.0, 1.6, 50.0), ren_cfg={}, step=STEP_D, want=None)
        path = os.path.join(HERE, "neus_d_8x8x64_progressive.npz")
        g = dict(np.load(path))
        g.update(active_levels=6, fd_eps=np.float64(geo.finite_difference_normal_eps), start_level=BAND["start_level"], start_step=BAND["start_step"],
                 update_steps=BAND["update_steps"])
        gg = geo.encoding.encoding.encoding.params.grad.numpy()
        assert not gg[2 * int(geo.encoding.encoding.encoding.meta.offset[6]):].any()
        np.savez_compressed(path, **g)
        print(f"neus_d: eps {float(g['fd_eps'])} -> {path} ({os.path.getsize(path) / 1e6:.2f} MB)")
