"""Golden vectors of `textured-background` and `solid-color-background`: the REFERENCE's own classes
(threestudio/models/background/textured_background.py, solid_color_background.py), imported in place under ref_harness.py and run on the CPU.

  python tests/golden/make_goldens_background.py      # writes tests/golden/background_textured.npz and background_solid.npz

Inputs, colours, parameter gradients for a fixed d_color, and the two state dicts (keys and tensors).  The .npz files are data only.
"""
from __future__ import annotations

import os
import random
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import ref_harness as H  # noqa: E402

H.install()
import background_util as U  # noqa: E402

from threestudio.models.background.solid_color_background import SolidColorBackground  # noqa: E402
from threestudio.models.background.textured_background import TexturedBackground  # noqa: E402

TEXTURED = {"default": (3, 64, 64, 400, 11), "odd": (4, 5, 7, 300, 12)}       # name -> (C, H, W, random directions, seed)
SOLID_DIRS_SHAPE = (2, 4, 5, 3)
AUG_SEEDS = {"fire": (3, 21), "pass": (2, 22)}      # (random.seed, torch.manual_seed): the first random.random() is 0.238 (fires) / 0.956 (does not)


def make_textured():
    save = {}
    for name, (C, Ht, Wt, n, seed) in TEXTURED.items():
        dirs = U.with_special(U.random_dirs(n, seed))
        g = torch.Generator().manual_seed(seed + 100)
        d_color = torch.randn(dirs.shape[0], C, generator=g)
        save[f"{name}_dirs"], save[f"{name}_d_color"] = dirs.numpy(), d_color.numpy()
        for act in ("sigmoid", "none"):
            torch.manual_seed(seed)
            bg = TexturedBackground({"n_output_dims": C, "height": Ht, "width": Wt, "color_activation": act})
            color = bg(dirs)
            assert color.shape == (dirs.shape[0], C)
            (color * d_color).sum().backward()
            save[f"{name}_texture"] = bg.texture.detach().numpy().copy()          # the same seed: the same texture for both activations
            save[f"{name}_color_{act}"] = color.detach().numpy()
            save[f"{name}_grad_{act}"] = bg.texture.grad.numpy().copy()
    sd = TexturedBackground({}).state_dict()        # keys and shapes; default_texture[None] above is such a state dict's tensor
    save["sd_keys"] = np.array(sorted(sd))
    for k, v in sd.items():
        save["sd_shape/" + k] = np.array(v.shape)
    path = os.path.join(HERE, "background_textured.npz")
    np.savez_compressed(path, **save)
    print(f"textured -> {path} ({os.path.getsize(path) / 1e3:.1f} kB)")


def make_solid():
    save = {}
    g = torch.Generator().manual_seed(31)
    dirs = torch.nn.functional.normalize(torch.randn(*SOLID_DIRS_SHAPE, generator=g), dim=-1)
    d_color = torch.randn(*SOLID_DIRS_SHAPE[:-1], 3, generator=g)
    save["dirs"], save["d_color"] = dirs.numpy(), d_color.numpy()
    colour = (0.2, 0.5, 0.9)
    save["colour"] = np.array(colour, np.float32)

    def run(tag, cfg, seeds=None):
        bg = SolidColorBackground({"color": colour, **cfg})
        bg.train()
        if seeds is not None:
            random.seed(seeds[0])
            torch.manual_seed(seeds[1])
        out = bg(dirs)
        save[f"{tag}_color"] = out.detach().numpy()
        if cfg.get("learned"):
            (out * d_color).sum().backward()
            save[f"{tag}_grad"] = bg.env_color.grad.numpy().copy()
        if seeds is not None:       # the draws the call made, in its order: random.random() first, torch.rand only when it fires
            random.seed(seeds[0])
            torch.manual_seed(seeds[1])
            r = random.random()
            save[f"{tag}_seeds"], save[f"{tag}_rand"] = np.array(seeds), np.float64(r)
            fired = r < bg.cfg.random_aug_prob
            save[f"{tag}_fired"] = np.bool_(fired)
            if fired:
                save[f"{tag}_rand_color"] = torch.rand(dirs.shape[0], 1, 1, 3).numpy()
            save[f"{tag}_next_torch_draw"] = torch.rand(4).numpy()      # where the torch stream stands after the call
        return bg

    run("fixed", {"learned": False})
    bg = run("learned", {"learned": True})
    fire = run("aug_fire", {"learned": True, "random_aug": True, "random_aug_prob": 0.5}, AUG_SEEDS["fire"])
    run("aug_pass", {"learned": True, "random_aug": True, "random_aug_prob": 0.5}, AUG_SEEDS["pass"])
    assert bool(save["aug_fire_fired"]) and not bool(save["aug_pass_fired"]), (save["aug_fire_rand"], save["aug_pass_rand"])
    assert not fire.env_color.grad.any()                    # `color * 0 +`: in the graph, zero gradient
    fire.eval()
    random.seed(AUG_SEEDS["fire"][0])
    save["aug_eval_color"] = fire(dirs).detach().numpy()     # training = False never augments
    for tag, m in (("learned", bg), ("fixed", SolidColorBackground({"color": colour}))):
        sd = m.state_dict()
        save[f"sd_{tag}_keys"] = np.array(sorted(sd))
        for k, v in sd.items():
            save[f"sd_{tag}/" + k] = v.numpy()
    save["sd_learned_is_parameter"] = np.bool_(isinstance(bg.env_color, torch.nn.Parameter))
    path = os.path.join(HERE, "background_solid.npz")
    np.savez_compressed(path, **save)
    print(f"solid -> {path} ({os.path.getsize(path) / 1e3:.1f} kB); draws {save['aug_fire_rand']:.4f} {save['aug_pass_rand']:.4f}")


if __name__ == "__main__":
    make_textured()
    make_solid()
