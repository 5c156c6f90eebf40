"""Goldens of the validation / test passes from the REFERENCE's own code (build container only):
  threestudio/data/uncond.py:347-467            RandomCameraDataset, both splits, with the SV and MV eval settings of make_goldens_camera.py
  custom/amortized/data/multiprompt.py:85-164   MultipromptRandomCameraDataset4Test (seeded noises), ...4FixPrompt (item keys)
  threestudio/utils/saving.py:77-109,179-299    SaverMixin.get_image_grid_ on the panels of test_step (scaledreamer.py:252-304)
saving.py imports cv2, imageio, wandb, matplotlib, trimesh and pytorch_lightning.loggers at module level; none of them is needed by
get_image_grid_ for equal-sized rgb / grey panels except cv2.cvtColor, which only reverses the channel order there.  They are stubbed
here (the harness is left as it is).    python tests/golden/make_goldens_views.py  ->  tests/golden/{eval_views,image_grid}.npz
"""
import importlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_harness as H  # noqa: E402
import make_goldens_camera as MC  # noqa: E402  (installs the harness, stubs pl.LightningDataModule; SV / MV settings)

H.install_amortized()
m = H._mod("custom.amortized.data")
m.__path__ = [os.path.join(H.REFERENCE, "custom", "amortized", "data")]


def _stub_saving_imports():
    H._mod("cv2", cvtColor=lambda img, code: img[..., ::-1], COLOR_RGB2BGR=0, COLOR_RGBA2BGRA=1, COLOR_BGR2RGB=2)
    H._mod("pytorch_lightning.loggers", WandbLogger=object)
    for name in ("imageio", "wandb", "matplotlib", "trimesh"):
        try:
            importlib.import_module(name)
        except ImportError:
            H._mod(name)
    if not hasattr(sys.modules["matplotlib"], "__file__"):
        sys.modules["matplotlib"].__path__ = []
        H._mod("matplotlib.pyplot")
        H._mod("matplotlib.cm")
        sys.modules["matplotlib"].cm = sys.modules["matplotlib.cm"]
        H._mod("matplotlib.colors", LinearSegmentedColormap=object)


EVAL = dict(eval_height=6, eval_width=9, n_val_views=4, n_test_views=5)
LIBRARY = {"train": ["a red car", "a blue house."], "val": ["a zoomed out DSLR photo of a hamburger", "an owl, carved from wood."]}
FIX = dict(eval_prompt="a red car", n_test_views=5, dim_gaussian=8, eval_height=6, eval_width=9)


def eval_views():
    from threestudio.data.uncond import RandomCameraDataModuleConfig, RandomCameraDataset
    from threestudio.data.uncond_multiview import RandomMultiviewCameraDataModuleConfig
    from custom.amortized.data.multiprompt import (MultipromptRandomCameraDataModuleConfig, MultipromptRandomCameraDataset4FixPrompt,
                                                   MultipromptRandomCameraDataset4Test)

    out = {}
    for tag, cfg_cls, base in (("sv", RandomCameraDataModuleConfig, MC.SV), ("mv", RandomMultiviewCameraDataModuleConfig, MC.MV)):
        c = dict(base)
        c.update(EVAL)
        for split in ("val", "test"):
            ds = RandomCameraDataset(cfg_cls(**c), split)
            batch = ds.collate([ds[i] for i in range(len(ds))])
            for k, v in batch.items():
                out[f"{tag}.{split}.{k}"] = v.numpy() if torch.is_tensor(v) else np.asarray(v)
    torch.manual_seed(7)
    ds = MultipromptRandomCameraDataset4Test(MultipromptRandomCameraDataModuleConfig(dim_gaussian=8, **EVAL), "test", LIBRARY)
    out["mp4test.seed"], out["mp4test.noises"] = np.asarray(7), ds.noises.numpy()
    out["mp4test.prompts"] = np.asarray([b["prompt"][0] for b in ds])      # no "test" split: the "val" prompts
    b = ds.collate({"prompt": [LIBRARY["val"][0]]})
    out["mp4test.batch_noise"], out["mp4test.batch_index"], out["mp4test.batch_azimuth"] = b["noise"].numpy(), b["index"].numpy(), b["azimuth"].numpy()
    for tag, extra in (("plain", {}), ("target", dict(target_prompt="a blue house.")),
                       ("target_cam", dict(target_prompt="a blue house.", eval_fix_camera=3))):
        ds = MultipromptRandomCameraDataset4FixPrompt(MultipromptRandomCameraDataModuleConfig(**FIX, **extra), "test")
        items = [ds[i] for i in range(ds.n_views)]
        out[f"mpfix.{tag}.index"] = np.asarray([it["index"] for it in items])
        out[f"mpfix.{tag}.name"] = np.asarray([it["name"] for it in items])
        out[f"mpfix.{tag}.prompt"] = np.asarray([it["prompt"] for it in items])
        out[f"mpfix.{tag}.noise"] = np.stack([it["noise"].numpy() for it in items])
        out[f"mpfix.{tag}.azimuth"] = np.stack([it["azimuth"].numpy() for it in items])
        out[f"mpfix.{tag}.c2w"] = np.stack([it["c2w"].numpy() for it in items])
        if "ratio" in items[0]:
            out[f"mpfix.{tag}.ratio"] = np.stack([it["ratio"].numpy() for it in items])
            out[f"mpfix.{tag}.prompt_target"] = np.asarray([it["prompt_target"] for it in items])
    np.savez_compressed(os.path.join(HERE, "eval_views.npz"), **out)


def image_grid():
    _stub_saving_imports()
    from threestudio.utils.saving import SaverMixin

    rng = np.random.default_rng(11)
    B, Hh, W = 2, 5, 7
    rgb = rng.uniform(-0.2, 1.2, (B, Hh, W, 3)).astype(np.float32)
    normal = rng.uniform(0.0, 1.0, (B, Hh, W, 3)).astype(np.float32)
    opacity = rng.uniform(0.0, 1.0, (B, Hh, W, 1)).astype(np.float32)
    opacity[0, 0, :3, 0], opacity[1, 2, 2:5, 0] = 0.0, 1.0
    depth = rng.uniform(0.0, 3.0, (B, Hh, W, 1)).astype(np.float32)
    depth[0][opacity[0] < 0.3] = 0.0
    depth[1] = 1.7                                  # a constant image: 0 / 0 in the normalisation
    out = {k: torch.from_numpy(v) for k, v in (("comp_rgb", rgb), ("comp_normal", normal), ("opacity", opacity), ("depth", depth))}
    saver = SaverMixin()

    def step_panels(b, with_normal):                # the list test_step builds (scaledreamer.py:256-301)
        d = out["depth"][b, :, :, 0]
        d = (d - d.min()) / (d.max() - d.min())
        return ([{"type": "rgb", "img": out["comp_rgb"][b], "kwargs": {"data_format": "HWC"}}]
                + ([{"type": "rgb", "img": out["comp_normal"][b], "kwargs": {"data_format": "HWC", "data_range": (0, 1)}}] if with_normal else [])
                + [{"type": "grayscale", "img": out["opacity"][b, :, :, 0], "kwargs": {"cmap": None, "data_range": (0, 1)}},
                   {"type": "grayscale", "img": d, "kwargs": {"cmap": None, "data_range": (0, 1)}}])

    to_rgb = lambda a: np.ascontiguousarray(a[..., ::-1])
    with np.errstate(all="ignore"):
        grid4 = np.stack([to_rgb(saver.get_image_grid_(step_panels(b, True), align="max")) for b in range(B)])
        grid3 = np.stack([to_rgb(saver.get_image_grid_(step_panels(b, False), align="max")) for b in range(B)])
        rows2 = to_rgb(saver.get_image_grid_([step_panels(0, False)[:2], step_panels(1, False)[:2]], align="max"))
    assert grid4.shape == (B, Hh, 4 * W, 3) and grid3.shape == (B, Hh, 3 * W, 3) and rows2.shape == (2 * Hh, 2 * W, 3) and grid4.dtype == np.uint8
    np.savez_compressed(os.path.join(HERE, "image_grid.npz"), rgb=rgb, normal=normal, opacity=opacity, depth=depth, grid4=grid4, grid3=grid3,
                        rows2=rows2)


if __name__ == "__main__":
    eval_views()
    image_grid()
    print("view goldens written")
