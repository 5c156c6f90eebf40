"""Wall time of the single-prompt test pass at the shipped size: `asd_sd_nerf` with seeded random weights, system.test() over
120 views at 512 x 512, and the share of it spent in the two entries of csrc/image.hip (asd_image_minmax_f32 + asd_image_grid_u8).

    python tools/views_time.py [--views 120] [--size 512]

Two passes after a warm-up of three views: the first is timed as a whole (host clock around a device synchronise); in the second, the grid
composition (saving.compose) is bracketed by device synchronises and its time summed, as is the PNG writing.  One JSON line."""
import argparse
import json
import os
import random
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=120)
    ap.add_argument("--size", type=int, default=512)
    a = ap.parse_args()
    from scaledreamer_amd import presets, saving
    from scaledreamer_amd.registry import find
    import scaledreamer_amd.plugins  # noqa: F401

    presets.ALLOW_RANDOM_WEIGHTS = True
    torch.manual_seed(5)
    random.seed(5)
    cfg = presets.asd_sd_nerf()
    cfg["system"]["guidance_type"] = ""
    system = find(cfg["system_type"])(cfg["system"])
    system.train()
    with torch.no_grad():
        system.geometry.encoding.encoding.encoding.params.uniform_(-0.2, 0.2)
        system.background.encoding.encoding.encoding.params.uniform_(-0.5, 0.5)
    system.on_train_batch_start()

    def datamodule(n):
        d = dict(cfg["data"])
        d.update(eval_height=a.size, eval_width=a.size, n_test_views=n)
        return find(cfg["data_type"])(d)

    with tempfile.TemporaryDirectory() as tmp:
        system.test(datamodule(3).test_dataset(), os.path.join(tmp, "warm"))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        system.test(datamodule(a.views).test_dataset(), os.path.join(tmp, "whole"))
        torch.cuda.synchronize()
        whole = time.perf_counter() - t0

        spent = {"compose": 0.0, "png": 0.0}

        def bracket(fn, key):
            def timed(*args, **kw):
                torch.cuda.synchronize()
                t = time.perf_counter()
                out = fn(*args, **kw)
                torch.cuda.synchronize()
                spent[key] += time.perf_counter() - t
                return out
            return timed

        compose, write_png = saving.compose, saving.write_png
        saving.compose, saving.write_png = bracket(compose, "compose"), bracket(write_png, "png")
        try:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            system.test(datamodule(a.views).test_dataset(), os.path.join(tmp, "split"))
            torch.cuda.synchronize()
            split = time.perf_counter() - t0
        finally:
            saving.compose, saving.write_png = compose, write_png
    print(json.dumps({"views": a.views, "size": a.size, "test_pass_s": round(whole, 3), "bracketed_pass_s": round(split, 3),
                      "image_entries_s": round(spent["compose"], 4), "image_entries_share": round(spent["compose"] / split, 5),
                      "png_write_s": round(spent["png"], 3), "imageio": "imageio" in sys.modules}))


if __name__ == "__main__":
    main()
