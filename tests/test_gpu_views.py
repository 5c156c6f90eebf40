"""Validation / test passes on the device: asd_image_minmax_f32 and asd_image_grid_u8 (csrc/image.hip) against torch, against the
reference's bytes (tests/golden/image_grid.npz) and against the CPU restatement (saving.grid_cpu, itself pinned to those bytes by
tests/test_views_cpu.py); the evaluation rays; and the two systems' validate() / test() end to end.  Every comparison of bytes is exact:
the arithmetic is fp32 without contraction and with IEEE division on both sides."""
import os
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")


# ---- asd_image_minmax_f32 -----------------------------------------------------------------------------------------------------------------
def _minmax_input(n_images, n_per_image):
    g = torch.Generator().manual_seed(n_images * 1000003 + n_per_image)
    x = torch.randn(n_images, n_per_image, generator=g) * 3.0
    if (n_images, n_per_image) == (2, 130 * 67):          # the extrema in the last element of one image and the first of the other
        x[0, -1], x[0, 0] = 50.0, -40.0
        x[1, 0], x[1, -1] = 60.0, -70.0
    return x


@pytest.mark.parametrize("n_images,n_per_image", [(1, 1), (3, 35), (2, 130 * 67), (1, 512 * 512)])
def test_image_minmax_is_exact(n_images, n_per_image):
    from scaledreamer_amd import ops

    x = _minmax_input(n_images, n_per_image)
    buf = torch.full((2 * n_images + 16,), 7.5, device="cuda")
    out = buf[8:8 + 2 * n_images].view(n_images, 2)
    got = ops.image_minmax(x.cuda(), out=out)
    want = torch.stack([x.amin(dim=1), x.amax(dim=1)], dim=1)
    assert got.data_ptr() == out.data_ptr() and torch.equal(got.cpu(), want)
    assert bool((buf[:8] == 7.5).all()) and bool((buf[8 + 2 * n_images:] == 7.5).all()), "guard floats around minmax"
    if (n_images, n_per_image) == (2, 130 * 67):
        assert want.tolist() == [[-40.0, 50.0], [-70.0, 60.0]]
    # an image that does not start on a 16-byte boundary (a view at an odd float offset) goes through the same head / body / tail split
    if n_per_image > 8:
        y = torch.cat([torch.zeros(1), x.reshape(-1)]).cuda()[1:].view(n_images, n_per_image)
        assert y.data_ptr() % 16 == 4 and torch.equal(ops.image_minmax(y).cpu(), want)


@pytest.mark.parametrize("n_per_image", [35, 512 * 512])
def test_image_minmax_nan_poisons_its_image_only(n_per_image):
    from scaledreamer_amd import ops

    x = _minmax_input(3, n_per_image)
    x[1, n_per_image // 2] = float("nan")
    got = ops.image_minmax(x.cuda()).cpu()
    assert bool(torch.isnan(got[1]).all())
    assert torch.equal(got[[0, 2]], torch.stack([x.amin(dim=1), x.amax(dim=1)], dim=1)[[0, 2]])
    assert torch.equal(torch.isnan(got), torch.isnan(torch.stack([x.amin(dim=1), x.amax(dim=1)], dim=1)))     # torch's own NaN rule


def test_image_minmax_refuses_empty_images():
    from scaledreamer_amd import _lib, ops

    with pytest.raises(_lib.AsdError, match="n_per_image"):
        ops.image_minmax(torch.zeros(2, 0, device="cuda"))


# ---- asd_image_grid_u8 --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLD, "image_grid.npz"))


def _gold_panels(g, with_normal, dev="cuda"):
    t = lambda k: torch.from_numpy(g[k]).to(dev)
    return ([("rgb", t("rgb"), 0.0, 1.0, False)] + ([("rgb", t("normal"), 0.0, 1.0, False)] if with_normal else [])
            + [("grayscale", t("opacity")[..., 0], 0.0, 1.0, False), ("grayscale", t("depth")[..., 0], 0.0, 1.0, True)])


@pytest.mark.parametrize("key,with_normal", [("grid4", True), ("grid3", False)])
def test_image_grid_matches_reference_bytes(gold, key, with_normal):
    from scaledreamer_amd import ops

    got = ops.image_grid(_gold_panels(gold, with_normal))
    assert got.dtype == torch.uint8 and got.is_cuda
    np.testing.assert_array_equal(got.cpu().numpy(), gold[key])
    assert not got[1, :, -7:].any(), "a constant depth image gives an all-zero panel"


def _random_panels(B, H, W, P, seed):
    g = torch.Generator().manual_seed(seed)
    kinds = [("rgb", -0.2, 1.2, 0.0, 1.0, False), ("grayscale", 0.0, 3.0, 0.0, 1.0, True), ("grayscale", -0.1, 1.1, 0.0, 1.0, False),
             ("rgb", -1.5, 1.5, -1.0, 1.0, False)][:P]
    out = []
    for kind, a, b, lo, hi, nz in kinds:
        shape = (B, H, W, 3) if kind == "rgb" else (B, H, W)
        out.append((kind, torch.rand(shape, generator=g) * (b - a) + a, lo, hi, nz))
    return out


@pytest.mark.parametrize("B,H,W,P", [(1, 1, 1, 1), (2, 5, 7, 3), (3, 33, 130, 4), (1, 512, 512, 4)])
def test_image_grid_matches_cpu_restatement(B, H, W, P):
    """(1,1,1,1): one pixel, no whole dword; (2,5,7,3): rows of 63 bytes, off dword alignment from the second row on, and 210 pixels = 52
    groups of four + 2 single pixels; (3,33,130,4): several blocks; (1,512,512,4): the shipped view size, past the grid cap's first trip"""
    from scaledreamer_amd import ops
    from scaledreamer_amd.saving import grid_cpu

    panels = _random_panels(B, H, W, P, seed=B * 7 + W)
    want = grid_cpu(panels)
    n = want.numel()
    buf = torch.full((n + 32,), 0xA5, dtype=torch.uint8, device="cuda")
    out = buf[16:16 + n].view(B, H, P * W, 3)
    got = ops.image_grid([(k, s.cuda(), lo, hi, nz) for k, s, lo, hi, nz in panels], out=out)
    assert tuple(got.shape) == (B, H, P * W, 3) and torch.equal(got.cpu(), want)
    assert bool((buf[:16] == 0xA5).all()) and bool((buf[16 + n:] == 0xA5).all()), "guard bytes around out"


def test_image_grid_special_values():
    from scaledreamer_amd import ops
    from scaledreamer_amd.saving import grid_cpu

    inf, nan = float("inf"), float("nan")
    gray = torch.tensor([[[inf, -inf, nan, 0.25, 1.0]]])
    rgb = torch.tensor([[[[nan, 0.5, 2.0], [nan, nan, nan], [0.0, 1.0, -1.0], [0.999, 0.001, 0.5], [nan, 0.0, nan]]]])
    panels = [("grayscale", gray, 0.0, 1.0, False), ("rgb", rgb, 0.0, 1.0, False), ("grayscale", torch.full((1, 1, 5), 2.5), 0.0, 1.0, True)]
    got = ops.image_grid([(k, s.cuda(), lo, hi, nz) for k, s, lo, hi, nz in panels]).cpu()
    assert got[0, 0, :5, 0].tolist() == [255, 0, 0, 63, 255] and torch.equal(got[0, 0, :5, 0], got[0, 0, :5, 2])     # +-inf -> 255 / 0
    assert got[0, 0, 5].tolist() == [0, 127, 255] and got[0, 0, 6].tolist() == [0, 0, 0] and got[0, 0, 9].tolist() == [0, 0, 0]    # rgb NaN -> 0
    assert not got[0, 0, 10:].any()                                                                                  # constant: all zero
    assert torch.equal(got, grid_cpu(panels))


def test_image_grid_refusals():
    from scaledreamer_amd import _lib, ops

    g = torch.zeros(1, 2, 2, device="cuda")
    with pytest.raises(_lib.AsdError, match="unequal size"):
        ops.image_grid([("grayscale", g, 0.0, 1.0, False), ("grayscale", torch.zeros(1, 2, 3, device="cuda"), 0.0, 1.0, False)])
    with pytest.raises(_lib.AsdError, match="lo < hi"):
        ops.image_grid([("grayscale", g, 1.0, 1.0, False)])
    with pytest.raises(_lib.AsdError, match="1 to 8 panels"):
        ops.image_grid([("grayscale", g, 0.0, 1.0, False)] * 9)
    with pytest.raises(_lib.AsdError, match="device tensors"):
        ops.image_grid([("grayscale", g.cpu(), 0.0, 1.0, False)])


# ---- evaluation rays ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["sv", "mv"])
def test_eval_rays_match_reference(tag):
    from test_views_cpu import EVAL, _datamodule

    views = np.load(os.path.join(GOLD, "eval_views.npz"))
    dm = _datamodule(tag)
    for split, ds in (("val", dm.val_dataset()), ("test", dm.test_dataset())):
        batches = list(ds)
        assert len(batches) == (EVAL["n_val_views"] if split == "val" else EVAL["n_test_views"])
        for i, b in enumerate(batches):
            assert b["rays_o"].is_cuda and b["rays_d"].is_cuda and tuple(b["rays_o"].shape) == (1, 6, 9, 3) and b["index"].tolist() == [i]
            assert "focal_length" not in b and (b["height"], b["width"]) == (6, 9)
            for k in ("rays_o", "rays_d"):
                np.testing.assert_allclose(b[k][0].cpu().numpy(), views[f"{tag}.{split}.{k}"][i], rtol=2e-6, atol=2e-6, err_msg=f"{tag} {split} {k} {i}")
        item = ds[1]
        assert item["index"] == 1 and tuple(item["rays_d"].shape) == (6, 9, 3) and torch.equal(item["rays_d"], batches[1]["rays_d"][0])


# ---- end to end ---------------------------------------------------------------------------------------------------------------------------
def _png(path):
    from PIL import Image

    with Image.open(path) as im:
        assert im.mode == "RGB"
        return np.asarray(im).copy()


def _sequence_frames(path):
    """frames of the written sequence: a GIF where imageio is missing (then the path says so)"""
    from PIL import Image

    assert os.path.exists(path) and path.endswith((".gif", ".mp4"))
    if path.endswith(".mp4"):
        import imageio

        return len(imageio.mimread(path))
    with Image.open(path) as im:
        return im.n_frames


@pytest.fixture(scope="module")
def single():
    from scaledreamer_amd import presets
    from scaledreamer_amd.registry import find
    import scaledreamer_amd.plugins  # noqa: F401

    torch.manual_seed(5)
    random.seed(5)
    cfg = presets.asd_sd_nerf()
    cfg["system"]["guidance_type"] = ""
    cfg["data"].update(eval_height=32, eval_width=32, n_test_views=3, n_val_views=2)
    system = find(cfg["system_type"])(cfg["system"])
    system.train()
    with torch.no_grad():
        system.geometry.encoding.encoding.encoding.params.uniform_(-0.2, 0.2)
        system.background.encoding.encoding.encoding.params.uniform_(-0.5, 0.5)
    system.on_train_batch_start()            # occupancy grid from this field (step 0: all cells)
    return system, find(cfg["data_type"])(cfg["data"])


def test_single_prompt_test_pass(single, tmp_path):
    from scaledreamer_amd import ops

    system, dm = single
    system.train()
    paths = system.test(dm.test_dataset(), str(tmp_path))
    assert system.training, "the training flag is restored"
    pngs = [str(tmp_path / "it0-test" / f"{i}.png") for i in range(3)]
    assert paths[:3] == pngs and len(paths) == 4 and os.path.dirname(paths[3]) == str(tmp_path) and os.path.basename(paths[3]).startswith("it0-test.")
    assert _sequence_frames(paths[3]) == 3
    system.eval()
    try:
        for i, batch in enumerate(dm.test_dataset()):
            with torch.no_grad():
                out = system({k: (v.cuda() if torch.is_tensor(v) else v) for k, v in batch.items()})
            want = ops.image_grid([("rgb", out["comp_rgb"], 0.0, 1.0, False), ("rgb", out["comp_normal"], 0.0, 1.0, False),
                                   ("grayscale", out["opacity"][..., 0], 0.0, 1.0, False), ("grayscale", out["depth"][..., 0], 0.0, 1.0, True)])
            got = _png(pngs[i])
            assert got.shape == (32, 128, 3)
            np.testing.assert_array_equal(got, want[0].cpu().numpy())        # eval draws no jitter: the second forward is the first
            first = (out["comp_rgb"][0].clamp(0.0, 1.0) * 255.0).to(torch.int32).to(torch.uint8)
            np.testing.assert_array_equal(got[:, :32], first.cpu().numpy())
            assert got[:, :32].std() > 0 and got[:, 96:].max() == 255, "a rendered picture, a depth panel that spans its range"
    finally:
        system.train()


def test_single_prompt_validate_layouts(single, tmp_path):
    system, dm = single
    system.train()
    system.cfg.validation_via_video = False
    paths = system.validate(dm.val_dataset(), str(tmp_path / "a"))
    assert paths == [str(tmp_path / "a" / f"it0-{i}.png") for i in range(2)] and all(os.path.exists(p) for p in paths)
    assert sorted(os.listdir(tmp_path / "a")) == ["it0-0.png", "it0-1.png"] and _png(paths[0]).shape == (32, 128, 3)
    system.cfg.validation_via_video = True
    try:
        paths = system.validate(dm.val_dataset(), str(tmp_path / "b"))
    finally:
        system.cfg.validation_via_video = False
    assert len(paths) == 1 and os.listdir(tmp_path / "b") == [os.path.basename(paths[0])] and os.path.basename(paths[0]).startswith("it0-val.")
    assert _sequence_frames(paths[0]) == 2 and system.training
    system.cfg.visualize_samples = True
    try:
        with pytest.raises(NotImplementedError):
            system.validate(dm.val_dataset(), str(tmp_path / "c"))
    finally:
        system.cfg.visualize_samples = False
    assert system.training


PROMPTS = ["a red car, shiny.", "an owl carved from wood"]


def _multi(extra_data=None, **system_kw):
    from scaledreamer_amd import presets
    from scaledreamer_amd.multiprompt import SyntheticMultiPromptProcessor
    from scaledreamer_amd.registry import find
    import scaledreamer_amd.plugins  # noqa: F401

    torch.manual_seed(0)
    random.seed(0)
    dev = torch.device("cuda", 0)
    cfg = presets.asd_sd_hyper_ingp(PROMPTS)
    cfg["system"]["guidance_type"] = ""
    cfg["system"].update(system_kw)
    cfg["data"].update(eval_height=16, eval_width=16, n_test_views=2, n_val_views=2, prompt_library={"train": PROMPTS, "val": PROMPTS, "test": PROMPTS})
    cfg["data"].update(extra_data or {})
    proc = SyntheticMultiPromptProcessor(PROMPTS, seed=2, device=dev, ctx_dim=128, global_dim=1024)
    system = find(cfg["system_type"])(cfg["system"], prompt_processor=proc)
    system.train()
    system.on_train_batch_start()            # the per-step update a trained (or loaded) system has had; the drivers themselves run none
    return system, find(cfg["data_type"])(cfg["data"], rank=0, n_ranks=1)


def test_multi_prompt_test_pass(tmp_path):
    system, dm = _multi()
    paths = system.test(dm.test_dataset(), str(tmp_path))
    names = ["a_red_car_shiny", "an_owl_carved_from_wood"]
    want = [str(tmp_path / "it0-test" / n / f"{i}.png") for n in names for i in range(2)]
    assert paths[:4] == want and len(paths) == 6 and system.training
    for n, seq in zip(names, paths[4:]):
        assert os.path.dirname(seq) == str(tmp_path / "it0-test") and os.path.basename(seq).startswith(n + ".") and _sequence_frames(seq) == 2
    imgs = [_png(p) for p in want]
    assert all(im.shape[0] == 16 and im.shape[1] % 16 == 0 and im.shape[1] >= 48 for im in imgs)
    assert not np.array_equal(imgs[0], imgs[2]), "two prompts, two pictures"
    # views rendered in slices give the same files
    system.EVAL_VIEWS_PER_CALL = 1
    again = system.test(dm.test_dataset(), str(tmp_path / "sliced"))
    for a, b in zip(want, again[:4]):
        np.testing.assert_array_equal(_png(a), _png(b))


def test_multi_prompt_interpolation_and_validation(tmp_path):
    system, dm = _multi(dict(eval_prompt=PROMPTS[0], target_prompt=PROMPTS[1]))
    paths = system.test(dm.test_dataset(), str(tmp_path))
    d = tmp_path / "it0-test" / "a_red_car_shiny_to_an_owl_carved_from_wood"
    assert paths[:2] == [str(d / "0.png"), str(d / "1.png")] and len(paths) == 3 and _sequence_frames(paths[2]) == 2
    assert not np.array_equal(_png(paths[0]), _png(paths[1])), "ratio 0 and ratio 1 at two azimuths"
    # validation: it{step}-val/<name>/ with the video option (the preset's), it{step}/<name>/ without; the frames stay
    paths = system.validate(dm.val_dataset(), str(tmp_path / "v"))
    assert len(paths) == 6 and sorted(os.listdir(tmp_path / "v")) == ["it0-val"]
    assert os.path.isdir(tmp_path / "v" / "it0-val" / "a_red_car_shiny") and all(os.path.exists(p) for p in paths)
    system.cfg.validation_via_video = False
    paths = system.validate(dm.val_dataset(), str(tmp_path / "w"))
    assert paths == [str(tmp_path / "w" / "it0" / n / f"{i}.png") for n in ("a_red_car_shiny", "an_owl_carved_from_wood") for i in range(2)]


def test_multi_prompt_rgb_as_latents_is_refused(tmp_path):
    system, dm = _multi(rgb_as_latents=True)
    with pytest.raises(NotImplementedError, match="decode_latents"):
        system.test(dm.test_dataset(), str(tmp_path))
    assert system.training
