"""Validation / test passes, host side: the evaluation datasets against the reference's own (tests/golden/eval_views.npz), the torch
restatement of the image grid against the reference's get_image_grid_ (tests/golden/image_grid.npz, byte for byte), PNG and sequence
writing, and what is refused.  Goldens: tests/golden/make_goldens_views.py."""
import os

import numpy as np
import pytest
import torch

GOLD = os.path.join(os.path.dirname(__file__), "golden")
SV = dict(batch_size=[2, 1], width=[16, 32], height=[16, 32], resolution_milestones=[10000], camera_distance_range=[1.0, 1.5],
          fovy_range=[40, 70], elevation_range=[-10, 45], camera_perturb=0.0, center_perturb=0.0, up_perturb=0.0,
          eval_camera_distance=1.2, eval_fovy_deg=70.0, n_val_views=30)
MV = dict(batch_size=[8, 4], n_view=4, width=[16, 32], height=[16, 32], resolution_milestones=[10000],
          camera_distance_range=[0.8, 1.0], fovy_range=[15, 60], elevation_range=[0, 30], camera_perturb=0.0, center_perturb=0.0,
          up_perturb=0.0, eval_camera_distance=3.0, eval_fovy_deg=40.0, n_val_views=30)
EVAL = dict(eval_height=6, eval_width=9, n_val_views=4, n_test_views=5)
HOST_KEYS = ["mvp_mtx", "c2w", "camera_positions", "light_positions", "elevation", "azimuth", "camera_distances", "fovy", "proj_mtx"]
LIBRARY = {"train": ["a red car", "a blue house."], "val": ["a zoomed out DSLR photo of a hamburger", "an owl, carved from wood."]}


@pytest.fixture(scope="module")
def views():
    return np.load(os.path.join(GOLD, "eval_views.npz"))


@pytest.fixture(scope="module")
def grids():
    return np.load(os.path.join(GOLD, "image_grid.npz"))


def _datamodule(tag):
    import scaledreamer_amd.data  # noqa: F401
    from scaledreamer_amd.registry import find

    cfg = dict(SV if tag == "sv" else MV)
    cfg.update(EVAL)
    return find("random-camera-datamodule" if tag == "sv" else "mvdream-random-multiview-camera-datamodule")(cfg)


@pytest.mark.parametrize("tag", ["sv", "mv"])
@pytest.mark.parametrize("split", ["val", "test"])
def test_eval_cameras_match_reference(views, tag, split):
    dm = _datamodule(tag)
    ds = dm.val_dataset() if split == "val" else dm.test_dataset()
    n = EVAL["n_val_views"] if split == "val" else EVAL["n_test_views"]
    assert len(ds) == n
    b = ds.cameras(range(n))
    for k in HOST_KEYS:
        want = views[f"{tag}.{split}.{k}"]
        assert b[k].dtype == torch.float32 and tuple(b[k].shape) == want.shape, k
        np.testing.assert_allclose(b[k].numpy(), want, rtol=2e-6, atol=2e-6, err_msg=f"{tag} {split} {k}")
    assert b["index"].dtype == torch.int64 and b["index"].tolist() == views[f"{tag}.{split}.index"].tolist() == list(range(n))
    assert b["height"] == int(views[f"{tag}.{split}.height"]) == 6 and b["width"] == int(views[f"{tag}.{split}.width"]) == 9
    # the reference's collated batch has these keys and the rays; nothing else
    assert set(b) - {"focal_length"} | {"rays_o", "rays_d"} == {k.split(".", 2)[2] for k in views.files if k.startswith(f"{tag}.{split}.")}
    # the rays of these cameras, through the oracle's restatement of asd_generate_rays
    from oracle import oracle as O

    ro, rd = O.generate_rays(b["c2w"].numpy(), b["focal_length"].numpy(), 6, 9, True)
    np.testing.assert_allclose(ro, views[f"{tag}.{split}.rays_o"], rtol=2e-6, atol=2e-6)
    np.testing.assert_allclose(rd, views[f"{tag}.{split}.rays_d"], rtol=2e-6, atol=2e-6)
    one = ds.cameras([n - 1])
    assert one["index"].tolist() == [n - 1] and torch.equal(one["c2w"][0], b["c2w"][n - 1])


def test_eval_azimuth_ends():
    dm = _datamodule("sv")
    test, val = dm.test_dataset().host["azimuth"], dm.val_dataset().host["azimuth"]
    assert float(test[0]) == 0.0 and float(test[-1]) == 360.0
    assert float(val[0]) == 0.0 and float(val.max()) == 270.0


def test_eval_batch_size_other_than_one_is_refused():
    import scaledreamer_amd.data  # noqa: F401
    from scaledreamer_amd.registry import find

    dm = find("random-camera-datamodule")(dict(SV, eval_batch_size=2))
    with pytest.raises(ValueError, match="eval_batch_size"):
        dm.test_dataset()


def _mp(extra=None, name="multiprompt-camera-datamodule", rank=0, n_ranks=1):
    import scaledreamer_amd.multiprompt  # noqa: F401
    from scaledreamer_amd.registry import find

    cfg = dict(dim_gaussian=8, prompt_library=LIBRARY, **EVAL)
    cfg.update(extra or {})
    return find(name)(cfg, rank=rank, n_ranks=n_ranks)


@pytest.mark.parametrize("name", ["multiprompt-camera-datamodule", "multiprompt-multiview-camera-datamodule"])
def test_multiprompt_test_set_reproduces_noise_and_prompts(views, name):
    from scaledreamer_amd.multiprompt import MultipromptRandomCameraDataset4Test

    dm = _mp(name=name)
    torch.manual_seed(int(views["mp4test.seed"]))
    ds = dm.test_dataset()
    assert isinstance(ds, MultipromptRandomCameraDataset4Test) and isinstance(dm.val_dataset(), MultipromptRandomCameraDataset4Test)
    np.testing.assert_array_equal(ds.noises.numpy(), views["mp4test.noises"])
    assert ds.prompt_library == views["mp4test.prompts"].tolist() == LIBRARY["val"] and len(ds) == 2      # no "test" split: "val"
    cam = ds.dataset.cameras(range(ds.n_views))
    assert cam["index"].tolist() == views["mp4test.batch_index"].tolist()
    np.testing.assert_allclose(cam["azimuth"].numpy(), views["mp4test.batch_azimuth"], rtol=2e-6, atol=2e-6)
    np.testing.assert_array_equal(ds.noises[0][None].numpy(), views["mp4test.batch_noise"])
    # one batch per prompt of the rank's shard
    assert _mp(name=name, rank=1, n_ranks=2).val_dataset().prompt_library == LIBRARY["val"][1::2]


@pytest.mark.parametrize("tag,extra", [("plain", {}), ("target", dict(target_prompt="a blue house.")),
                                       ("target_cam", dict(target_prompt="a blue house.", eval_fix_camera=3))])
def test_multiprompt_fix_prompt_items(views, tag, extra):
    from scaledreamer_amd.multiprompt import MultipromptRandomCameraDataset4FixPrompt

    ds = _mp(dict(eval_prompt="a red car", **extra)).test_dataset()
    assert isinstance(ds, MultipromptRandomCameraDataset4FixPrompt) and len(ds) == 5
    items = [ds.host_item(i) for i in range(len(ds))]
    g = lambda k: views[f"mpfix.{tag}.{k}"]
    assert [it["index"] for it in items] == g("index").tolist()
    assert [it["name"] for it in items] == g("name").tolist() and [it["prompt"] for it in items] == g("prompt").tolist()
    np.testing.assert_array_equal(np.stack([it["noise"].numpy() for it in items]), g("noise"))
    np.testing.assert_allclose(np.stack([it["azimuth"].numpy() for it in items]), g("azimuth"), rtol=2e-6, atol=2e-6)
    np.testing.assert_allclose(np.stack([it["c2w"].numpy() for it in items]), g("c2w"), rtol=2e-6, atol=2e-6)
    if extra:
        np.testing.assert_array_equal(np.stack([it["ratio"].numpy() for it in items]), g("ratio"))
        assert [it["prompt_target"] for it in items] == g("prompt_target").tolist()
        assert items[0]["name"] == "a red car_to_a blue house."
    else:
        assert "ratio" not in items[0] and "prompt_target" not in items[0]
    if tag == "target_cam":
        assert len({float(it["azimuth"]) for it in items}) == 1


# ---- image grid -------------------------------------------------------------------------------------------------------------------------
def _step_panels(g, b, with_normal):
    """what validation_step / test_step hand to save_image_grid: the depth panel asks for its own range (data_range None)"""
    t = lambda k: torch.from_numpy(g[k])
    return ([{"type": "rgb", "img": t("rgb")[b], "kwargs": {"data_format": "HWC"}}]
            + ([{"type": "rgb", "img": t("normal")[b], "kwargs": {"data_format": "HWC", "data_range": (0, 1)}}] if with_normal else [])
            + [{"type": "grayscale", "img": t("opacity")[b, :, :, 0], "kwargs": {"cmap": None, "data_range": (0, 1)}},
               {"type": "grayscale", "img": t("depth")[b, :, :, 0], "kwargs": {"cmap": None, "data_range": None}}])


def test_cpu_grid_matches_reference_bytes(grids):
    from scaledreamer_amd.saving import SaverMixin

    s = SaverMixin()
    for b in range(2):
        for key, with_normal in (("grid4", True), ("grid3", False)):
            got = s.get_image_grid_(_step_panels(grids, b, with_normal))
            assert got.dtype == torch.uint8
            np.testing.assert_array_equal(got.numpy(), grids[key][b], err_msg=f"{key} image {b}")
    rows = s.get_image_grid_([_step_panels(grids, 0, False)[:2], _step_panels(grids, 1, False)[:2]])
    np.testing.assert_array_equal(rows.numpy(), grids["rows2"])
    assert not grids["grid4"][1][:, 21:].any(), "the constant depth image is an all-zero panel"
    # CHW input is the same picture
    chw = [{"type": "rgb", "img": torch.from_numpy(grids["rgb"])[0].permute(2, 0, 1), "kwargs": {"data_format": "CHW"}}]
    np.testing.assert_array_equal(s.get_image_grid_(chw).numpy(), grids["grid4"][0][:, :7])


def test_cpu_grid_special_values():
    from scaledreamer_amd.saving import grid_cpu

    inf = float("inf")
    gray = torch.tensor([[[inf, -inf, float("nan"), 0.25]]])
    out = grid_cpu([("grayscale", gray, 0.0, 1.0, False), ("rgb", torch.full((1, 1, 4, 3), float("nan")), 0.0, 1.0, False)])
    assert out.shape == (1, 1, 8, 3)
    assert out[0, 0, :4, 0].tolist() == [255, 0, 0, 63] and not out[0, 0, 4:].any()       # 0.25 * 255 = 63.75: truncated
    assert not grid_cpu([("grayscale", torch.full((1, 2, 2), 3.0), 0.0, 1.0, True)]).any()


def test_png_round_trip_and_paths(grids, tmp_path):
    from PIL import Image

    from scaledreamer_amd.saving import SaverMixin

    s = SaverMixin()
    with pytest.raises(ValueError, match="Save dir"):
        s.get_save_dir()
    s.set_save_dir(str(tmp_path))
    path = s.save_image_grid("it0-test/3.png", _step_panels(grids, 0, True), name="test_step", step=0, texts=["ignored"])
    assert path == os.path.join(str(tmp_path), "it0-test", "3.png") == s.get_save_path("it0-test/3.png")
    with Image.open(path) as im:
        assert im.mode == "RGB"
        np.testing.assert_array_equal(np.asarray(im), grids["grid4"][0])


def _frames(tmp_path):
    from PIL import Image

    d = tmp_path / "it0-test"
    d.mkdir()
    colours = {2: (255, 0, 0), 9: (0, 255, 0), 10: (0, 0, 255)}
    for i in (10, 9, 2):
        Image.fromarray(np.full((4, 6, 3), colours[i], np.uint8)).save(str(d / f"{i}.png"))
    (d / "notes.txt").write_text("not a frame")
    return colours


def test_sequence_orders_frames_by_captured_integer(tmp_path):
    from PIL import Image

    from scaledreamer_amd.saving import SaverMixin

    colours = _frames(tmp_path)
    s = SaverMixin()
    s.set_save_dir(str(tmp_path))
    path = s.save_img_sequence("it0-test", "it0-test", r"(\d+)\.png", save_format="gif", fps=30)
    assert path == str(tmp_path / "it0-test.gif")
    with Image.open(path) as im:
        assert im.n_frames == 3
        got = []
        for k in range(3):
            im.seek(k)
            got.append(tuple(int(c) for c in np.asarray(im.convert("RGB"))[0, 0]))
    assert got == [colours[2], colours[9], colours[10]]


def test_sequence_keeps_one_frame_per_file_even_when_frames_repeat(tmp_path):
    """the first and last view of a test orbit (azimuth 0 and 360) are the same picture: still two frames"""
    from PIL import Image

    from scaledreamer_amd.saving import SaverMixin

    d = tmp_path / "seq"
    d.mkdir()
    rng = np.random.default_rng(0)
    a, b = (rng.integers(0, 256, (9, 13, 3)).astype(np.uint8) for _ in range(2))
    for i, im in enumerate((a, a, b, b, a)):
        Image.fromarray(im).save(str(d / f"{i}.png"))
    s = SaverMixin()
    s.set_save_dir(str(tmp_path))
    path = s.save_img_sequence("seq", "seq", r"(\d+)\.png", save_format="gif", fps=10)
    with Image.open(path) as im:
        assert im.n_frames == 5 and im.size == (13, 9) and im.info.get("loop") == 0
        got = []
        for k in range(5):
            im.seek(k)
            assert im.info["duration"] == 100
            got.append(np.asarray(im.convert("RGB")).copy())
    for k in (1, 4):
        np.testing.assert_array_equal(got[k], got[0])
    np.testing.assert_array_equal(got[3], got[2])
    assert not np.array_equal(got[2], got[0])
    # 117 pixels fit a 256-colour palette: the frames are the files
    np.testing.assert_array_equal(got[0], a)
    np.testing.assert_array_equal(got[2], b)


def test_mp4_without_imageio_returns_the_gif(tmp_path, monkeypatch):
    import sys

    from PIL import Image

    from scaledreamer_amd.saving import SaverMixin

    _frames(tmp_path)
    monkeypatch.setitem(sys.modules, "imageio", None)          # `import imageio` raises ImportError
    s = SaverMixin()
    s.set_save_dir(str(tmp_path))
    path = s.save_img_sequence("it0-test", "it0-test", r"(\d+)\.png", save_format="mp4", fps=30)
    assert path == str(tmp_path / "it0-test.gif") and not (tmp_path / "it0-test.mp4").exists()
    with Image.open(path) as im:
        assert im.n_frames == 3


def test_unported_panels_are_refused_each_with_its_own_message():
    from scaledreamer_amd.saving import SaverMixin

    s = SaverMixin()
    img = torch.zeros(4, 4)
    with pytest.raises(NotImplementedError, match="colour map 'jet'"):
        s.get_image_grid_([{"type": "grayscale", "img": img, "kwargs": {}}])            # the reference's default cmap
    with pytest.raises(NotImplementedError, match="colour map 'magma'"):
        s.get_image_grid_([{"type": "grayscale", "img": img, "kwargs": {"cmap": "magma"}}])
    with pytest.raises(NotImplementedError, match="'uv' panels"):
        s.get_image_grid_([{"type": "uv", "img": torch.zeros(4, 4, 2), "kwargs": {}}])
    with pytest.raises(ValueError, match="unequal size"):
        s.get_image_grid_([{"type": "grayscale", "img": img, "kwargs": {"cmap": None}},
                           {"type": "grayscale", "img": torch.zeros(4, 5), "kwargs": {"cmap": None}}])
    with pytest.raises(ValueError, match="align"):
        s.get_image_grid_([{"type": "grayscale", "img": img, "kwargs": {"cmap": None}}], align="centre")


def test_systems_carry_the_eval_hooks():
    from scaledreamer_amd.multiprompt import MultipromptRadienceFieldGeneratorSystem
    from scaledreamer_amd.saving import SaverMixin
    from scaledreamer_amd.system import StableDreamer

    for cls in (StableDreamer, MultipromptRadienceFieldGeneratorSystem):
        assert issubclass(cls, SaverMixin)
        for name in ("validation_step", "on_validation_epoch_end", "test_step", "on_test_epoch_end", "validate", "test"):
            assert callable(getattr(cls, name)), name
    assert MultipromptRadienceFieldGeneratorSystem.test_step is not StableDreamer.test_step
    assert MultipromptRadienceFieldGeneratorSystem._eval_name({"prompt": ["an owl, carved from wood."]}) == "an_owl_carved_from_wood"
    assert MultipromptRadienceFieldGeneratorSystem._eval_name({"prompt": ["x"], "name": ["a red car_to_a blue house."]}) == "a_red_car_to_a_blue_house"
