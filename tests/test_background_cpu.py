"""`textured-background` and `solid-color-background` without a GPU: the float64 restatement of tests/background_util.py and the plugins'
CPU route against the goldens the reference's own classes produced (tests/golden/make_goldens_background.py), the registry names, the
config defaults, the state-dict layout and the RNG draw order of random_aug."""
import dataclasses
import os
import random

import numpy as np
import pytest
import torch

import background_util as U

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TEXTURED = ("default", "odd")
ACTS = ("sigmoid", "none")


@pytest.fixture(scope="module")
def tex():
    return dict(np.load(os.path.join(GOLDEN, "background_textured.npz")))


@pytest.fixture(scope="module")
def solid():
    return dict(np.load(os.path.join(GOLDEN, "background_solid.npz")))


def _find(name):
    import scaledreamer_amd.plugins  # noqa: F401
    from scaledreamer_amd.registry import find

    return find(name)


def test_registry_names_resolve():
    from scaledreamer_amd import background as B

    assert _find("solid-color-background") is B.SolidColorBackground
    assert _find("textured-background") is B.TexturedBackground
    assert _find("neural-environment-map-background") is B.NeuralEnvironmentMapBackground


def test_library_symbols_are_listed():
    from scaledreamer_amd import _lib, ops

    for n in ("asd_bg_texture_fwd", "asd_bg_texture_bwd_workspace", "asd_bg_texture_bwd", "asd_bg_solid_fwd", "asd_bg_solid_bwd"):
        assert n in _lib.SYMBOLS and hasattr(_lib.lib(), n), n
    for n in ("bg_texture_fwd", "bg_texture_bwd", "bg_solid_fwd", "bg_solid_bwd"):
        assert callable(getattr(ops, n))


def test_config_defaults_are_the_reference_ones():
    S, T = _find("solid-color-background").Config, _find("textured-background").Config
    own = lambda c: {f.name: f.default for f in dataclasses.fields(c) if f.name != "weights"}
    assert own(S) == {"n_output_dims": 3, "color": (1.0, 1.0, 1.0), "learned": False, "random_aug": False, "random_aug_prob": 0.5}
    assert own(T) == {"n_output_dims": 3, "height": 64, "width": 64, "color_activation": "sigmoid"}


@pytest.mark.parametrize("name", TEXTURED)
@pytest.mark.parametrize("act", ACTS)
def test_restatement_equals_the_reference(tex, name, act):
    """float64 restatement against the reference's fp32 grid_sample: colours within the forward tolerance of the GPU tests, gradients
    within the 8 backward units the GPU tests allow an fp32 pass (the largest ratio is printed)"""
    t, dirs, d_color = (torch.from_numpy(tex[f"{name}_{k}"]) for k in ("texture", "dirs", "d_color"))
    texture = t[0]
    color = U.texture_color(texture, dirs, act)
    err = float((color - torch.from_numpy(tex[f"{name}_color_{act}"]).double()).abs().max())
    assert err <= U.forward_tolerance(texture, act), err
    grad = U.texture_grad(texture, dirs, d_color, act)
    unit, n_t = U.backward_unit(texture, dirs, d_color, act)
    want = torch.from_numpy(tex[f"{name}_grad_{act}"])[0].double()
    diff = (grad - want).abs()
    print(f"{name} {act}: forward error {err:.3e}, largest backward ratio {float((diff / unit.clamp_min(1e-300)).max()):.3f} units")
    assert float((diff - 8.0 * unit).max()) <= 0.0
    assert not grad[:, n_t == 0].any() and not want[:, n_t == 0].any()
    assert (n_t > 0).any() and float(want.abs().max()) > 0


def test_special_directions_land_where_the_mapping_says():
    """both poles give v = 0.5, the sign of a zero y picks the seam row, (0, 0, 0) is the +z pole; u runs along the width"""
    H, W = 5, 7
    ix, iy = U.sample_point(U.special_dirs(), H, W)
    want_ix = [0.0, W - 1.0, W / 2 - 0.5, W / 2 - 0.5, W / 2 - 0.5, W / 2 - 0.5, W / 2 - 0.5, W / 2 - 0.5, W / 2 - 0.5, W / 2 - 0.5, 0.0]
    want_iy = [H / 2 - 0.5, H / 2 - 0.5, H / 2 - 0.5, H - 1.0, 0.75 * H - 0.5, 0.25 * H - 0.5, H - 1.0, 0.0, H - 1.0, 0.0, H / 2 - 0.5]
    torch.testing.assert_close(ix, torch.tensor(want_ix, dtype=torch.float64), rtol=0, atol=1e-12)
    torch.testing.assert_close(iy, torch.tensor(want_iy, dtype=torch.float64), rtol=0, atol=1e-12)


@pytest.mark.parametrize("name", TEXTURED)
@pytest.mark.parametrize("act", ACTS)
def test_textured_plugin_on_cpu_equals_the_reference(tex, name, act):
    t, dirs, d_color = (torch.from_numpy(tex[f"{name}_{k}"]) for k in ("texture", "dirs", "d_color"))
    C, H, W = t.shape[1:]
    bg = _find("textured-background")({"n_output_dims": C, "height": H, "width": W, "color_activation": act})
    assert isinstance(bg.texture, torch.nn.Parameter) and bg.texture.shape == (1, C, H, W)
    bg.load_state_dict({"texture": t})
    color = bg(dirs)
    assert color.shape == (dirs.shape[0], C)
    torch.testing.assert_close(color.detach(), torch.from_numpy(tex[f"{name}_color_{act}"]), rtol=0, atol=1e-6)
    (color * d_color).sum().backward()
    torch.testing.assert_close(bg.texture.grad, torch.from_numpy(tex[f"{name}_grad_{act}"]), rtol=1e-5, atol=1e-6)
    with torch.no_grad():
        img = bg(dirs[:12].view(1, 3, 4, 3))
    assert img.shape == (1, 3, 4, C)
    torch.testing.assert_close(img.view(12, C), color.detach()[:12], rtol=0, atol=1e-6)        # (torch's vector and tail loops differ in the last bit)


def test_textured_state_dict_layout(tex):
    bg = _find("textured-background")({})
    sd = bg.state_dict()
    assert sorted(sd) == list(tex["sd_keys"]) == ["texture"]
    for k in sd:
        assert tuple(sd[k].shape) == tuple(tex["sd_shape/" + k])
    a, b = _find("textured-background")({}), _find("textured-background")({})
    assert not torch.equal(a.texture, b.texture) and abs(float(a.texture.detach().std()) - 1.0) < 0.05     # torch.randn


def _solid(cfg, solid):
    bg = _find("solid-color-background")({"color": tuple(float(v) for v in solid["colour"]), **cfg})
    bg.train()
    return bg


def test_solid_plugin_on_cpu_equals_the_reference(solid):
    dirs, d_color = torch.from_numpy(solid["dirs"]), torch.from_numpy(solid["d_color"])
    fixed = _solid({"learned": False}, solid)
    assert not isinstance(fixed.env_color, torch.nn.Parameter) and "env_color" in dict(fixed.named_buffers())
    out = fixed(dirs)
    assert torch.equal(out, torch.from_numpy(solid["fixed_color"])) and not out.requires_grad
    learned = _solid({"learned": True}, solid)
    assert isinstance(learned.env_color, torch.nn.Parameter)
    out = learned(dirs)
    assert torch.equal(out.detach(), torch.from_numpy(solid["learned_color"]))
    (out * d_color).sum().backward()
    torch.testing.assert_close(learned.env_color.grad, torch.from_numpy(solid["learned_grad"]), rtol=1e-6, atol=1e-6)
    torch.testing.assert_close(learned.env_color.grad.double(), U.solid_grad(d_color.view(-1, 3), 1)[0], rtol=1e-6, atol=1e-6)
    assert torch.equal(U.solid_color(torch.from_numpy(solid["colour"])[None], 40).view(2, 4, 5, 3), torch.from_numpy(solid["fixed_color"]))


@pytest.mark.parametrize("tag", ("aug_fire", "aug_pass"))
def test_solid_random_aug_draws_in_the_reference_order(solid, tag):
    """both host RNGs pinned as the generator pinned them: random.random() first, torch.rand(B, 1, 1, C) only when it fires"""
    dirs, d_color = torch.from_numpy(solid["dirs"]), torch.from_numpy(solid["d_color"])
    bg = _solid({"learned": True, "random_aug": True, "random_aug_prob": 0.5}, solid)
    seeds = solid[f"{tag}_seeds"]
    random.seed(int(seeds[0]))
    torch.manual_seed(int(seeds[1]))
    out = bg(dirs)
    assert torch.equal(torch.rand(4), torch.from_numpy(solid[f"{tag}_next_torch_draw"]))
    assert torch.equal(out.detach(), torch.from_numpy(solid[f"{tag}_color"]))
    fired = bool(solid[f"{tag}_fired"])
    assert fired == (tag == "aug_fire")
    (out * d_color).sum().backward()
    if fired:       # `color * 0 +`: the learned colour stays in the graph and receives a zero gradient
        rc = torch.from_numpy(solid[f"{tag}_rand_color"])
        assert torch.equal(out.detach(), rc.expand(2, 4, 5, 3)) and bg.env_color.grad is not None and not bg.env_color.grad.any()
    else:
        torch.testing.assert_close(bg.env_color.grad, torch.from_numpy(solid["learned_grad"]), rtol=1e-6, atol=1e-6)


def test_solid_hooks_and_eval(solid):
    dirs = torch.from_numpy(solid["dirs"])
    bg = _solid({"learned": True, "random_aug": True, "random_aug_prob": 0.5}, solid)
    calls = []
    bg.rand_fn = lambda: calls.append("rand") or 0.1
    bg.rand_color_fn = lambda b, c: calls.append(("color", b, c)) or torch.full((b, 1, 1, c), 0.25)
    out = bg(dirs)
    assert calls == ["rand", ("color", 2, 3)] and torch.equal(out.detach(), torch.full((2, 4, 5, 3), 0.25))
    bg.rand_fn = lambda: calls.append("rand") or 0.9
    out = bg(dirs)
    assert calls[2:] == ["rand"] and torch.equal(out.detach(), torch.from_numpy(solid["learned_color"]))
    bg.eval()       # training = False never augments, and draws nothing
    bg.rand_fn = lambda: pytest.fail("eval drew from the RNG")
    assert torch.equal(bg(dirs).detach(), torch.from_numpy(solid["aug_eval_color"]))
    assert torch.equal(torch.from_numpy(solid["aug_eval_color"]), torch.from_numpy(solid["learned_color"]))


def test_solid_state_dict_layout_and_load(solid):
    for tag, learned in (("learned", True), ("fixed", False)):
        bg = _find("solid-color-background")({"learned": learned})
        sd = bg.state_dict()
        assert sorted(sd) == list(solid[f"sd_{tag}_keys"]) == ["env_color"]
        rec = {k: torch.from_numpy(solid[f"sd_{tag}/" + k]) for k in sd}
        assert all(sd[k].shape == rec[k].shape and sd[k].dtype == rec[k].dtype for k in sd)
        bg.load_state_dict(rec)
        assert torch.equal(bg.env_color.detach(), torch.from_numpy(solid["colour"]))
    assert bool(solid["sd_learned_is_parameter"])
