"""GPU parity of `neus-volume-renderer` + `implicit-sdf` against the goldens produced by the reference's own classes
(tests/golden/make_goldens_neus.py): every key of the output dictionary, the kept sample set exactly, and the parameter gradients of the
generator's loss — on the fused route (ASD_NEUS=1) and the composed one (ASD_NEUS=0).  Bounds: those of tests/test_gpu_renderer_golden.py
(the same field kernels produce the values)."""
import json

import numpy as np
import pytest
import torch

from golden_util import load_renderer_golden

pytestmark = pytest.mark.gpu

CASES = ["neus_a_16x16x64", "neus_b_12x12x96", "neus_c_8x8x64_volsdf"]
BG_ENC = {"otype": "HashGrid", "n_features_per_level": 2, "log2_hashmap_size": 19, "n_levels": 4, "base_resolution": 4, "per_level_scale": 4.0}
_CACHE = {}


def golden(name):
    if name not in _CACHE:          # (loaded once: the 12.6 M-entry table comes from its seed rule)
        _CACHE[name] = load_renderer_golden(name)
    return _CACHE[name]


def build_system(g):
    import scaledreamer_amd.plugins  # noqa: F401
    from scaledreamer_amd.registry import find

    cfg = json.loads(str(g["ren_cfg"]))
    geo = find("implicit-sdf")({"radius": 1.0, "normal_type": "finite_difference", "sdf_bias": "sphere", "sdf_bias_params": 0.5})
    mat = find("no-material")({"n_output_dims": 3, "color_activation": "sigmoid"})
    bg = find("neural-environment-map-background")({"color_activation": "sigmoid", "random_aug": True, "random_aug_prob": 0.5,
                                                    "dir_encoding_config": BG_ENC})
    ren = find("neus-volume-renderer")({"radius": 1.0, **cfg}, geometry=geo, material=mat, background=bg)
    sd_geo = {"encoding.encoding.encoding.params": g["grid"], "sdf_network.layers.0.weight": g["w1s"], "sdf_network.layers.2.weight": g["w2s"],
              "feature_network.layers.0.weight": g["w1f"], "feature_network.layers.2.weight": g["w2f"]}
    sd_bg = {"encoding.encoding.encoding.params": g["bgrid"], "network.layers.0.weight": g["bw0"], "network.layers.2.weight": g["bw1"],
             "network.layers.4.weight": g["bw2"]}
    geo.load_state_dict({k: torch.from_numpy(v) for k, v in sd_geo.items()}, strict=False)
    bg.load_state_dict({k: torch.from_numpy(v) for k, v in sd_bg.items()}, strict=False)
    for m in (geo, mat, bg, ren):
        m.cuda().train()
    ren.load_state_dict({"estimator.occs": torch.from_numpy(g["occs"]), "estimator.binaries": torch.from_numpy(g["binaries"]),
                         "variance._inv_std": torch.from_numpy(g["inv_std_param"])}, strict=False)
    geo.update_step(0, 0)
    ren.cfg.grid_prune, saved = False, ren.cfg.grid_prune          # cos_anneal_ratio of the fixture's step without an occupancy update
    ren.update_step(0, int(g["step"]))
    ren.cfg.grid_prune = saved
    assert ren.cos_anneal_ratio == float(g["cos_anneal_ratio"])
    jit = torch.from_numpy(g["jitter"]).cuda()
    ren.jitter_fn = lambda n, device: jit
    bg.rand_fn = lambda: 0.9
    return geo, mat, bg, ren


def reference_loss(out, g):
    t = lambda k: torch.from_numpy(g[k]).cuda()
    loss_eikonal = ((torch.linalg.norm(out["sdf_grad"], ord=2, dim=-1) - 1.0) ** 2).mean()
    return ((out["comp_rgb"] * t("g_rgb")).sum() + 0.1 * (out["depth"] * t("g_depth")).sum() + 0.5 * (out["opacity"] * t("g_opacity")).sum()
            + 10.0 * loss_eikonal), loss_eikonal


@pytest.mark.parametrize("route", ["1", "0"], ids=["fused", "composed"])
@pytest.mark.parametrize("name", CASES)
def test_neus_renderer_matches_reference_outputs_and_grads(name, route, monkeypatch):
    monkeypatch.setenv("ASD_NEUS", route)
    g = golden(name)
    geo, mat, bg, ren = build_system(g)
    dev = lambda k: torch.from_numpy(g[k]).cuda()
    out = ren(rays_o=dev("rays_o"), rays_d=dev("rays_d"), light_positions=dev("light_positions"), elevation=None, azimuth=None)
    expected = {k[4:] for k in g if k.startswith("out_")}
    assert set(out.keys()) == expected
    n = g["out_weights"].shape[0]
    assert out["weights"].shape == (n, 1) and out["ray_indices"].dtype == torch.int64
    cpu = {k: v.detach().cpu().numpy() for k, v in out.items()}
    np.testing.assert_array_equal(cpu["ray_indices"], g["out_ray_indices"])
    for k in ["t_points", "t_intervals", "points", "t_dirs"]:
        np.testing.assert_array_equal(cpu[k], g["out_" + k], err_msg=k)
    for k in ["sdf", "features", "weights", "comp_rgb", "comp_rgb_fg", "comp_rgb_bg", "opacity", "depth", "inv_std"]:
        assert cpu[k].shape == g["out_" + k].shape, k
        np.testing.assert_allclose(cpu[k], g["out_" + k], rtol=2e-5, atol=1e-5, err_msg=k)
    # normal = sdf_grad / |sdf_grad| with |sdf_grad| ~ 1 for this field: the un-normalised difference quotient carries the normal's bound
    np.testing.assert_allclose(cpu["normal"], g["out_normal"], rtol=0, atol=2e-3)
    np.testing.assert_allclose(cpu["sdf_grad"], g["out_sdf_grad"], rtol=0, atol=2e-3)
    assert out["shading_normal"] is out["normal"] or torch.equal(out["shading_normal"], out["normal"])

    loss, loss_eikonal = reference_loss(out, g)
    assert abs(loss.item() - float(g["loss"])) < 2e-4 * max(1.0, abs(float(g["loss"])))
    assert abs(loss_eikonal.item() - float(g["loss_eikonal"])) < 2e-4 * max(1.0, abs(float(g["loss_eikonal"])))
    loss.backward()
    got = {"w1s": geo.sdf_network.layers[0].weight, "w2s": geo.sdf_network.layers[2].weight, "w1f": geo.feature_network.layers[0].weight,
           "w2f": geo.feature_network.layers[2].weight, "bw0": bg.network.layers[0].weight, "bw1": bg.network.layers[2].weight,
           "bw2": bg.network.layers[4].weight, "inv_std_param": ren.variance._inv_std}
    for k, p in got.items():
        ref = g["g_" + k]
        scale = max(float(np.abs(ref).max()), 1e-6)
        np.testing.assert_allclose(p.grad.cpu().numpy() / scale, ref / scale, rtol=0, atol=3e-3, err_msg=k)
    gg = geo.encoding.encoding.encoding.params.grad.cpu().numpy()
    idx, val = g["g_grid_idx"], g["g_grid_val"]
    np.testing.assert_allclose(gg[idx] / np.abs(val).max(), val / np.abs(val).max(), rtol=0, atol=3e-3)
    assert abs(np.linalg.norm(gg.astype(np.float64)) / float(g["g_grid_l2"]) - 1) < 3e-3


@pytest.mark.parametrize("route", ["1", "0"], ids=["fused", "composed"])
def test_eval_mode_and_empty_rays(route, monkeypatch):
    monkeypatch.setenv("ASD_NEUS", route)
    g = golden(CASES[0])
    geo, mat, bg, ren = build_system(g)
    ren.eval(); geo.eval(); bg.eval()
    dev = lambda k: torch.from_numpy(g[k]).cuda()
    with torch.no_grad():
        out = ren(rays_o=dev("rays_o"), rays_d=dev("rays_d"), light_positions=dev("light_positions"))
    per_sample = {"weights", "t_points", "t_intervals", "t_dirs", "ray_indices", "points", "sdf", "sdf_grad", "normal", "features"}
    assert "comp_normal" in out and not (per_sample & set(out.keys())) and "inv_std" in out
    assert out["comp_rgb"].shape == (1, int(g["h"]), int(g["w"]), 3) and out["comp_normal"].shape == (1, int(g["h"]), int(g["w"]), 3)
    assert torch.isfinite(out["comp_normal"]).all() and float(out["comp_normal"].min()) >= 0.0 and float(out["comp_normal"].max()) <= 1.0
    # rays that miss the box entirely: one dummy sample, background only
    o = torch.full((1, 4, 4, 3), 5.0, device="cuda")
    d = torch.nn.functional.normalize(torch.ones(1, 4, 4, 3, device="cuda"), dim=-1)
    ren.train()
    out = ren(rays_o=o, rays_d=d, light_positions=o[:, 0, 0])
    assert out["weights"].shape == (1, 1) and int(out["ray_indices"][0]) == 0
    # the dummy sample (ray 0, t = 0, zero length, far outside the surface) has the reference's alpha (0 + 1e-5) / (1 + 1e-5)
    op = out["opacity"].reshape(-1)
    assert float(op[1:].detach().abs().max()) == 0.0 and float(op[0].detach().abs()) <= 1.01e-5
    assert torch.equal(out["comp_rgb"].reshape(-1, 3)[1:], out["comp_rgb_bg"].reshape(-1, 3)[1:])
    torch.testing.assert_close(out["comp_rgb"], out["comp_rgb_bg"])
    out["comp_rgb"].sum().backward()            # the dummy sample carries a graph as any other


def test_eval_image_is_the_same_on_both_routes(monkeypatch):
    g = golden(CASES[1])
    dev = lambda k: torch.from_numpy(g[k]).cuda()
    outs = {}
    for route in ("1", "0"):
        monkeypatch.setenv("ASD_NEUS", route)
        geo, mat, bg, ren = build_system(g)
        ren.eval(); geo.eval(); bg.eval()
        with torch.no_grad():
            outs[route] = ren(rays_o=dev("rays_o"), rays_d=dev("rays_d"), light_positions=dev("light_positions"))
    assert set(outs["0"]) == set(outs["1"])
    for k in outs["0"]:
        torch.testing.assert_close(outs["1"][k], outs["0"][k], rtol=2e-5, atol=1e-5, msg=k)


def test_estimator_sampling_with_alpha_fn_keeps_the_fixture_samples():
    """nerfacc_api.OccGridEstimator.sampling(alpha_fn=...) — the reference's call (neus_volume_renderer.py:183-194) — keeps what the renderer's
    own pruned branch keeps"""
    from scaledreamer_amd.neus_renderer import step_alpha

    g = golden(CASES[0])
    geo, mat, bg, ren = build_system(g)
    ro, rd = torch.from_numpy(g["rays_o"]).cuda().reshape(-1, 3), torch.from_numpy(g["rays_d"]).cuda().reshape(-1, 3)

    def alpha_fn(t_starts, t_ends, ray_indices):
        pos = ro[ray_indices] + rd[ray_indices] * ((t_starts + t_ends) / 2.0)[..., None]
        sdf = geo.forward_sdf(pos)[..., 0]
        return step_alpha(sdf, ren.variance(sdf), ren.render_step_size, False)

    ri, t0, t1 = ren.estimator.sampling(ro, rd, alpha_fn=alpha_fn, render_step_size=ren.render_step_size, alpha_thre=0.01, stratified=True,
                                        jitter=torch.from_numpy(g["jitter"]).cuda())
    np.testing.assert_array_equal(ri.cpu().numpy(), g["out_ray_indices"])
    np.testing.assert_array_equal(((t0 + t1) / 2.0).cpu().numpy(), g["out_t_points"][:, 0])
