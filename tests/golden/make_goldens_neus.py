"""Golden vectors of the single-prompt SDF route: the REFERENCE's own ImplicitSDF + NeuSVolumeRenderer + NoMaterial +
NeuralEnvironmentMapBackground, imported in place under ref_harness.py and run on the CPU oracle (see make_goldens.py).

  python tests/golden/make_goldens_neus.py       # writes tests/golden/neus_*.npz and neus_state_dict_keys.json

The harness's occupancy estimator ignores alpha_fn; the subclass below adds nerfacc's alpha visibility rule (render_visibility_from_alpha:
keep = T >= early_stop_eps and alpha >= alpha_thre, T the exclusive product of 1 - alpha along the ray).  The generator ASSERTS that no
candidate sits within 1e-4 (relative) of either threshold, so keep decisions can be compared exactly; pick another seed if it fires.
The .npz files are data only (inputs, seeds / generation rules, expected outputs).
"""
from __future__ import annotations

import json
import os
import random
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_harness as H  # noqa: E402

H.install_amortized()        # (install() + nerfacc.render_weight_from_alpha)

from make_goldens import BG_ENC, camera_rays, grid_params  # noqa: E402
from threestudio.models.background.neural_environment_map_background import NeuralEnvironmentMapBackground  # noqa: E402
from threestudio.models.geometry.implicit_sdf import ImplicitSDF  # noqa: E402
from threestudio.models.materials.no_material import NoMaterial  # noqa: E402
from threestudio.models.renderers.neus_volume_renderer import NeuSVolumeRenderer  # noqa: E402

MARGIN = 1e-4
LOG = {}


class AlphaOccGridEstimator(H.OracleOccGridEstimator):
    def sampling(self, rays_o, rays_d, sigma_fn=None, alpha_fn=None, near_plane=0.0, far_plane=1e10, t_min=None, t_max=None,
                 render_step_size=1e-3, early_stop_eps=1e-4, alpha_thre=0.0, stratified=False, cone_angle=0.0):
        if alpha_fn is None:
            return super().sampling(rays_o, rays_d, sigma_fn, None, near_plane, far_plane, t_min, t_max, render_step_size, early_stop_eps,
                                    alpha_thre, stratified, cone_angle)
        # the candidates: the parent without a pruning function
        ri, t0, t1 = super().sampling(rays_o, rays_d, None, None, near_plane, far_plane, t_min, t_max, render_step_size, early_stop_eps,
                                      alpha_thre, stratified, cone_angle)
        alpha_thre = min(alpha_thre, float(self.occs.mean().item()))
        alphas = alpha_fn(t0, t1, ri).detach() if t0.shape[0] else torch.zeros(0)
        a64 = alphas.double().numpy()
        idx = ri.numpy()
        T = np.ones_like(a64)
        run, last = 1.0, -1
        for i in range(a64.shape[0]):
            if idx[i] != last:
                run, last = 1.0, idx[i]
            T[i] = run
            run *= 1.0 - a64[i]
        assert not (np.abs(a64 - alpha_thre) <= MARGIN * alpha_thre).any(), "a candidate alpha sits on alpha_thre: choose another seed"
        assert not (np.abs(T - early_stop_eps) <= MARGIN * early_stop_eps).any(), "a transmittance sits on early_stop_eps: choose another seed"
        # an alpha above 1 (VolSDF: step * inv_std > 1) makes the running product change sign: outside what a density-based pruning pass can
        # express, so the fixtures stay below it
        assert a64.size == 0 or a64.max() < 1.0 or not self.volsdf, "a VolSDF candidate alpha reaches 1: lower learned_variance_init"
        keep = torch.from_numpy((T >= early_stop_eps) & (a64 >= alpha_thre))
        LOG.update(cand_ray_indices=ri.numpy().copy(), cand_t_starts=t0.numpy().copy(), cand_t_ends=t1.numpy().copy(),
                   cand_alpha=alphas.numpy().copy(), cand_keep=keep.numpy().copy(), alpha_thre=np.float64(alpha_thre))
        return ri[keep], t0[keep], t1[keep]


sys.modules["nerfacc"].OccGridEstimator = AlphaOccGridEstimator


def build(spp, seed, grid_amp, ren_cfg):
    torch.manual_seed(seed)
    geo = ImplicitSDF({"radius": 1.0, "normal_type": "finite_difference", "sdf_bias": "sphere", "sdf_bias_params": 0.5})
    mat = NoMaterial({"n_output_dims": 3, "color_activation": "sigmoid"})
    bg = NeuralEnvironmentMapBackground({"color_activation": "sigmoid", "random_aug": True, "random_aug_prob": 0.5, "dir_encoding_config": BG_ENC})
    ren = NeuSVolumeRenderer({"radius": 1.0, "num_samples_per_ray": spp, **ren_cfg}, geometry=geo, material=mat, background=bg)
    with torch.no_grad():
        geo.encoding.encoding.encoding.params.copy_(torch.from_numpy(grid_params(seed, 12_599_920, grid_amp)))
        bg.encoding.encoding.encoding.params.copy_(torch.from_numpy(grid_params(seed + 1, 1_581_184, 0.5)))
        for p in list(geo.sdf_network.parameters()) + list(geo.feature_network.parameters()):
            p.mul_(2.0)
    geo.update_step(0, 0)
    return geo, mat, bg, ren


def occupancy_from_field(geo, ren):
    """the warm-up occupancy update at step 0 without jitter: occ = occ_eval_fn(cell centre) (neus_volume_renderer.py:364-377)"""
    res = 32
    ix, iy, iz = torch.meshgrid(*[torch.arange(res)] * 3, indexing="ij")
    x = (torch.stack([ix, iy, iz], -1).reshape(-1, 3).float() + 0.5) / res * 2 - 1
    grabbed = {}

    class Grab(torch.nn.Module):
        def update_every_n_steps(self, step, occ_eval_fn):
            grabbed["fn"] = occ_eval_fn

    est, ren.estimator = ren.estimator, Grab()
    ren.train()
    ren.update_step(0, 0)
    ren.estimator = est
    with torch.no_grad():
        occ = grabbed["fn"](x)[..., 0]
    thre = min(float(occ.mean()), 0.01)
    return occ, (occ > thre).view(1, res, res, res)


def make(name, h, w, spp, seed, grid_amp, cam, ren_cfg, step, want):
    LOG.clear()
    geo, mat, bg, ren = build(spp, seed, grid_amp, ren_cfg)
    if ren.cfg.grid_prune:
        occ, binaries = occupancy_from_field(geo, ren)
        ren.estimator.occs.copy_(occ)
        ren.estimator.binaries.copy_(binaries)
    rays_o, rays_d, cam_pos = camera_rays(h, w, *cam)
    rng = np.random.default_rng(seed + 7)
    jitter = rng.uniform(0, 1, h * w).astype(np.float32)
    ren.estimator.jitter = jitter
    ren.estimator.volsdf = bool(ren.cfg.use_volsdf)
    random.random = lambda: 0.9
    ren.train(); geo.train(); bg.train(); mat.train()
    class NoUpdate(torch.nn.Module):
        def update_every_n_steps(self, step, occ_eval_fn):
            pass

    est, ren.estimator = ren.estimator, NoUpdate()
    ren.update_step(0, step)            # cos_anneal_ratio
    ren.estimator = est
    alpha_log = {}
    ref_get_alpha = ren.get_alpha

    def get_alpha(sdf, normal, dirs, dists):
        a = ref_get_alpha(sdf, normal, dirs, dists)
        alpha_log["alpha"] = a.detach().numpy().copy()
        return a
    ren.get_alpha = get_alpha
    out = ren(rays_o=rays_o, rays_d=rays_d, light_positions=cam_pos)
    g_rgb = torch.from_numpy(rng.normal(size=(1, h, w, 3)).astype(np.float32))
    g_depth = torch.from_numpy(rng.normal(size=(1, h, w, 1)).astype(np.float32))
    g_opacity = torch.from_numpy(rng.normal(size=(1, h, w, 1)).astype(np.float32))
    loss_eikonal = ((torch.linalg.norm(out["sdf_grad"], ord=2, dim=-1) - 1.0) ** 2).mean()
    loss = (out["comp_rgb"] * g_rgb).sum() + 0.1 * (out["depth"] * g_depth).sum() + 0.5 * (out["opacity"] * g_opacity).sum() + 10.0 * loss_eikonal
    loss.backward()

    kept = np.bincount(out["ray_indices"].numpy(), minlength=h * w)
    if want == "empty_ray":
        assert (kept == 0).any(), "case (a) needs a ray that keeps nothing"
    if want == "long_ray":
        assert kept.max() >= 65, "case (b) needs a ray that keeps 65 or more samples"
    tc = (out["t_dirs"] * out["normal"]).sum(-1).detach().numpy()
    cfg = {k: getattr(ren.cfg, k) for k in ("num_samples_per_ray", "randomized", "eval_chunk_size", "learned_variance_init", "cos_anneal_end_steps",
                                            "use_volsdf", "near_plane", "far_plane", "estimator", "grid_prune", "prune_alpha_threshold",
                                            "num_samples_per_ray_importance")}
    save = dict(
        h=h, w=w, spp=spp, seed=seed, grid_amp=grid_amp, cam=np.array(cam, np.float32), step=step, ren_cfg=json.dumps(cfg),
        cos_anneal_ratio=np.float64(ren.cos_anneal_ratio), render_step_size=np.float64(ren.render_step_size),
        rays_o=rays_o.numpy(), rays_d=rays_d.numpy(), light_positions=cam_pos.numpy(), jitter=jitter,
        occs=ren.estimator.occs.numpy(), binaries=ren.estimator.binaries.numpy(), g_rgb=g_rgb.numpy(), g_depth=g_depth.numpy(),
        g_opacity=g_opacity.numpy(),
        w1s=geo.sdf_network.layers[0].weight.detach().numpy(), w2s=geo.sdf_network.layers[2].weight.detach().numpy(),
        w1f=geo.feature_network.layers[0].weight.detach().numpy(), w2f=geo.feature_network.layers[2].weight.detach().numpy(),
        bw0=bg.network.layers[0].weight.detach().numpy(), bw1=bg.network.layers[2].weight.detach().numpy(),
        bw2=bg.network.layers[4].weight.detach().numpy(), inv_std_param=ren.variance._inv_std.detach().numpy(),
        loss=np.float64(loss.item()), loss_eikonal=np.float64(loss_eikonal.item()), alpha=alpha_log["alpha"],
    )
    if LOG:
        with torch.no_grad():
            t0, t1, ri = (torch.from_numpy(LOG[k]) for k in ("cand_t_starts", "cand_t_ends", "cand_ray_indices"))
            pos = rays_o.reshape(-1, 3)[ri] + rays_d.reshape(-1, 3)[ri] * ((t0 + t1) / 2.0)[..., None]
            LOG["cand_sdf"] = geo.forward_sdf(pos)[..., 0].numpy()
        save.update(LOG)
    for k, v in out.items():
        save["out_" + k] = v.detach().numpy()
    for k, p in (("w1s", geo.sdf_network.layers[0].weight), ("w2s", geo.sdf_network.layers[2].weight), ("w1f", geo.feature_network.layers[0].weight),
                 ("w2f", geo.feature_network.layers[2].weight), ("bw0", bg.network.layers[0].weight), ("bw1", bg.network.layers[2].weight),
                 ("bw2", bg.network.layers[4].weight), ("inv_std_param", ren.variance._inv_std)):
        save["g_" + k] = p.grad.numpy()
    gg = geo.encoding.encoding.encoding.params.grad.numpy()
    top = np.argsort(-np.abs(gg))[:20000].astype(np.int64)
    save.update(g_grid_idx=top, g_grid_val=gg[top], g_grid_l2=np.float64(np.linalg.norm(gg.astype(np.float64))))
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **save)
    print(f"{name}: N={out['weights'].shape[0]} samples (max {kept.max()} / ray, {(kept == 0).sum()} empty rays), loss={loss.item():.6f}, "
          f"opacity mean={out['opacity'].mean().item():.4f}, true_cos in [{tc.min():.3f}, {tc.max():.3f}], "
          f"inv_std grad={ren.variance._inv_std.grad.item():.4e} -> {path} ({os.path.getsize(path) / 1e6:.2f} MB)")
    return geo, ren


if __name__ == "__main__":
    which = sys.argv[1:] or ["a", "b", "c"]
    geo = ren = None
    if "a" in which:    # pruning with the alpha threshold, anneal ratio 1
        geo, ren = make("neus_a_16x16x64", 16, 16, 64, seed=31, grid_amp=0.05, cam=(20.0, 40.0, 1.6, 50.0), ren_cfg={}, step=0, want="empty_ray")
    if "b" in which:    # no grid pruning, anneal ratio 0.5: rays keep more than one wave trip of samples, both relu branches live
        geo, ren = make("neus_b_12x12x96", 12, 12, 96, seed=37, grid_amp=0.05, cam=(-25.0, 115.0, 2.6, 50.0),
                        ren_cfg={"grid_prune": False, "cos_anneal_end_steps": 100}, step=50, want="long_ray")
    if "c" in which:    # VolSDF opacity, pruned; inv_std = exp(2.5): step * inv_std = 0.66
        geo, ren = make("neus_c_8x8x64_volsdf", 8, 8, 64, seed=41, grid_amp=0.05, cam=(10.0, -60.0, 1.5, 45.0), ren_cfg={"use_volsdf": True, "learned_variance_init": 0.25},
                        step=0,
                        want=None)
    if geo is not None:
        keys = {"geometry": sorted(geo.state_dict().keys()), "renderer": sorted(k for k in ren.state_dict().keys() if not k.startswith("estimator.")),      # (the estimator is nerfacc's, stubbed here)
                "geometry_defaults": {k: v for k, v in vars(ImplicitSDF.Config()).items() if isinstance(v, (int, float, str, bool, type(None), dict))},
                "renderer_defaults": {k: v for k, v in vars(NeuSVolumeRenderer.Config()).items() if isinstance(v, (int, float, str, bool, type(None)))}}
        with open(os.path.join(HERE, "neus_state_dict_keys.json"), "w") as f:
            json.dump(keys, f, indent=1, sort_keys=True)
