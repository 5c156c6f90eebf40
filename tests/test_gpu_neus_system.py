"""The single-prompt SDF route end to end: one training step of `scaledreamer-system` with `implicit-sdf` + `neus-volume-renderer` and the
eikonal regulariser, the shape initialisation loop on the fused sdf entry against the composed one, and mesh export of an exact sphere."""
import os
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _sdf_preset():
    from scaledreamer_amd import presets

    with presets.random_weights_allowed():       # seeded random prior (no checkpoint offline); scoped, not a process-wide switch
        cfg = presets.asd_sd_nerf()
    s = cfg["system"]
    s["geometry_type"] = "implicit-sdf"
    s["geometry"] = {"radius": 1.0, "normal_type": "finite_difference", "sdf_bias": "sphere", "sdf_bias_params": 0.5,
                     "pos_encoding_config": s["geometry"]["pos_encoding_config"]}
    s["renderer_type"] = "neus-volume-renderer"
    s["renderer"] = {"radius": 1.0, "num_samples_per_ray": 128, "cos_anneal_end_steps": 100}
    s["material"]["requires_normal"] = False
    s["background"]["random_aug"] = False        # (a random-colour step gives the background an all-zero gradient)
    s["loss"] = {"lambda_asd": 1.0, "lambda_orient": 0.0, "lambda_sparsity": 30, "lambda_opaque": 0.0, "lambda_z_variance": 0.0, "lambda_eikonal": 10.0}
    s["optimizer"]["params"] = {"geometry.encoding": {"lr": 0.01}, "geometry.sdf_network": {"lr": 0.001}, "geometry.feature_network": {"lr": 0.001},
                                "background.encoding": {"lr": 0.01}, "background.network": {"lr": 0.001}, "renderer": {"lr": 0.001}}
    return cfg


def test_one_training_step_with_the_eikonal_term():
    """as the step test of tests/test_gpu_amortized.py builds it: reduced-width HIP UNet, full VAE"""
    from scaledreamer_amd.data import RandomCameraIterableDataset
    from scaledreamer_amd.diffusion import weights as W
    from scaledreamer_amd.diffusion.engine import HipBackend
    from scaledreamer_amd.guidance import PromptUtils
    from scaledreamer_amd.registry import find
    import scaledreamer_amd.plugins  # noqa: F401

    torch.manual_seed(0)
    random.seed(0)
    dev = torch.device("cuda", 0)
    cfg = _sdf_preset()
    backend = HipBackend(dev, unet_cfg=W.UNetConfig(model_channels=128, context_dim=128), vae_cfg=W.VAEConfig(), seed=3)
    g = torch.Generator().manual_seed(1)
    pu = PromptUtils(torch.randn(4, 77, 128, generator=g).to(dev), torch.randn(1, 77, 128, generator=g).expand(4, -1, -1).contiguous().to(dev),
                     front_threshold=30.0, back_threshold=30.0)
    system = find(cfg["system_type"])(cfg["system"], guidance_backend=backend, prompt_utils=pu)
    system.train()
    data = RandomCameraIterableDataset(cfg["data"])
    batch = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in data.collate().items()}
    loss = system.train_one_step(batch)
    assert torch.isfinite(loss).item()
    assert system.geometry.fused and system.renderer.cos_anneal_ratio == 0.0
    for k in ("train/loss_asd", "train/loss_eikonal", "train/inv_std", "train/loss_sparsity"):
        assert k in system.logged and torch.isfinite(system.logged[k]).all().item(), k
    assert abs(float(system.logged["train/inv_std"].detach()) - float(np.exp(3.0))) < 0.5        # exp(10 * 0.3) before its first update
    named = [(f"{m}.{n}", p) for m in ("geometry", "background", "renderer") for n, p in getattr(system, m).named_parameters() if p.requires_grad]
    assert "renderer.variance._inv_std" in dict(named)
    for n, p in named:
        assert p.grad is not None and torch.isfinite(p.grad).all().item() and float(p.grad.abs().max()) > 0, n


INIT_STEPS = 50


def _init_losses(fused: bool, steps: int = INIT_STEPS):
    import scaledreamer_amd.plugins  # noqa: F401
    from scaledreamer_amd.registry import find

    torch.manual_seed(7)
    geo = find("implicit-sdf")({"shape_init": "sphere", "shape_init_params": 0.5}).cuda()
    assert geo.fused
    start = {k: v.detach().clone() for k, v in geo.state_dict().items()}
    if not fused:
        geo._fcfg = None           # the composed route: HIP hash-grid encoding + tensor-op MLP
    geo.SHAPE_INIT_STEPS = steps
    torch.manual_seed(11)          # the loop's points
    geo.initialize_shape()
    return torch.stack(geo.shape_init_losses).double().cpu().numpy(), geo, start


def _hashgrid_float64(meta, params, x):
    """the hash-grid encoding (tcnn's layout as include/asd_hip.h states it: per level pos = scale x + 0.5, trilinear weights, dense index
    x + y res + z res^2 or the xor hash, modulo the level's size) as float64 tensor ops; params [n_params] viewed as [entries, 2], x [n, 3] in [0, 1]"""
    table = params.view(-1, 2)
    x = x.clamp(0.0, 1.0)
    out = []
    for l in range(meta.n_levels):
        pos = x * float(meta.scale[l]) + 0.5
        cell = torch.floor(pos)
        w = pos - cell
        cell = cell.long()
        acc = 0.0
        for corner in range(8):
            b = [(corner >> d) & 1 for d in range(3)]
            wt = 1.0
            for d in range(3):
                wt = wt * (w[:, d] if b[d] else 1.0 - w[:, d])
            cx, cy, cz = (cell[:, d] + b[d] for d in range(3))
            if meta.dense[l]:
                res = int(meta.resolution[l])
                idx = (cx + cy * res + cz * res * res) & 0xFFFFFFFF
            else:
                idx = cx ^ ((cy * 2654435761) & 0xFFFFFFFF) ^ ((cz * 805459861) & 0xFFFFFFFF)
            idx = idx % int(meta.size[l]) + int(meta.offset[l])
            acc = acc + wt[:, None] * table[idx]
        out.append(acc)
    return torch.cat(out, dim=1)


def _init_losses_float64(geo, start, steps: int = INIT_STEPS):
    """the same loop — same start, same seeded points, Adam at 1e-3 over every parameter, MSE against |x| - 0.5 — with the hash-grid
    interpolation, the sdf head and Adam in float64"""
    meta = geo.encoding.encoding.encoding.meta
    grid = start["encoding.encoding.encoding.params"].double().requires_grad_(True)
    w1 = start["sdf_network.layers.0.weight"].double().requires_grad_(True)
    w2 = start["sdf_network.layers.2.weight"].double().requires_grad_(True)
    optim = torch.optim.Adam([grid, w1, w2], lr=1e-3)
    torch.manual_seed(11)
    losses = []
    for _ in range(steps):
        pts = (torch.rand((10000, 3), dtype=torch.float32).cuda() * 2.0 - 1.0)
        gt = (pts.double() ** 2).sum(dim=-1, keepdim=True).sqrt() - 0.5
        x = pts.double()
        enc = _hashgrid_float64(meta, grid, (x + 1.0) / 2.0)
        sdf = torch.relu(enc @ w1.t()) @ w2.t()
        loss = ((sdf - gt) ** 2).mean()
        optim.zero_grad()
        loss.backward()
        optim.step()
        losses.append(loss.detach())
    return torch.stack(losses).cpu().numpy()


def test_initialize_shape_on_the_fused_entry_follows_the_composed_loop():
    """Per step, on the loss: e_fused <= 4 e_composed + 2e-6 max|ref|, e_* the distance from the float64 loop written above (the rule of
    tests/test_gpu_neus_kernels.py).  What Adam's normalised update makes of rounding noise in a gradient grows e_composed as it grows
    e_fused.  The pairs are printed."""
    fused, geo, start = _init_losses(True)
    composed, _, start_c = _init_losses(False)
    assert all(torch.equal(start[k], start_c[k]) for k in start)
    ref = _init_losses_float64(geo, start)
    assert fused.shape == composed.shape == ref.shape == (INIT_STEPS,) and np.isfinite(fused).all()
    e_f, e_c = np.abs(fused - ref), np.abs(composed - ref)
    bound = 4.0 * e_c + 2e-6 * np.abs(ref)
    print("step loss_ref loss_fused loss_composed e_fused e_composed bound")
    for i in range(INIT_STEPS):
        print(f"{i:3d} {ref[i]:.9e} {fused[i]:.9e} {composed[i]:.9e} {e_f[i]:.3e} {e_c[i]:.3e} {bound[i]:.3e}")
    bad = [i for i in range(INIT_STEPS) if not e_f[i] <= bound[i]]
    assert not bad, bad
    assert fused[-1] < fused[0] and composed[-1] < composed[0] and ref[-1] < ref[0]
    with torch.no_grad():          # the loop trained the sdf head towards |x| - 0.5: the centre is inside, the corner outside
        s = geo.forward_sdf(torch.tensor([[0.0, 0.0, 0.0], [0.9, 0.9, 0.9]], device="cuda"))
    assert float(s[0]) < float(s[1])


def test_initialize_shape_is_not_run_without_a_request():
    import scaledreamer_amd.plugins  # noqa: F401
    from scaledreamer_amd.registry import find

    geo = find("implicit-sdf")({}).cuda()
    before = geo.sdf_network.layers[0].weight.detach().clone()
    geo.initialize_shape()
    assert torch.equal(before, geo.sdf_network.layers[0].weight.detach()) and not hasattr(geo, "shape_init_losses")


def test_export_of_an_exact_sphere(tmp_path):
    """network output zeroed: sdf = |x| - 0.5 exactly.  mt-grid at resolution 32, threshold 0, no outlier removal: every vertex lies on a grid
    edge that crosses the sphere, within one grid cell (2 / 31) of radius 0.5"""
    from scaledreamer_amd.registry import find

    torch.manual_seed(0)
    cfg = _sdf_preset()["system"]
    cfg.update(guidance_type="", optimizer={}, exporter={"fmt": "obj", "save_uv": False, "save_normal": True})
    cfg["geometry"].update(isosurface_method="mt-grid", isosurface_resolution=32, isosurface_threshold=0.0)
    system = find("scaledreamer-system")(cfg).eval()
    geo = system.geometry
    assert geo.cfg.isosurface_remove_outliers is False
    with torch.no_grad():
        geo.sdf_network.layers[2].weight.zero_()
        x = torch.tensor([[0.3, 0.4, 0.0], [0.0, 0.0, 0.0], [1.0, 0.0, 0.0]], device="cuda")
        torch.testing.assert_close(geo.forward_sdf(x)[:, 0], torch.tensor([0.0, -0.5, 0.5], device="cuda"), rtol=0, atol=1e-6)
    paths = system.export(str(tmp_path))
    assert paths and paths[-1].endswith(".obj") and os.path.exists(paths[-1])
    v = np.array([[float(t) for t in line.split()[1:4]] for line in open(paths[-1]) if line.startswith("v ")])
    f = [line for line in open(paths[-1]) if line.startswith("f ")]
    assert v.shape[0] > 100 and len(f) > 100
    r = np.linalg.norm(v, axis=1)
    print(f"{v.shape[0]} vertices, {len(f)} faces, radius in [{r.min():.4f}, {r.max():.4f}]")
    assert np.abs(r - 0.5).max() <= 2.0 / 31.0
