"""What the three volume renderers return on every route, as one file per tree — to show that a refactor of their Python layer
(nerfacc_api.py, renderer.py, neus_renderer.py, volsdf_renderer.py) changes nothing:

    [ASD_HIP_LIB=/path/to/libasd_hip.so] python tools/renderer_identity.py --out DIR          (GPU box; writes DIR/renderer.pt)
    python tools/renderer_identity.py --compare REF.pt OTHER.pt [--noise REF_AGAIN.pt]        (anywhere)

The run is seeded on the host and the jitter is injected.  Per case: every entry of the output dictionary (deferred ones forced) in the
order the dictionary lists them, `last_n_samples`, and every parameter gradient of a loss that weights every differentiable entry with a
seeded random tensor.
    nerf    implicit-volume, no-material (requires_normal), neural-environment-map-background: the three training routes (fused pass, composed
            pass with the kept count on the device, count-reading pass), each with the four forms of bg_color and on an all-miss batch; eval
    neus    implicit-sdf: ASD_NEUS 1 and 0, use_volsdf both ways; training, eval, all-miss
    volsdf  a small Hyper-iNGP: ASD_VOLSDF 1 and 0; training and eval
The package is imported from the tree this file lies in: copy tools/ next to another tree's scaledreamer_amd/ to record that tree.

--compare is tools/field_geometry_identity.py's, with outputs judged like gradients: a tensor that two runs of REF's tree (--noise) give
bit for bit must be equal bit for bit, one that they do not (sums through atomics: field gradients, the index_add_ behind comp_normal) may
differ from REF by at most twice what REF's two runs differ by.  Key sets must be equal (profiles/renderer_identity.txt)."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from field_geometry_identity import compare  # noqa: E402

GRID = {"otype": "HashGrid", "n_levels": 16, "n_features_per_level": 2, "log2_hashmap_size": 12, "base_resolution": 16,
        "per_level_scale": 1.447269237440378}
BG_ENC = {"otype": "HashGrid", "n_features_per_level": 2, "log2_hashmap_size": 12, "n_levels": 4, "base_resolution": 4, "per_level_scale": 4.0}
HYPER = {"c_dim": 1024, "out_dims": {"sdf_weights": [64, 1], "feature_weights": [64, 3]}, "spectral_norm": False, "n_neurons": 64, "n_hidden_layers": 1}
B, H, W = 2, 16, 16


def camera_rays(gen, eye_radius):
    """pinhole rays from B cameras on a sphere looking at the origin, [B, H, W, 3] on the device"""
    eye = F.normalize(torch.randn(B, 3, generator=gen), dim=-1) * eye_radius
    fwd = F.normalize(-eye, dim=-1)
    right = F.normalize(torch.cross(fwd, torch.tensor([[0.0, 0.0, 1.0]]).expand(B, -1), dim=-1), dim=-1)
    up = torch.cross(right, fwd, dim=-1)
    ys, xs = torch.meshgrid((torch.arange(H) + 0.5) / H - 0.5, (torch.arange(W) + 0.5) / W - 0.5, indexing="ij")
    d = fwd[:, None, None, :] + 0.9 * xs[None, :, :, None] * right[:, None, None, :] - 0.9 * ys[None, :, :, None] * up[:, None, None, :]
    return eye[:, None, None, :].expand(B, H, W, 3).contiguous().cuda(), F.normalize(d, dim=-1).contiguous().cuda()


def miss_rays():
    o = torch.full((B, H, W, 3), 5.0, device="cuda")
    return o, F.normalize(torch.ones(B, H, W, 3, device="cuda"), dim=-1)


def record(out, tag, ren, modules, call, train):
    """one forward (and, in training, one backward under seeded upstream gradients) of `call`; everything it gives goes into `out`"""
    gen = torch.Generator().manual_seed(99)
    params = {f"{m}.{k}": p for m, mod in modules.items() for k, p in mod.named_parameters()}
    for p in params.values():
        p.grad = None
    for mod in list(modules.values()) + [ren]:
        mod.train(train)
    with torch.set_grad_enabled(train):
        res = call()
    keys = list(res.keys())
    out[f"out/{tag}/_key_order"] = torch.tensor(list("\n".join(keys).encode()), dtype=torch.uint8)
    loss = 0.0
    for k in keys:
        v = res[k]
        out[f"out/{tag}/{k}"] = v.detach().cpu().clone()
        if train and v.requires_grad:
            loss = loss + (v * torch.randn(v.shape, generator=gen).cuda()).sum()
    if hasattr(ren, "last_n_samples"):
        out[f"out/{tag}/_last_n_samples"] = torch.tensor(ren.last_n_samples)
    if train:
        loss.backward()
        for k, p in params.items():
            if p.grad is not None:
                out[f"grad/{tag}/{k}"] = p.grad.detach().cpu().clone()
    torch.cuda.synchronize()


def build(names, ren_cfg, seed):
    import scaledreamer_amd.plugins  # noqa: F401
    from scaledreamer_amd.registry import find

    torch.manual_seed(seed)
    geo_name, geo_cfg, bg_name, bg_cfg, ren_name = names
    geo = find(geo_name)(geo_cfg).cuda()
    mat = find("no-material")({"n_output_dims": 3, "color_activation": "sigmoid", "requires_normal": True}).cuda()
    bg = find(bg_name)(bg_cfg).cuda()
    ren = find(ren_name)(ren_cfg, geometry=geo, material=mat, background=bg).cuda()
    with torch.no_grad():          # a hash table with something in it
        p = geo.encoding.encoding.encoding.params
        p.copy_((torch.randn(p.shape, generator=torch.Generator().manual_seed(seed)) * 0.1).cuda())
    for m in (geo, mat, bg, ren):
        m.train()
    geo.do_update_step(0, 0)
    ren.do_update_step(0, 0)          # the warm-up occupancy update from the field, where the renderer keeps a grid
    return ren, {"geo": geo, "bg": bg, "ren": ren}


def nerf(out):
    from scaledreamer_amd.renderer import NeRFVolumeRenderer

    gen = torch.Generator().manual_seed(1)
    ren, mods = build(("implicit-volume", {"radius": 1.0, "normal_type": "finite_difference", "pos_encoding_config": GRID},
                       "neural-environment-map-background", {"color_activation": "sigmoid", "random_aug": False, "dir_encoding_config": BG_ENC},
                       "nerf-volume-renderer"), {"radius": 1.0, "num_samples_per_ray": 64}, 11)
    ro, rd = camera_rays(gen, 1.25)
    jit = torch.rand(B * H * W, generator=gen).cuda()
    ren.jitter_fn = lambda n, device: jit
    colour = torch.rand(B, 3, generator=gen).cuda()
    image = torch.rand(B, H, W, 3, generator=gen).cuda()
    forms = {"bg_none": None, "bg_per_view": colour, "bg_image": image, "bg_flat": image.reshape(-1, 3)}
    fused_ok = NeRFVolumeRenderer._fused_pass_ok
    for route in ("fused", "sync_free", "count"):
        os.environ["ASD_SYNC_FREE"] = "0" if route == "count" else "1"
        NeRFVolumeRenderer._fused_pass_ok = (lambda self, n_rays: False) if route == "sync_free" else fused_ok
        for form, c in forms.items():
            record(out, f"nerf/{route}/{form}", ren, mods, lambda: ren(rays_o=ro, rays_d=rd, light_positions=ro[:, 0, 0], bg_color=c), True)
        mo, md = miss_rays()
        record(out, f"nerf/{route}/all_miss", ren, mods, lambda: ren(rays_o=mo, rays_d=md, light_positions=mo[:, 0, 0]), True)
    NeRFVolumeRenderer._fused_pass_ok = fused_ok
    os.environ.pop("ASD_SYNC_FREE")
    record(out, "nerf/eval", ren, mods, lambda: ren(rays_o=ro, rays_d=rd, light_positions=ro[:, 0, 0]), False)


def neus(out):
    gen = torch.Generator().manual_seed(2)
    ro, rd = camera_rays(gen, 1.25)
    jit = torch.rand(B * H * W, generator=gen).cuda()
    mo, md = miss_rays()
    for volsdf in (False, True):
        ren, mods = build(("implicit-sdf", {"radius": 1.0, "sdf_bias": "sphere", "sdf_bias_params": 0.5, "pos_encoding_config": GRID},
                           "neural-environment-map-background", {"color_activation": "sigmoid", "random_aug": False, "dir_encoding_config": BG_ENC},
                           "neus-volume-renderer"), {"radius": 1.0, "num_samples_per_ray": 128, "use_volsdf": volsdf}, 12)
        ren.jitter_fn = lambda n, device: jit
        for route in ("1", "0"):
            os.environ["ASD_NEUS"] = route
            tag = f"neus/{'volsdf' if volsdf else 'neus'}/route{route}"
            record(out, f"{tag}/train", ren, mods, lambda: ren(rays_o=ro, rays_d=rd, light_positions=ro[:, 0, 0]), True)
            record(out, f"{tag}/all_miss", ren, mods, lambda: ren(rays_o=mo, rays_d=md, light_positions=mo[:, 0, 0]), True)
            record(out, f"{tag}/eval", ren, mods, lambda: ren(rays_o=ro, rays_d=rd, light_positions=ro[:, 0, 0]), False)
    os.environ.pop("ASD_NEUS")


def volsdf(out):
    gen = torch.Generator().manual_seed(3)
    ren, mods = build(
        ("Hyper-iNGP", {"radius": 2.0, "normal_type": "finite_difference", "finite_difference_normal_eps": 0.01, "sdf_bias": "sphere",
                        "sdf_bias_params": 0.5, "shape_init": "sphere", "shape_init_params": 0.5, "hypernet_config": HYPER, "pos_encoding_config": GRID},
         "multiprompt-neural-hashgrid-environment-map-background",
         {"color_activation": "sigmoid", "random_aug": False, "pos_encoding_config": dict(GRID, per_level_scale=1.0)},
         "generative-space-volsdf-volume-renderer"),
        {"radius": 2.0, "use_volsdf": True, "trainable_variance": True, "learned_variance_init": 0.340119, "estimator": "importance",
         "num_samples_per_ray": 16, "num_samples_per_ray_importance": 32, "near_plane": 0.1, "far_plane": 4.0, "train_chunk_size": 0}, 13)
    ro, rd = camera_rays(gen, 1.25)
    text = torch.randn(B, 1024, generator=gen).cuda()
    jitters = [torch.rand(B * H * W, generator=gen).cuda() for _ in range(2)]
    colour = torch.rand(B, 3, generator=gen).cuda()

    def call(bg_color=None):
        jit = list(jitters)
        ren.estimator.jitter_fn = lambda n, device: jit.pop(0)
        return ren(rays_o=ro, rays_d=rd, light_positions=ro[:, 0, 0], text_embed=text, bg_color=bg_color)

    for route in ("1", "0"):
        os.environ["ASD_VOLSDF"] = route
        record(out, f"volsdf/route{route}/train", ren, mods, call, True)
        record(out, f"volsdf/route{route}/train_bg_per_view", ren, mods, lambda: call(colour), True)
        record(out, f"volsdf/route{route}/eval", ren, mods, call, False)
    os.environ.pop("ASD_VOLSDF")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--compare", nargs=2, metavar=("REF", "OTHER"))
    ap.add_argument("--noise", metavar="REF_AGAIN")
    a = ap.parse_args()
    if a.compare:
        sys.exit(compare(*a.compare, a.noise, noisy=("grad/", "out/")))
    os.makedirs(a.out, exist_ok=True)
    out = {}
    for case in (nerf, neus, volsdf):
        case(out)
        print(f"{case.__name__}: {sum(k.split('/')[1] == case.__name__ for k in out)} tensors", flush=True)
    torch.save(out, os.path.join(a.out, "renderer.pt"))


if __name__ == "__main__":
    main()
