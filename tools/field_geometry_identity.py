"""What the five field geometries hand the kernels and get back, as one file per tree — to show that a refactor of their Python layer
(geometry.py, sdf_geometry.py, hyper.py, sampled_geometry.py) changes nothing:

    [ASD_HIP_LIB=/path/to/libasd_hip.so] python tools/field_geometry_identity.py --out DIR          (GPU box; writes DIR/field_geometry.pt)
    python tools/field_geometry_identity.py --compare REF.pt OTHER.pt [--noise REF_AGAIN.pt]        (anywhere)

The run is seeded on the host.  `implicit-volume` (finite-difference and analytic normals), `implicit-sdf`, `Hyper-iNGP`, `3DConv-net` and
`Triplane-transformer-sdf`, B = 2 and n = 3001 where there is a batch, points reaching 10 % beyond the box: forward with and without normal
and the sdf-only (density-only) call, each under grad with random upstream gradients and again under no_grad.  Every output, every gradient
(grid or cache, every head weight, for Hyper-iNGP the hypernetwork's output weights) and the bytes of `_fcfg` go into the file.  The package
is imported from the tree this file lies in: copy it next to another tree's scaledreamer_amd/ to record that tree.

--compare: forward outputs and cfg bytes must be equal bit for bit.  The scatters sum through atomics, so two runs of ONE code are the
yardstick for a gradient (--noise, a second run of REF's tree): it may differ from REF by at most twice what REF's two runs differ by, and
is equal where those are equal.  Prints one row per tensor and exits 1 when a row fails (profiles/field_geometry_identity.txt)."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

N, RADIUS = 3001, 2.0
GRID = {"otype": "HashGrid", "n_levels": 16, "n_features_per_level": 2, "log2_hashmap_size": 16, "base_resolution": 16,
        "per_level_scale": 1.447269237440378}
SDF = {"radius": RADIUS, "normal_type": "finite_difference", "finite_difference_normal_eps": 0.01, "sdf_bias": "sphere", "sdf_bias_params": 0.8}
VOXEL_GEN = dict(z_dim=64, w_dim=256, c_dim=1024, num_layers=2, img_resolution=16, img_channels=32, channel_multiplier=1)
TRI_GEN = dict(backend="library", inner_dim=64, condition_dim=128, triplane_low_res=32, triplane_high_res=64, triplane_dim=32, num_layers=1,
               num_heads=4, local_text=True, mlp_ratio=4)
CASES = {          # name -> (registry name, config, how the cache is made: None = no cache)
    "volume": ("implicit-volume", {"radius": RADIUS, "pos_encoding_config": GRID}, None),
    "volume_analytic": ("implicit-volume", {"radius": RADIUS, "pos_encoding_config": GRID, "normal_type": "analytic"}, None),
    "sdf": ("implicit-sdf", dict(SDF, pos_encoding_config=GRID), None),
    "hyper": ("Hyper-iNGP", dict(SDF, pos_encoding_config=GRID), "hypernet"),
    "voxel": ("3DConv-net", dict(SDF, space_generator_config=VOXEL_GEN), (2, 32, 16, 16, 16)),
    "triplane": ("Triplane-transformer-sdf", dict(SDF, space_generator_config=TRI_GEN), (2, 3, 32, 64, 64)),
}


def record(name, out):
    import scaledreamer_amd.plugins  # noqa: F401
    from scaledreamer_amd.registry import find

    reg, cfg, cache_kind = CASES[name]
    g = torch.Generator().manual_seed(1234)
    torch.manual_seed(1234)          # the modules' default initialisation draws from the global generator
    geo = find(reg)(cfg)
    if hasattr(geo, "encoding"):
        with torch.no_grad():
            p = geo.encoding.encoding.encoding.params
            p.copy_(torch.randn(p.shape, generator=g) * 0.1)
    geo = geo.cuda()
    geo.do_update_step(0, 0)
    assert geo._fcfg is not None, name
    out[f"cfg/{name}"] = torch.frombuffer(bytearray(bytes(geo._fcfg)), dtype=torch.uint8).clone()
    batched = cache_kind is not None
    pts = ((torch.rand((2, N, 3) if batched else (N, 3), generator=g) * 2 - 1) * 1.1 * RADIUS).cuda()
    text = torch.randn(2, 768, generator=g).cuda()
    volume = torch.randn(cache_kind, generator=g) * 0.5 if isinstance(cache_kind, tuple) else None
    ups = {k: torch.randn(2 * N if batched else N, d, generator=g).cuda()          # the random upstream gradients, one per output name
           for k, d in (("density", 1), ("sdf", 1), ("features", 3), ("normal", 3), ("sdf_grad", 3))}
    sdf_only = geo.forward_density if reg == "implicit-volume" else geo.forward_sdf

    def cache():
        """a fresh cache per evaluation: (what forward takes, the leaves whose gradient is recorded)"""
        if cache_kind is None:
            return (), {}
        if cache_kind == "hypernet":
            c = geo.generate_space_cache(None, text)
            leaves = {f"{k}{i}": w for k, ws in c.items() for i, w in enumerate(ws)}
            for w in leaves.values():
                if w.requires_grad:
                    w.retain_grad()
            return (c,), leaves
        c = volume.clone().cuda().requires_grad_(True)
        return (c,), {"cache": c}

    def grads(tag, leaves):
        for k, p in geo.named_parameters():
            if p.grad is not None:
                out[f"grad/{name}/{tag}/{k}"] = p.grad.detach().cpu().clone()
                p.grad = None
        for k, t in leaves.items():
            if t.grad is not None:
                out[f"grad/{name}/{tag}/{k}"] = t.grad.detach().cpu().clone()

    for normal in (True, False):
        tag = "normal" if normal else "plain"
        args, leaves = cache()
        res = geo(pts, *args, output_normal=normal)
        for k, v in res.items():
            out[f"out/{name}/{tag}/{k}"] = v.detach().cpu().clone()
        sum((v * ups[k].view_as(v)).sum() for k, v in res.items() if k != "shading_normal").backward()
        grads(tag, leaves)
        with torch.no_grad():
            for k, v in geo(pts, *cache()[0], output_normal=normal).items():
                out[f"out/{name}/{tag}_nograd/{k}"] = v.cpu().clone()
    args, leaves = cache()
    s = sdf_only(pts, *args)
    out[f"out/{name}/only/sdf"] = s.detach().cpu().clone()
    if s.requires_grad:          # Hyper-iNGP's forward_sdf is a no_grad evaluation
        (s * ups["sdf"].view_as(s)).sum().backward()
        grads("only", leaves)
    with torch.no_grad():
        out[f"out/{name}/only_nograd/sdf"] = sdf_only(pts, *cache()[0]).cpu().clone()
    torch.cuda.synchronize()


def compare(ref, other, noise, noisy=("grad/",)):
    """`noisy`: the key prefixes judged against the run-to-run difference of REF's tree; everything else must be equal bit for bit"""
    a, b = torch.load(ref), torch.load(other)
    c = torch.load(noise) if noise else None
    bad = sorted(set(a) ^ set(b))
    for k in bad:
        print(f"{k}: in one file only")
    dist = lambda x, y: float((x.double() - y.double()).abs().max()) if x.numel() else 0.0  # noqa: E731
    print(f"# {'tensor':68s} {'shape':>20s} {'max|ref|':>10s} {'ref-ref2':>10s} {'ref-other':>10s}")
    for k in sorted(set(a) & set(b)):
        if a[k].shape != b[k].shape:
            print(f"{k}: shape {tuple(a[k].shape)} against {tuple(b[k].shape)}")
            bad.append(k)
            continue
        d_other = dist(a[k], b[k])
        d_noise = dist(a[k], c[k]) if c is not None and k in c else None
        if k.startswith(noisy):
            ok = d_other <= 2 * d_noise if d_noise is not None else torch.equal(a[k], b[k])
        else:
            ok = torch.equal(a[k], b[k])
        if not ok:
            bad.append(k)
        print(f"  {k:68s} {str(tuple(a[k].shape)):>20s} {float(a[k].double().abs().max()):10.3e} "
              f"{'-' if d_noise is None else format(d_noise, '10.3e'):>10s} {d_other:10.3e}  {'ok' if ok else 'FAIL'}")
    n = {kind: sum(k.startswith(kind) for k in a) for kind in ("out/", "grad/", "cfg/")}
    print(f"# {n['out/']} outputs, {n['grad/']} gradients, {n['cfg/']} cfg structs; {len(bad)} failing")
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--compare", nargs=2, metavar=("REF", "OTHER"))
    ap.add_argument("--noise", metavar="REF_AGAIN")
    a = ap.parse_args()
    if a.compare:
        sys.exit(compare(*a.compare, a.noise))
    os.makedirs(a.out, exist_ok=True)
    out = {}
    for name in CASES:
        record(name, out)
        print(f"{name}: {sum(k.split('/')[1] == name for k in out)} tensors", flush=True)
    torch.save(out, os.path.join(a.out, "field_geometry.pt"))


if __name__ == "__main__":
    main()
