"""CPU side of the occupancy-grid renderers' Python layer (nerfacc_api.py, renderer.py, neus_renderer.py): which ops entries the NeRF and
NeuS renderers and `OccGridEstimator.sampling` call in which order with which sizes and thresholds, what the output dictionary holds, what
the dummy sample of an all-miss batch looks like when it reaches compositing, and which background tensor compositing gets for every form
of `bg_color`.  Nothing here needs a device: the ops entries are plain-torch stand-ins (a fixed number of candidates per ray, every second
one kept), geometry / material / background are tiny modules.  Only the routes that read the kept count are reachable this way; the two
device-count routes are covered by tests/test_gpu_renderer_golden.py."""
import pytest
import torch
import torch.nn as nn

B, H, W, K = 2, 3, 3, 4          # 2 x 3 x 3 rays, K candidates per ray
NR = B * H * W
OCC_MEAN = 2.0 ** -8             # exact in fp32, also as the mean of 32^3 equal cells: alpha_thre = min(0.01, mean) = this


class _Ops:
    """recording stand-ins for the entries of scaledreamer_amd.ops the renderers call"""

    def __init__(self, miss=False):
        self.calls, self.bg, self.packed, self.miss, self.prune_vals = [], [], [], miss, []

    def pack_bits(self, binaries):
        self.calls.append(("pack_bits",))
        return torch.zeros((binaries.numel() + 31) // 32, dtype=torch.int32)

    def march(self, cfg, rays_o, rays_d, occ_bits, jitter=None, n_max=None):
        self.calls.append(("march", n_max, jitter is not None))
        nr, k = rays_o.shape[0], 0 if self.miss else K
        count = torch.full((nr,), k, dtype=torch.int32)
        offset = (torch.arange(nr, dtype=torch.int32) * k)
        n = nr * k if n_max is None else n_max
        ray_idx = torch.arange(nr, dtype=torch.int32).repeat_interleave(k)
        t0 = 1.0 + 0.25 * torch.arange(k, dtype=torch.float32).repeat(nr)
        t1 = t0 + 0.25
        pts = rays_o[ray_idx.long()] + rays_d[ray_idx.long()] * ((t0 + t1) / 2)[:, None]
        assert n == nr * k
        return count, offset, torch.tensor([nr * k], dtype=torch.int32), ray_idx, t0, t1, pts

    def _prune(self, name, vals, count, early_stop_eps, alpha_thre):
        self.calls.append((name, vals.shape[0], early_stop_eps, alpha_thre))
        self.prune_vals.append(vals.clone())
        keep = (torch.arange(vals.shape[0]) % 2 == 0).to(torch.uint8)
        return keep, (count // 2).to(torch.int32)

    def prune(self, sigma, t0, t1, offset, count, early_stop_eps, alpha_thre):
        return self._prune("prune", sigma, count, early_stop_eps, alpha_thre)

    def neus_prune(self, sdf, offset, count, inv_std_param, step, use_volsdf, early_stop_eps, alpha_thre):
        return self._prune("neus_prune", sdf, count, early_stop_eps, alpha_thre)

    def scan_i32(self, count):
        self.calls.append(("scan_i32", count.shape[0]))
        c = count.long()
        return (c.cumsum(0) - c).to(torch.int32), c.sum().to(torch.int32).reshape(1)

    def compact(self, rays_o, rays_d, offset, count, keep, t0, t1, kept_offset, n_out, zero_ray_idx=False):
        self.calls.append(("compact", keep is not None, n_out, zero_ray_idx))
        ray = torch.arange(count.shape[0]).repeat_interleave(count.long())
        sel = torch.ones(ray.shape[0], dtype=torch.bool) if keep is None else keep.bool()
        ri, k0, k1 = ray[sel], t0[sel], t1[sel]
        assert ri.shape[0] == n_out
        return ri, k0, k1, rays_o[ri] + rays_d[ri] * ((k0 + k1) / 2)[:, None], rays_d[ri]

    def composite_fwd(self, sigma, t0, t1, rgb, offset, count, bg, mode=0):
        self.calls.append(("composite_fwd", mode, sigma.shape[0]))
        self.bg.append(bg)
        self.packed.append((offset.clone(), count.clone()))
        nr, n = count.shape[0], sigma.shape[0]
        ray = torch.arange(nr).repeat_interleave(count.long())
        w = torch.full((n,), 0.125)
        op = torch.zeros(nr).index_add_(0, ray, w)
        fg = torch.zeros(nr, 3).index_add_(0, ray, w[:, None] * rgb.detach())
        comp = fg + (1 - op)[:, None] * bg if bg.shape[0] == nr else fg
        return dict(weights=w, opacity=op, depth=op * 2, rgb_fg=fg, z_var=op * 0.5, comp_rgb=comp)

    def composite_bwd(self, sigma, t0, t1, rgb, offset, count, bg, fwd, **kw):
        self.calls.append(("composite_bwd", kw.get("mode", 0), sigma.shape[0]))
        return torch.zeros_like(sigma), torch.zeros_like(rgb), torch.zeros_like(bg)

    def neus_composite_fwd(self, *a, **kw):
        raise AssertionError("the fused NeuS route needs a device")

    neus_composite_bwd = neus_composite_fwd

    def install(self, monkeypatch):
        from scaledreamer_amd import ops

        for name in ("pack_bits", "march", "prune", "neus_prune", "scan_i32", "compact", "composite_fwd", "composite_bwd",
                     "neus_composite_fwd", "neus_composite_bwd"):
            monkeypatch.setattr(ops, name, getattr(self, name))
        return self

    def sampler_calls(self):
        return [c for c in self.calls if c[0] != "pack_bits"]


class _Field(nn.Module):
    """density (NeRF) or sdf (NeuS) field with the geometries' call surface"""

    def __init__(self, sdf):
        super().__init__()
        self.key, self.w = "sdf" if sdf else "density", nn.Parameter(torch.tensor(0.5))

    def _value(self, points):
        return points.sum(-1, keepdim=True) * self.w + 1.0

    forward_density = forward_sdf = _value

    def forward(self, points, output_normal=False):
        out = {self.key: self._value(points), "features": points * self.w}
        if output_normal:
            n = torch.nn.functional.normalize(points + 1e-3, dim=-1)
            out.update({"normal": n, "shading_normal": n})
            if self.key == "sdf":
                out["sdf_grad"] = points * 2.0
        return out


class _Cfg:
    n_output_dims, color_activation = 3, "sigmoid"


class _Material(nn.Module):
    requires_normal, reads_normal, cfg = True, False, _Cfg()

    def forward(self, features, **kw):
        return torch.sigmoid(features)


class _Background(nn.Module):
    def forward(self, dirs):
        return dirs * 0.5 + 0.25


def _renderer(name, **cfg):
    import scaledreamer_amd.plugins  # noqa: F401
    from scaledreamer_amd.registry import find

    ren = find(name)({"radius": 1.0, "num_samples_per_ray": 16, **cfg}, geometry=_Field(name.startswith("neus")), material=_Material(),
                     background=_Background())
    if ren.cfg.grid_prune:
        ren.estimator.occs.fill_(OCC_MEAN)
        ren.estimator.binaries.fill_(True)
    ren.jitter_fn = lambda n, device: torch.full((n,), 0.5)
    return ren


def _rays():
    g = torch.Generator().manual_seed(0)
    o = torch.rand(B, H, W, 3, generator=g) - 2.0
    d = torch.nn.functional.normalize(torch.rand(B, H, W, 3, generator=g) + 0.1, dim=-1)
    return o, d, o[:, 0, 0]


IMG = ["comp_rgb", "comp_rgb_fg", "comp_rgb_bg", "opacity", "depth", "z_variance"]
SAMPLE = ["weights", "t_points", "t_intervals", "t_dirs", "ray_indices", "points"]
SAMPLE_COLS = {"weights": 1, "t_points": 1, "t_intervals": 1, "t_dirs": 3, "ray_indices": None, "points": 3}
IMG_COLS = {"comp_rgb": 3, "comp_rgb_fg": 3, "comp_rgb_bg": 3, "opacity": 1, "depth": 1, "z_variance": 1, "comp_normal": 3}
GEO = {"nerf": {"density": 1, "features": 3, "normal": 3, "shading_normal": 3},
       "neus": {"sdf": 1, "features": 3, "normal": 3, "shading_normal": 3, "sdf_grad": 3}}
KEPT = NR * K // 2
# mode -> (renderer config, training, all rays miss, kept samples, the sampler's ops calls for NeRF; NeuS differs in the eval chunking only)
MODES = {
    "train": ({}, True, False, KEPT,
              [("march", None, True), ("prune", NR * K, 1e-4, OCC_MEAN), ("scan_i32", NR), ("compact", True, KEPT, False)]),
    "eval": ({}, False, False, KEPT,
             [("march", None, False), ("prune", NR * K, 1e-4, OCC_MEAN), ("scan_i32", NR), ("compact", True, KEPT, False)]),
    "no_grid_prune": ({"grid_prune": False}, True, False, NR * K, [("march", None, True), ("compact", False, NR * K, False)]),
    "all_miss": ({}, True, True, 1, [("march", None, True), ("prune", 0, 1e-4, OCC_MEAN), ("scan_i32", NR), ("compact", True, 0, False)]),
}


def _check_outputs(kind, out, keys, n, training):
    assert list(out.keys()) == keys
    for k in keys:
        v = out[k]
        if k == "inv_std":
            assert v.shape == () and v.dtype == torch.float32
        elif k in IMG_COLS:
            assert v.shape == (B, H, W, IMG_COLS[k]) and v.dtype == torch.float32, k
        elif k == "ray_indices":
            assert v.shape == (n,) and v.dtype == torch.int64
        else:
            cols = SAMPLE_COLS.get(k) or GEO[kind][k]
            assert v.shape == (n, cols) and v.dtype == torch.float32, k


@pytest.mark.parametrize("mode", list(MODES))
def test_nerf_route_calls_and_outputs(mode, monkeypatch):
    cfg, training, miss, n, sampler = MODES[mode]
    trace = _Ops(miss).install(monkeypatch)
    ren = _renderer("nerf-volume-renderer", **cfg)
    ren.train(training)
    o, d, light = _rays()
    with torch.set_grad_enabled(training):
        out = ren(rays_o=o, rays_d=d, light_positions=light)
    from scaledreamer_amd.renderer import LazyOutputs

    assert type(out) is LazyOutputs
    assert trace.sampler_calls() == sampler + [("composite_fwd", 0, n)]
    if training:          # the material asks for a normal that nothing in the call reads: deferred, behind the eager entries
        assert out.pending() == {"normal", "shading_normal"}
        keys = IMG + SAMPLE + ["density", "features", "normal", "shading_normal"]
    else:
        keys = IMG + ["comp_normal"]
    _check_outputs("nerf", out, keys, n, training)
    assert ren.last_n_samples == n and type(ren.last_n_samples) is int
    if miss:
        _check_dummy(trace, out)


@pytest.mark.parametrize("mode", list(MODES))
def test_neus_route_calls_and_outputs(mode, monkeypatch):
    cfg, training, miss, n, sampler = MODES[mode]
    trace = _Ops(miss).install(monkeypatch)
    ren = _renderer("neus-volume-renderer", **cfg)
    ren.train(training)
    o, d, light = _rays()
    with torch.set_grad_enabled(training):
        out = ren(rays_o=o, rays_d=d, light_positions=light)
    assert type(out) is dict
    assert trace.sampler_calls() == sampler + [("composite_fwd", 1, n)]          # without a device: the composed route, alpha compositing
    keys = IMG[:5] + (SAMPLE + list(GEO["neus"]) if training else ["comp_normal"]) + ["inv_std"]
    _check_outputs("neus", out, keys, n, training)
    assert ren.last_n_samples == n and type(ren.last_n_samples) is int
    if trace.prune_vals and not miss:          # the composed pruning pass gets -log(1 - alpha) / dt of the step alpha, alpha clamped to 1
        from scaledreamer_amd.sdf_opacity import step_alpha

        with torch.no_grad():
            t0 = 1.0 + 0.25 * torch.arange(K, dtype=torch.float32).repeat(NR)
            ri = torch.arange(NR).repeat_interleave(K)
            pts = o.reshape(-1, 3)[ri] + d.reshape(-1, 3)[ri] * (t0 + 0.125)[:, None]
            sdf = ren.geometry.forward_sdf(pts)[..., 0]
            alpha = step_alpha(sdf, ren.variance(sdf), ren.render_step_size, False)
            want = -torch.log1p(-alpha.clamp(max=1.0)) / 0.25
        torch.testing.assert_close(trace.prune_vals[0], want)
    if miss:
        _check_dummy(trace, out)


def _check_dummy(trace, out):
    """the one dummy sample of an all-miss batch as compositing sees it: ray 0 holds one sample at offset 0, every other ray none"""
    offset, count = trace.packed[-1]
    assert offset.dtype == count.dtype == torch.int32
    assert count.tolist() == [1] + [0] * (NR - 1) and offset.tolist() == [0] + [1] * (NR - 1)
    assert out["ray_indices"].tolist() == [0]
    assert float(out["t_points"].abs().max()) == 0.0 and float(out["t_intervals"].abs().max()) == 0.0


def test_nerf_grid_prune_without_alpha_threshold_runs_no_pruning_pass(monkeypatch):
    trace = _Ops().install(monkeypatch)
    ren = _renderer("nerf-volume-renderer", prune_alpha_threshold=False)
    o, d, light = _rays()
    ren(rays_o=o, rays_d=d, light_positions=light)
    assert trace.sampler_calls() == [("march", None, True), ("compact", False, NR * K, False), ("composite_fwd", 0, NR * K)]


BG = {"none": None, "per_view": (B, 3), "image": (B, H, W, 3), "flat": (NR, 3)}


@pytest.mark.parametrize("form", list(BG))
@pytest.mark.parametrize("name", ["nerf-volume-renderer", "neus-volume-renderer"])
def test_background_tensor_that_reaches_compositing(name, form, monkeypatch):
    trace = _Ops().install(monkeypatch)
    ren = _renderer(name)
    o, d, light = _rays()
    colour = None if BG[form] is None else torch.rand(BG[form], generator=torch.Generator().manual_seed(1))
    out = ren(rays_o=o, rays_d=d, light_positions=light, bg_color=colour)
    got = trace.bg[-1]
    if form == "none":
        want = out["comp_rgb_bg"].reshape(NR, 3)
    elif form == "per_view" and name.startswith("nerf"):
        want = colour[:, None, None, :].expand(B, H, W, 3).reshape(NR, 3)
    elif form == "per_view":          # NeuS hands a per-view colour on as it came (as the reference's neus_volume_renderer.py does)
        want = colour
    else:
        want = colour.reshape(NR, 3)
    assert got.shape == want.shape and got.dtype == torch.float32 and torch.equal(got, want.detach())
    assert out["comp_rgb"].shape == (B, H, W, 3)


@pytest.mark.parametrize("fn", ["sigma_fn", "alpha_fn", None])
def test_estimator_sampling_call_trace(fn, monkeypatch):
    from scaledreamer_amd.nerfacc_api import OccGridEstimator

    trace = _Ops().install(monkeypatch)
    est = OccGridEstimator(roi_aabb=[-1.0] * 3 + [1.0] * 3, resolution=32, levels=1)
    est.occs.fill_(OCC_MEAN)
    est.binaries.fill_(True)
    o, d, _ = _rays()
    o, d = o.reshape(-1, 3), d.reshape(-1, 3)
    seen = []

    def values(t0, t1, ray_idx):
        assert ray_idx.dtype == torch.int64 and t0.shape == t1.shape == ray_idx.shape == (NR * K,)
        seen.append(1)
        return torch.full((NR * K, 1), 0.5)

    res = est.sampling(o, d, render_step_size=0.1, alpha_thre=0.01, stratified=True, **({fn: values} if fn else {}))
    assert len(res) == 3
    ri, t0, t1 = res
    assert ri.dtype == torch.int64
    if fn is None:
        assert trace.sampler_calls() == [("march", None, True)] and ri.shape == (NR * K,)
        return
    assert trace.sampler_calls() == [("march", None, True), ("prune", NR * K, 1e-4, OCC_MEAN), ("scan_i32", NR), ("compact", True, KEPT, False)]
    assert seen == [1] and ri.shape == t0.shape == t1.shape == (KEPT,)
    want = torch.full((NR * K,), 0.5 if fn == "sigma_fn" else float(-torch.log1p(torch.tensor(-0.5)) / 0.25))
    torch.testing.assert_close(trace.prune_vals[0], want)
    with pytest.raises(AssertionError, match=r"must have shape of \(N,\)"):
        est.sampling(o, d, render_step_size=0.1, **{fn: lambda t0, t1, ri: torch.zeros(3)})
    with pytest.raises(ValueError, match="Only one of sigma_fn and alpha_fn"):
        est.sampling(o, d, sigma_fn=values, alpha_fn=values)
