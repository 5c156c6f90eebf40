"""CPU side of the field geometries' Python layer (geometry.py, sdf_geometry.py, hyper.py, sampled_geometry.py): what each class writes into
the asd_field_cfg it hands the kernels, and which fused entry the two sampled classes call how often, with which flags, shapes and weights.
Nothing here needs a device: the structs are filled on the host, and the call trace runs over stand-ins for the four ops entries."""
import collections

import numpy as np
import pytest
import torch

from scaledreamer_amd import _lib

GRID = {"n_levels": 16, "n_features_per_level": 2, "log2_hashmap_size": 19, "base_resolution": 16, "per_level_scale": 1.447269237440378}
MLP = {"otype": "VanillaMLP", "activation": "ReLU", "output_activation": "none", "n_neurons": 64}
VOXEL_GEN = {"z_dim": 64, "w_dim": 256, "c_dim": 1024, "num_layers": 2, "img_resolution": 16, "img_channels": 32, "channel_multiplier": 1}
TRI_GEN = {"backend": "library", "inner_dim": 64, "condition_dim": 128, "triplane_low_res": 32, "triplane_high_res": 64, "triplane_dim": 32,
           "num_layers": 1, "num_heads": 4, "local_text": True, "mlp_ratio": 4}
SDF = {"radius": 2.0, "sdf_bias": "sphere", "sdf_bias_params": 0.8, "finite_difference_normal_eps": 0.01}
GENERATOR = {"implicit-sdf": {}, "Hyper-iNGP": {}, "3DConv-net": {"space_generator_config": VOXEL_GEN},
             "Triplane-transformer-sdf": {"space_generator_config": TRI_GEN}}


def _f32(v):
    return float(np.float32(v))


def _build(name, **over):
    import scaledreamer_amd.plugins  # noqa: F401
    from scaledreamer_amd.registry import find

    geo = find(name)({**GENERATOR.get(name, {}), **over})
    geo.do_update_step(0, 0)
    return geo


def _fields(f):
    return {"bbox_min": tuple(f.bbox_min), "bbox_max": tuple(f.bbox_max), "radius": f.radius, "bias_mode": f.bias_mode,
            "bias_value": f.bias_value, "blob_scale": f.blob_scale, "blob_std": f.blob_std, "activation": f.activation, "fd_eps": f.fd_eps,
            "n_hidden": f.n_hidden, "n_feature_dims": f.n_feature_dims, "field_mode": f.field_mode}


def test_field_cfg_struct_has_the_fields_the_table_names():
    assert [n for n, _ in _lib.FieldCfg._fields_] == list(_fields(_lib.FieldCfg()))


def test_field_cfg_of_the_four_sdf_classes():
    want = {"bbox_min": (-2.0,) * 3, "bbox_max": (2.0,) * 3, "radius": 2.0, "bias_mode": _lib.ASD_BIAS_SPHERE, "bias_value": _f32(0.8),
            "blob_scale": 0.0, "blob_std": 1.0, "activation": _lib.ASD_ACT_NONE, "fd_eps": _f32(0.01), "n_hidden": 64, "n_feature_dims": 3,
            "field_mode": _lib.ASD_FIELD_SDF}
    structs = {name: _build(name, **SDF)._fcfg for name in GENERATOR}
    for name, f in structs.items():
        assert f is not None, name
        assert _fields(f) == want, name
    assert len({bytes(f) for f in structs.values()}) == 1


@pytest.mark.parametrize("name", list(GENERATOR))
def test_field_cfg_float_bias_is_the_constant_mode(name):
    f = _build(name, radius=2.0, sdf_bias=0.25, finite_difference_normal_eps=0.01)._fcfg
    assert (f.bias_mode, f.bias_value, f.field_mode) == (_lib.ASD_BIAS_CONST, 0.25, _lib.ASD_FIELD_SDF)


def test_field_cfg_of_implicit_volume_defaults():
    geo = _build("implicit-volume", radius=1.0)
    assert geo.fused and geo._fused_blockers == []
    assert _fields(geo._fcfg) == {
        "bbox_min": (-1.0,) * 3, "bbox_max": (1.0,) * 3, "radius": 1.0, "bias_mode": _lib.ASD_BIAS_BLOB_MAGIC3D, "bias_value": 0.0,
        "blob_scale": 10.0, "blob_std": 0.5, "activation": _lib.ASD_ACT_SOFTPLUS, "fd_eps": _f32(0.01), "n_hidden": 64, "n_feature_dims": 3,
        "field_mode": _lib.ASD_FIELD_DENSITY}


def test_field_cfg_is_none_where_the_kernels_do_not_apply():
    ellipsoid = {**SDF, "sdf_bias": "ellipsoid", "sdf_bias_params": [0.5, 0.6, 0.7]}
    for name in GENERATOR:
        assert _build(name, **ellipsoid)._fcfg is None, name
    assert _build("3DConv-net", **SDF, mlp_network_config={**MLP, "n_hidden_layers": 2})._fcfg is None
    assert _build("Triplane-transformer-sdf", **SDF, mlp_network_config={**MLP, "n_hidden_layers": 1})._fcfg is None
    # the eligible counterparts of the two lines above are the classes' defaults (test_field_cfg_of_the_four_sdf_classes)
    import scaledreamer_amd.plugins  # noqa: F401
    from scaledreamer_amd.registry import find

    assert find("Hyper-iNGP")(dict(SDF))._fcfg is None          # its predicate needs the eps that the first update_step sets


def test_field_cfg_progressive_eps_of_implicit_sdf():
    import scaledreamer_amd.plugins  # noqa: F401
    from scaledreamer_amd.registry import find

    band = {"otype": "ProgressiveBandHashGrid", **GRID, "start_level": 4, "start_step": 100, "update_steps": 50}
    geo = find("implicit-sdf")({**SDF, "pos_encoding_config": band, "finite_difference_normal_eps": "progressive"})
    assert geo.fused and geo._fcfg.fd_eps == _f32(0.01)          # the stand-in until update_step has run
    before = bytes(geo._fcfg)
    for step, level in ((0, 4), (400, 10), (10 ** 6, 16)):
        geo.do_update_step(0, step)
        eps = 2 * 2.0 / (16 * 1.447269237440378 ** (level - 1))
        assert geo.finite_difference_normal_eps == eps
        assert geo._fcfg.fd_eps == _f32(eps)
    geo._fcfg.fd_eps = 0.01
    assert bytes(geo._fcfg) == before          # update_step touches nothing else


# ---- call trace of the two sampled classes -----------------------------------------------------------------------------------------------
TRI_W6 = ((96, 64), (64, 64), (1, 64), (96, 64), (64, 64), (3, 64))
VOX_DW = ((64, 32), (1, 64), (64, 32), (3, 64))
TRI_DW = ((64, 96), (64, 64), (1, 64), (64, 96), (64, 64), (3, 64))


class _Trace:
    """CPU stand-ins for ops.voxfield_fwd / _bwd / trifield_fwd / _bwd: ones of the documented shapes forward; backward adds 1.0 into the
    cache-gradient slice it is given and returns weight gradient k filled with k + 1"""

    def __init__(self):
        self.fwd, self.bwd = [], []

    @staticmethod
    def _outputs(n, want_normal, want_features):
        one = lambda *s: torch.ones(s)
        return one(n), one(n, 3) if want_features else None, one(n, 3) if want_normal else None, one(n, 3) if want_normal else None

    @staticmethod
    def _shape(t):
        return None if t is None else tuple(t.shape)

    def voxfield_fwd(self, voxel_cl, cfg, w1s, w2s, w1f, w2f, points, want_normal, want_features=True, save_enc=True):
        assert isinstance(cfg, _lib.FieldCfg) and voxel_cl.is_contiguous() and points.is_contiguous() and points.dtype == torch.float32
        self.fwd.append(("voxfield_fwd", tuple(voxel_cl.shape), tuple(tuple(w.shape) for w in (w1s, w2s, w1f, w2f)), tuple(points.shape),
                         bool(want_normal), bool(want_features), bool(save_enc)))
        return (*self._outputs(points.shape[0], want_normal, want_features), torch.ones(points.shape[0], 32) if save_enc else None)

    def trifield_fwd(self, planes_cl, cfg, weights6, points, want_normal, want_features=True):
        assert isinstance(cfg, _lib.FieldCfg) and planes_cl.is_contiguous() and points.is_contiguous() and points.dtype == torch.float32
        assert len(weights6) == 6 and all(w.is_contiguous() for w in weights6)
        self.fwd.append(("trifield_fwd", tuple(planes_cl.shape), tuple(tuple(w.shape) for w in weights6), tuple(points.shape),
                         bool(want_normal), bool(want_features), None))
        return self._outputs(points.shape[0], want_normal, want_features)

    def _backward(self, name, cache, weights, points, enc, sdf, grads, d_cache, dw_shapes):
        assert sdf.shape == (points.shape[0],) and all(g is None or g.is_contiguous() for g in grads)
        assert d_cache.shape == cache.shape and d_cache.is_contiguous()
        self.bwd.append((name, tuple(cache.shape), tuple(tuple(w.shape) for w in weights), tuple(points.shape), self._shape(enc),
                         tuple(self._shape(g) for g in grads), tuple(d_cache.shape)))
        d_cache.add_(1.0)
        return tuple(torch.full(s, k + 1.0) for k, s in enumerate(dw_shapes))

    def voxfield_bwd(self, voxel_cl, cfg, w1s, w2s, w1f, w2f, points, enc, sdf, d_sdf, d_features, d_normal, d_fd_grad, d_voxel):
        return self._backward("voxfield_bwd", voxel_cl, (w1s, w2s, w1f, w2f), points, enc, sdf, (d_sdf, d_features, d_normal, d_fd_grad),
                              d_voxel, VOX_DW)

    def trifield_bwd(self, planes_cl, cfg, weights6, points, sdf, d_sdf, d_features, d_normal, d_fd_grad, d_planes):
        assert all(w.is_contiguous() for w in weights6)
        return self._backward("trifield_bwd", planes_cl, weights6, points, None, sdf, (d_sdf, d_features, d_normal, d_fd_grad), d_planes, TRI_DW)


@pytest.mark.parametrize("kind", ["voxel", "triplane"])
def test_call_trace_of_the_sampled_classes(kind, monkeypatch):
    from scaledreamer_amd import ops

    vox = kind == "voxel"
    geo = _build("3DConv-net" if vox else "Triplane-transformer-sdf", **SDF)
    trace = _Trace()
    for entry in ("voxfield_fwd", "voxfield_bwd", "trifield_fwd", "trifield_bwd"):
        monkeypatch.setattr(ops, entry, getattr(trace, entry))
    monkeypatch.setattr(type(geo), "_use_fused", lambda self, points: True)
    gen = torch.Generator().manual_seed(0)
    if vox:          # channel-last in memory, as the HIP generators hand their output over: no transpose kernel on the way in
        cache = torch.rand(2, 16, 16, 16, 32, generator=gen).movedim(-1, 1)
        entry, fwd, bwd, w_shapes = (16, 16, 16, 32), "voxfield_fwd", "voxfield_bwd", VOX_DW
    else:
        cache = torch.rand(2, 3, 64, 64, 32, generator=gen).permute(0, 1, 4, 2, 3)
        entry, fwd, bwd, w_shapes = (3, 64, 64, 32), "trifield_fwd", "trifield_bwd", TRI_W6
    cache.requires_grad_(True)
    pts = torch.rand(2, 7, 3, generator=gen) * 2 - 1
    pts5 = torch.rand(2, 5, 3, generator=gen)

    out = geo(pts, cache, output_normal=True)
    s = geo.forward_sdf(pts5, cache)
    (sum(v.sum() for v in out.values()) + s.sum()).backward()
    with torch.no_grad():
        out_ng = geo(pts, cache, output_normal=False)
        s_ng = geo.forward_sdf(pts, cache)

    # forward calls, in order; every one sees ONE cache entry (and the tri-plane entry six contiguous weights, first layers transposed)
    call = lambda n, want_normal, want_features, save_enc: (fwd, entry, w_shapes, (n, 3), want_normal, want_features, save_enc if vox else None)
    assert trace.fwd == (2 * [call(7, True, True, True)] + 2 * [call(5, False, True, True)]          # forward_sdf under grad runs the node
                         + 2 * [call(7, False, True, False)] + 2 * [call(7, False, False, False)])
    # backward calls, as a multiset: autograd decides the order
    back = lambda n, grads: (bwd, entry, w_shapes, (n, 3), (n, 32) if vox else None, grads, entry)
    assert collections.Counter(trace.bwd) == collections.Counter(
        2 * [back(5, ((5,), None, None, None))] + 2 * [back(7, ((7,), (7, 3), (7, 3), (7, 3)))])

    assert out["sdf"].shape == (14, 1) and s.shape == (2, 5, 1)
    assert sorted(out) == ["features", "normal", "sdf", "sdf_grad", "shading_normal"]
    assert all(out[k].shape == (14, 3) for k in ("features", "normal", "shading_normal", "sdf_grad"))
    assert sorted(out_ng) == ["features", "sdf"] and out_ng["sdf"].shape == (14, 1) and out_ng["features"].shape == (14, 3)
    assert s_ng.shape == (2, 7, 1) and not s_ng.requires_grad and not out_ng["sdf"].requires_grad
    # ONE shared gradient buffer per cache, hit twice per entry (the forward and the sdf-only evaluation)
    assert cache.grad.shape == cache.shape and bool((cache.grad == 2.0).all())
    # 2 entries x 2 evaluations, each returning k + 1 for weight k, in the parameter's own layout: a permuted tuple or a lost transpose shows
    weights = geo._heads_weights()
    assert len(weights) == len(w_shapes)
    for k, w in enumerate(weights):
        assert w.grad.shape == w.shape and bool((w.grad == 4.0 * (k + 1)).all()), k
