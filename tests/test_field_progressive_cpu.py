"""CPU side of the coarse-to-fine SDF route: the schedule of ProgressiveBandHashGrid and of finite_difference_normal_eps "progressive"
against the reference's own numbers (tests/golden/progressive_band.npz, made by make_goldens_progressive.py), the level limit in the grid
meta, configuration errors, state-dict keys, the ABI struct size, and the guards of the GPU tests' oracle (field_progressive_util.py: E32
is reproducible from the seeds, the left-out share stays under its cap)."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import field_progressive_util as U
from golden_util import GOLDEN_DIR

GRID = {"n_levels": 16, "n_features_per_level": 2, "log2_hashmap_size": 19, "base_resolution": 16, "per_level_scale": 1.447269237440378}


def _find(name):
    import scaledreamer_amd.plugins  # noqa: F401
    from scaledreamer_amd.registry import find

    return find(name)


def _band(g=None, **over):
    cfg = {"otype": "ProgressiveBandHashGrid", **GRID, "start_level": 4, "start_step": 100, "update_steps": 50}
    if g is not None:
        cfg.update(start_level=int(g["start_level"]), start_step=int(g["start_step"]), update_steps=int(g["update_steps"]))
    cfg.update(over)
    return cfg


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(GOLDEN_DIR, "progressive_band.npz")))


def _mask_of(meta):
    m = np.zeros(int(meta.n_levels) * 2, np.float32)
    m[: 2 * (int(meta.n_levels) - int(meta.n_masked_levels))] = 1.0
    return m


def test_schedule_mask_and_eps_equal_the_reference_at_every_step(golden):
    geo = _find("implicit-sdf")({"radius": float(golden["radius"]), "pos_encoding_config": _band(golden), "finite_difference_normal_eps": "progressive"})
    band = geo.encoding.encoding
    assert type(band).__name__ == "ProgressiveBandHashGrid" and geo.fused
    assert geo._meta is band.encoding.meta          # ONE ctypes object: what update_step writes is what the kernels are handed
    for i, step in enumerate(int(s) for s in golden["steps"]):
        geo.do_update_step(0, step)
        assert band.current_level == int(golden["current_level"][i]), step
        np.testing.assert_array_equal(_mask_of(geo._meta), golden["mask"][i], err_msg=f"step {step}")
        assert geo.finite_difference_normal_eps == float(golden["fd_eps"][i]), step         # the reference's own expression: bit-equal
        assert geo._fcfg.fd_eps == np.float32(golden["fd_eps"][i]), step


def test_meta_follows_the_schedule_with_the_references_two_quirks():
    from scaledreamer_amd.networks import CompositeEncoding, ProgressiveBandHashGrid, get_encoding

    enc = get_encoding(3, _band())
    assert isinstance(enc, CompositeEncoding) and isinstance(enc.encoding, ProgressiveBandHashGrid)
    band, meta = enc.encoding, enc.encoding.encoding.meta
    assert (band.n_output_dims, band.n_level, band.n_features_per_level) == (32, 16, 2)
    assert (band.start_level, band.start_step, band.update_steps, band.current_level) == (4, 100, 50, 4)
    # quirk 1: before the first update_step the reference's mask is all zero although current_level reads start_level
    assert meta.n_masked_levels == 16 and band.n_active_levels == 0
    enc.do_update_step(0, 0)
    assert meta.n_masked_levels == 12 and band.current_level == 4
    enc.do_update_step(0, 400)
    assert meta.n_masked_levels == 6 and band.current_level == 10
    # quirk 2: the mask only grows — a step counter that goes backwards lowers current_level, no level is switched off
    enc.do_update_step(0, 150)
    assert band.current_level == 5 and meta.n_masked_levels == 6
    enc.do_update_step(0, 10 ** 6)
    assert band.current_level == 16 and meta.n_masked_levels == 0


def test_config_errors_keep_their_messages():
    from scaledreamer_amd.networks import get_encoding

    for otype in ("ProgressiveBandFrequency", "HashGridSpatialTime"):
        with pytest.raises(NotImplementedError, match="out of scope"):
            get_encoding(3, {"otype": otype, **GRID})
    sdf, vol = _find("implicit-sdf"), _find("implicit-volume")
    with pytest.raises(NotImplementedError, match="ProgressiveBandHashGrid"):
        sdf({"finite_difference_normal_eps": "progressive"})
    with pytest.raises(NotImplementedError, match="ProgressiveBandHashGrid"):
        sdf({"finite_difference_normal_eps": "progressive", "pos_encoding_config": {"otype": "HashGrid", **GRID}})
    with pytest.raises(NotImplementedError, match="derivative of the hash grid"):
        sdf({"normal_type": "analytic", "pos_encoding_config": _band()})
    with pytest.raises(NotImplementedError, match="level limit"):
        vol({"normal_type": "analytic", "pos_encoding_config": _band()})
    # a progressive grid with a fixed eps, and implicit-volume on a progressive grid, are legal and fused
    assert sdf({"pos_encoding_config": _band()}).fused
    geo = vol({"pos_encoding_config": _band()})
    assert geo.fused and geo._meta.n_masked_levels == 16
    geo.do_update_step(0, 200)
    assert geo._meta.n_masked_levels == 10
    # the composed route (ellipsoid bias) runs through the same encoding object
    comp = sdf({"pos_encoding_config": _band(), "finite_difference_normal_eps": "progressive", "sdf_bias": "ellipsoid", "sdf_bias_params": [0.5, 0.5, 0.5]})
    assert not comp.fused
    comp.do_update_step(0, 200)
    assert comp._meta.n_masked_levels == 10 and comp.finite_difference_normal_eps == 2.0 / (16 * 1.447269237440378 ** 5)


def test_state_dict_keys_equal_those_of_the_plain_grid():
    sdf = _find("implicit-sdf")
    plain = sdf({"pos_encoding_config": {"otype": "HashGrid", **GRID}})
    prog = sdf({"pos_encoding_config": _band(), "finite_difference_normal_eps": "progressive"})
    assert list(prog.state_dict().keys()) == list(plain.state_dict().keys())
    assert "encoding.encoding.encoding.params" in prog.state_dict()
    with open(os.path.join(GOLDEN_DIR, "neus_state_dict_keys.json")) as f:
        assert sorted(prog.state_dict().keys()) == json.load(f)["geometry"]          # the reference's keys: its checkpoint loads
    prog.load_state_dict(plain.state_dict())


def test_sizeof_grid_meta_is_unchanged(oracle):
    from scaledreamer_amd import _lib

    assert C.sizeof(_lib.GridMeta) == C.sizeof(type(oracle.grid_meta())) == 16 + 5 * 4 * _lib.ASD_MAX_LEVELS
    assert _lib.GridMeta.reserved.offset == 12          # the word asd_grid_meta.n_masked_levels names; GridMeta.n_masked_levels is its property
    m = _lib.GridMeta()
    m.n_masked_levels = 5
    assert m.reserved == 5 and m.n_masked_levels == 5
    m = _lib.make_grid_meta(16, 2, 19, 16, 1.447269237440378)
    assert m.n_masked_levels == 0          # asd_grid_meta_init zeroes it: every existing caller gets the plain grid
    assert bytes(m) == bytes(oracle.grid_meta())


def test_golden_encodings_are_the_oracle_encode_times_the_mask(oracle, golden):
    """what the GPU tests compare the kernels with bit for bit is what the reference's ProgressiveBandHashGrid returns"""
    from golden_util import grid_params

    table = grid_params(int(golden["seed"]), 12_599_920, float(golden["grid_amp"]))
    full = oracle.hashgrid_fwd(oracle.grid_meta(), table, golden["x"])
    assert not golden["enc_before_update"].any()
    for a in (4, 6, 16):
        np.testing.assert_array_equal(golden[f"enc_{a}"], full * U.column_mask(a).numpy().astype(np.float32))


@pytest.mark.parametrize("key", ["A/4", "A/5", "A/6", "A/16", "B/4", "B/5", "B/6", "B/16"])
def test_left_out_share_is_under_its_cap_and_e32_is_reproducible(key):
    """The float32 run's matrix products go through the CPU's BLAS, whose summation order differs between machines: the recomputed
    max-norm errors must agree with the recorded ones within a factor of 1.5 (the bound of test_field_analytic_cpu.py)."""
    meta_name, a = key.split("/")
    c = U.case(meta_name, int(a))
    left = int((~c.keep).sum())
    assert left == U.LEFT_OUT[key]
    assert left <= U.MAX_LEFT_OUT * c.n
    assert set(c.e32) == set(U.E32[key])
    for k, v in U.E32[key].items():
        assert v / 1.5 <= c.e32[k] <= v * 1.5, (k, v, c.e32[k])


@pytest.mark.parametrize("key", ["A/0", "B/0", "A/1", "B/1"])
def test_forward_e32_of_the_exact_zero_cases(key):
    meta_name, a = key.split("/")
    c = U.case(meta_name, int(a), with_bwd=False)
    assert set(c.e32) == set(U.E32[key])
    for k, v in U.E32[key].items():
        assert v / 1.5 <= c.e32[k] <= v * 1.5, (k, v, c.e32[k])
    if a == "0":
        assert c.keep.all() and not c.ref.features.any()
        bias = torch.as_tensor(c.pts).double().norm(dim=-1) - U.CFG["bias_value"]
        assert float((c.ref.sdf - bias).abs().max()) <= 1e-15          # no level active: the sdf is the bias
