"""CPU side of the analytic-normal feature: the float64 oracle of field_analytic_util.py is checked against the C oracle's encode, the
`implicit-volume` eligibility rules for normal_type "analytic", and the recorded E32 values the GPU tests take their bounds from."""
import numpy as np
import pytest
import torch

import field_analytic_util as U


@pytest.mark.parametrize("meta_name", ["A", "B"])
def test_restated_encode_equals_the_c_oracle(oracle, meta_name):
    meta, P, pts, _ = U.draw(meta_name, 257)
    om = oracle.grid_meta(*U.METAS[meta_name])
    assert bytes(om) == bytes(meta)
    u = ((pts + U.RADIUS) / (2 * U.RADIUS)).astype(np.float32)
    want = oracle.hashgrid_fwd(om, P.grid, u)
    table = torch.tensor(P.grid).view(-1, 2)
    got32, _ = U.encode(meta, table, torch.tensor(u))
    got64, pos = U.encode(meta, table.double(), torch.tensor(u).double())
    # float32 rounding, per level: the position s u + 0.5 <= s + 1 is rounded to an ulp, 2^-23 (s + 1) at most (the C oracle fuses the
    # multiply-add, torch rounds twice); that moves the weights along each of the 3 axes by as much, and the value by that times the
    # difference of two corner values (< 1 for tables in (-0.5, 0.5)); the 8-term sum itself adds a few 2^-24
    tol = np.repeat([3 * 2.0 ** -23 * (float(meta.scale[l]) + 1) + 8 * 2.0 ** -24 for l in range(16)], 2)
    assert (np.abs(got32.numpy() - want) <= tol).all()
    assert (np.abs(got64.numpy() - want) <= tol).all()
    assert pos.shape == (257, 16, 3)


def test_analytic_is_fused_eligible_and_the_rest_refuse():
    import scaledreamer_amd.plugins  # noqa: F401
    from scaledreamer_amd.registry import find

    geo = find("implicit-volume")
    assert geo({"normal_type": "analytic"}).fused
    assert geo({"normal_type": "analytic", "n_feature_dims": 0}).fused
    mlp32 = {"otype": "VanillaMLP", "activation": "ReLU", "output_activation": "none", "n_neurons": 32, "n_hidden_layers": 1}
    with pytest.raises(NotImplementedError, match=r"fused field kernels only.*n_neurons 32"):
        geo({"normal_type": "analytic", "mlp_network_config": mlp32})
    enc_xyz = {"otype": "HashGrid", "n_levels": 16, "n_features_per_level": 2, "log2_hashmap_size": 19, "base_resolution": 16,
               "per_level_scale": 1.447269237440378, "include_xyz": True}
    with pytest.raises(NotImplementedError, match=r"fused field kernels only.*include_xyz"):
        geo({"normal_type": "analytic", "pos_encoding_config": enc_xyz})
    with pytest.raises(NotImplementedError, match=r"fused field kernels only.*n_feature_dims 8"):
        geo({"normal_type": "analytic", "n_feature_dims": 8})
    with pytest.raises(NotImplementedError, match="derivative of the hash grid"):
        find("implicit-sdf")({"normal_type": "analytic"})
    # the other normal types keep their routes
    assert geo({"normal_type": "finite_difference"}).fused and not geo({"normal_type": "pred"}).fused


@pytest.mark.parametrize("key", ["A/softplus_magic3d/257", "A/truncexp_dreamfusion/257", "A/softplus_magic3d/1", "B/softplus_magic3d/257"])
def test_recorded_e32_is_reproducible_from_the_seeds(key):
    """The float32 run's matrix products go through the CPU's BLAS, whose summation order differs between machines: the recomputed
    max-norm errors must agree with the recorded ones within a factor of 1.5, and the left-out share must be the recorded count."""
    meta, cfg, n = key.split("/")
    c = U.case(meta, cfg, int(n))
    left = int((~c.keep).sum())
    assert left == {"A/softplus_magic3d/257": 5, "A/truncexp_dreamfusion/257": 5, "A/softplus_magic3d/1": 0, "B/softplus_magic3d/257": 11}[key]
    assert left <= U.MAX_LEFT_OUT * c.n
    assert set(c.e32) == set(U.E32[key])
    for k, v in U.E32[key].items():
        assert v / 1.5 <= c.e32[k] <= v * 1.5, (k, v, c.e32[k])
