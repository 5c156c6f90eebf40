"""No IEEE-rounded fp32 division inside the GroupNorm / SiLU streaming kernels: the library is built without
fast-math, so a plain `a / b` in a kernel is v_div_scale x2 + v_rcp + v_fma x4-5 + v_div_fmas + v_div_fixup, and that made the passes
over the VAE's large tensors VALU-bound.  tools/isa_mix.py compiles the sources with the Makefile's flags and counts; needs hipcc only."""
import functools
import importlib.util
import os
import re
import shutil

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "scaledreamer_amd", "csrc")


@functools.lru_cache(maxsize=None)
def _analyse(source):      # one compile per source and session
    return _isa_mix().analyse(os.path.join(CSRC, source))


def _isa_mix():
    spec = importlib.util.spec_from_file_location("isa_mix", os.path.join(ROOT, "tools", "isa_mix.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _have_hipcc():
    return os.path.exists("/opt/rocm/bin/hipcc") or shutil.which("hipcc") is not None


@pytest.mark.skipif(not _have_hipcc(), reason="hipcc is not installed")
@pytest.mark.parametrize("source,kernels", [
    ("nn_ops.hip", ["gn_apply_kernel", "gn_bwd_stats_kernel", "gn_bwd_apply_kernel", "silu_kernel"]),
    ("gemm.hip", ["splitk_epilogue_gnapply_kernel"]),
])
def test_no_ieee_division_in_the_silu_streaming_kernels(source, kernels):
    res = _analyse(source)
    for k in kernels:
        found = [n for n in res if re.match(re.escape(k) + r"\b", n.replace("void ", ""))]
        assert found, f"{k} not found in the assembly of {source}: {sorted(res)}"
        for n in found:
            t = res[n]["total"]
            assert t["v_div_scale"] == 0, f"{n}: {t['v_div_scale']} v_div_scale_f32 (an fp32 `/` came back; use the helpers of asd_common.h)"
            assert t["valu"] > 0 and t["loads"] > 0        # the counts are of a real kernel body
    # every instance of the templated kernels was seen: SiLU on / off, dx_add on / off, both block widths
    if source == "nn_ops.hip":
        assert len([n for n in res if "gn_bwd_stats_kernel" in n]) == 4 and len([n for n in res if "gn_bwd_apply_kernel" in n]) == 4


@pytest.mark.skipif(not _have_hipcc(), reason="hipcc is not installed")
def test_backward_statistics_main_loop_is_light():
    """the two-row loop of gn_bwd_stats_kernel<512, SiLU>: 45 VALU per element pair with the division (361 per trip of 16 elements),
    26 without; one basic block (SiLU is a template parameter, no branch per channel)"""
    res = _analyse("nn_ops.hip")
    name = [n for n in res if re.search(r"gn_bwd_stats_kernel<512, (1|true)>", n)]
    assert len(name) == 1, sorted(res)
    loop = res[name[0]]["main_loop"]
    assert loop["blocks"] == 1 and loop["v_exp"] == loop["v_rcp"] and loop["v_exp"] > 0
    assert loop["valu"] <= 17 * loop["v_exp"], loop     # <= 17 VALU per element (13 today), 22.6 before
