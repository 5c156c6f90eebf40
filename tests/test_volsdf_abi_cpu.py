"""The pass-level VolSDF entries (include/asd_hip.h: asd_volsdf_*) at the C boundary, without a GPU: declared, listed, exported, and every
argument check answers before the HIP runtime is touched — a NULL required pointer, a negative ray count or S <= 0 is an error with a message,
zero rays is OK without a launch."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["asd_volsdf_edges", "asd_volsdf_samples", "asd_volsdf_proposal_cdf", "asd_volsdf_composite_fwd", "asd_volsdf_composite_bwd"]

P = C.c_void_p(0x1000)          # a non-NULL pointer that no accepted call may dereference on the host (and no launch happens in these tests)
NULL = C.c_void_p(0)
i32, f32 = C.c_int32, C.c_float


def _calls(n_rays, S):
    """name -> (argument list with every required pointer set, indices of the REQUIRED pointers)"""
    n, s = i32(n_rays), i32(S)
    return {
        "asd_volsdf_edges": ([P, P, n, i32(2), s, NULL, f32(0.1), f32(4.0), NULL, P, NULL], [0, 1, 9]),
        "asd_volsdf_samples": ([P, P, P, n, s, NULL, NULL, NULL, NULL, NULL, NULL], [0, 1, 2]),
        "asd_volsdf_proposal_cdf": ([P, P, P, n, s, P, NULL], [0, 1, 2, 5]),
        "asd_volsdf_composite_fwd": ([P, P, i32(1), NULL, P, P, P, n, s, P, P, P, P, P, P, NULL, NULL], [0, 1, 4, 5, 6, 9, 10, 11, 12, 13, 14]),
        "asd_volsdf_composite_bwd": ([P, P, i32(1), NULL, P, P, P, n, s, P, P, P, NULL, NULL, NULL, NULL, NULL, NULL, NULL, P, P, NULL, NULL, NULL, NULL],
                                     [0, 1, 4, 5, 6, 9, 10, 11, 19, 20]),
    }


def _lib():
    from scaledreamer_amd import _lib

    return _lib.lib()


def test_entries_are_declared_listed_and_exported():
    from scaledreamer_amd import _lib

    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "asd_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(asd_[a-z0-9_]+)\s*\(", src))
    lib = C.CDLL(_lib.LIB_PATH)
    for n in NAMES:
        assert n in declared, f"{n} is not declared in include/asd_hip.h"
        assert n in _lib.SYMBOLS, f"{n} is not listed in _lib.SYMBOLS"
        assert hasattr(lib, n), f"{n} is not exported"


def _rejected(name, args):
    lib = _lib()
    rc = getattr(lib, name)(*args)
    return rc != 0 and name.encode() in lib.asd_last_error()


@pytest.mark.parametrize("name", NAMES)
def test_zero_rays_is_ok_without_a_launch(name):
    args, _ = _calls(0, 193)[name]
    assert getattr(_lib(), name)(*args) == 0


@pytest.mark.parametrize("name", NAMES)
def test_null_required_pointers_are_reported(name):
    args, required = _calls(0, 193)[name]          # (zero rays: were a check missing, the call would return OK instead of launching on a bad pointer)
    for idx in required:
        bad = list(args)
        bad[idx] = NULL
        assert _rejected(name, bad), f"{name}: argument {idx} = NULL was accepted"


@pytest.mark.parametrize("name", NAMES)
def test_negative_ray_count_and_empty_rays_are_reported(name):
    assert _rejected(name, _calls(-1, 193)[name][0]), f"{name}: n_rays = -1 was accepted"
    for S in (0, -3):
        assert _rejected(name, _calls(0, S)[name][0]), f"{name}: S = {S} was accepted"
        assert _rejected(name, _calls(777, S)[name][0]), f"{name}: S = {S} was accepted"


def test_dependent_arguments_are_reported():
    lib = _lib()
    args, _ = _calls(0, 193)["asd_volsdf_composite_fwd"]
    args[3] = P                                   # normals without a comp_normal output
    assert lib.asd_volsdf_composite_fwd(*args) != 0 and b"comp_normal" in lib.asd_last_error()
    args[2], args[3] = i32(2), NULL
    assert lib.asd_volsdf_composite_fwd(*args) != 0 and b"color_act" in lib.asd_last_error()
    args, _ = _calls(0, 193)["asd_volsdf_composite_bwd"]
    args[18] = P                                  # a comp_normal gradient without the normals
    assert lib.asd_volsdf_composite_bwd(*args) != 0 and b"normals" in lib.asd_last_error()
    args[18], args[22] = NULL, P                  # a variance gradient without its partial-sum buffer
    assert lib.asd_volsdf_composite_bwd(*args) != 0 and b"partial" in lib.asd_last_error()
    args, _ = _calls(0, 4096)["asd_volsdf_proposal_cdf"]
    assert lib.asd_volsdf_proposal_cdf(*args) != 0 and b"proposal samples" in lib.asd_last_error()
