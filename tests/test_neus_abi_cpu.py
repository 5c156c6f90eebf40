"""The NeuS entries (include/asd_hip.h: asd_neus_*) at the C boundary, without a GPU: declared, listed, exported, and every argument check
answers before the HIP runtime is touched — a NULL required pointer or a negative size is an error with a message, zero rays / samples is
OK without a launch."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["asd_neus_step_alpha", "asd_neus_prune_count", "asd_neus_composite_fwd", "asd_neus_composite_bwd"]

P = C.c_void_p(0x1000)          # a non-NULL pointer that no accepted call may dereference on the host (and no launch happens in these tests)
NULL = C.c_void_p(0)
i32, f32 = C.c_int32, C.c_float


def _calls(n):
    """name -> (argument list with every required pointer set, indices of the REQUIRED pointers, index of the size argument)"""
    common = [P, P, P, P, P, P, i32(1), P, f32(0.5), i32(0), P, P, P, i32(n)]
    return {
        "asd_neus_step_alpha": ([P, i32(n), NULL, P, f32(0.01), i32(0), P, NULL], [0, 3, 6]),
        "asd_neus_prune_count": ([P, P, P, i32(n), P, f32(0.01), i32(0), f32(1e-4), f32(0.01), P, P, NULL], [0, 1, 2, 4, 9, 10]),
        "asd_neus_composite_fwd": (common + [P, P, P, P, P, NULL, NULL], [0, 1, 2, 3, 4, 5, 7, 10, 11, 12, 14, 15, 16, 17, 18]),
        "asd_neus_composite_bwd": (common + [P, P, NULL, NULL, NULL, NULL, NULL, P, NULL, P, NULL, NULL, NULL, NULL],
                                   [0, 1, 2, 3, 4, 5, 7, 10, 11, 12, 14, 15, 21, 23]),
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
        assert getattr(_lib.lib(), n).argtypes, f"{n} has no argtypes"


def _rejected(name, args):
    lib = _lib()
    rc = getattr(lib, name)(*args)
    return rc != 0 and name.encode() in lib.asd_last_error()


@pytest.mark.parametrize("name", NAMES)
def test_zero_size_is_ok_without_a_launch(name):
    args, _ = _calls(0)[name]
    assert getattr(_lib(), name)(*args) == 0


@pytest.mark.parametrize("name", NAMES)
def test_null_required_pointers_are_reported(name):
    args, required = _calls(0)[name]          # (zero size: were a check missing, the call would return OK instead of launching on a bad pointer)
    for idx in required:
        bad = list(args)
        bad[idx] = NULL
        assert _rejected(name, bad), f"{name}: argument {idx} = NULL was accepted"


@pytest.mark.parametrize("name", NAMES)
def test_negative_sizes_are_reported(name):
    assert _rejected(name, _calls(-1)[name][0]), f"{name}: a size of -1 was accepted"


def test_dependent_arguments_are_reported():
    lib = _lib()
    for name in ("asd_neus_composite_fwd", "asd_neus_composite_bwd"):
        args, _ = _calls(0)[name]
        args[6] = i32(2)
        assert getattr(lib, name)(*args) != 0 and b"color_act" in lib.asd_last_error()
    args, _ = _calls(0)["asd_neus_composite_bwd"]
    args[25] = P                                  # a variance gradient without its partial-sum buffer
    assert lib.asd_neus_composite_bwd(*args) != 0 and b"partial" in lib.asd_last_error()
