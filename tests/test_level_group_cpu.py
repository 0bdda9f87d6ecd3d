"""CPU: the host half of the group form of the leveller and the limiter: the two symbols and their
bindings, the ABI version, and the range checks that are answered before any HIP call (there is no GPU here, so an answer at all shows
where they sit)."""
import ctypes as C
import inspect
import os
import re

from fq3hip import _lib
from fq3hip import leveller, limiter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbols_and_bindings():
    lib = _lib.load()
    ptrs, i64s, ints = C.POINTER(C.c_void_p), C.POINTER(C.c_int64), C.POINTER(C.c_int)
    want = {"fq3_leveller_push_group": [ptrs, C.c_int, ptrs, i64s, ints, ptrs, C.c_void_p],
            "fq3_limit_push_group": [ptrs, C.c_int, ptrs, i64s, ints, ptrs, i64s, i64s, C.c_void_p]}
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fq3hip.h")).read(), flags=re.S)
    for name, args in want.items():
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        res, got = _lib.SIGNATURES[name]
        assert res is C.c_int and got == args, name
        declared = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, hdr).group(1).split(",")
        assert len(declared) == len(args) and declared[1].split() == ["int", "B"] and declared[-1].split() == ["void*", "stream"], name
    assert not hasattr(lib, "fq3_loud_push_group")                   # the meters' group launch is the leveller's own business
    assert _lib.FQ3_STAGE_GROUP_MAX == leveller.GROUP_MAX == limiter.GROUP_MAX == 32
    lib.fq3_abi_version.restype = C.c_int
    assert lib.fq3_abi_version() == 5                                # additive: the version stays
    assert list(inspect.signature(leveller.push_group).parameters) == ["levellers", "pcms", "finals", "outs"]
    assert list(inspect.signature(limiter.push_group).parameters) == ["limiters", "pcms", "finals"]


def test_range_checks_come_before_any_hip_call():
    lib = _lib.load()
    one_p, one_l, one_i = (C.c_void_p * 1)(None), (C.c_int64 * 1)(0), (C.c_int * 1)(0)
    forms = {"fq3_leveller_push_group": ([one_p, 1, one_p, one_l, one_i, one_p, None], (0, 2, 3, 4, 5)),
             "fq3_limit_push_group": ([one_p, 1, one_p, one_l, one_i, one_p, one_l, one_l, None], (0, 2, 3, 4, 5, 6, 7))}
    for name, (full, arrays) in forms.items():
        fn = getattr(lib, name)
        for B in (-1, 33, 1 << 20):
            assert fn(*(full[:1] + [B] + full[2:])) == _lib.FQ3_EINVAL, (name, B)
            assert b"32" in lib.fq3_last_error() and name.encode() in lib.fq3_last_error()
        for at in arrays:                                            # every array
            args = list(full)
            args[at] = None
            assert fn(*args) == _lib.FQ3_EINVAL, (name, at)
            assert b"null array" in lib.fq3_last_error()
        assert fn(*full) == _lib.FQ3_EINVAL and b"null object" in lib.fq3_last_error()      # a null object in the array
        assert fn(*([None, 0] + [None] * (len(full) - 2))) == 0      # B == 0: nothing to do


def test_python_functions_answer_without_a_gpu():
    import pytest
    assert leveller.push_group([], [], []) == [] and limiter.push_group([], [], []) == []
    for fn in (leveller.push_group, limiter.push_group):
        with pytest.raises(ValueError, match="one pcm and one final flag"):
            fn([], [None], [])
