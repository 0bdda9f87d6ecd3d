"""CPU: the host half of the group form of the FLAC stage: the symbol and its binding, the ABI version, and
the range checks that are answered before any HIP call (there is no GPU here, so an answer at all shows where they sit).

Rows of two designs (sample rate, block size) are refused as well, but that case needs two objects, and fq3_flac_create allocates device
memory: it is left to tests/test_gpu_flac_group.py (test_all_or_nothing), as are the per-row checks against an object's state."""
import ctypes as C
import os
import re

from fq3hip import _lib
from fq3hip import audio_out

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "fq3_flac_push_group"


def test_symbol_and_binding():
    lib = _lib.load()
    ptrs, i64s, ints = C.POINTER(C.c_void_p), C.POINTER(C.c_int64), C.POINTER(C.c_int)
    assert NAME in _lib.SIGNATURES and hasattr(lib, NAME)
    res, got = _lib.SIGNATURES[NAME]
    assert res is C.c_int and got == [ptrs, C.c_int, ptrs, i64s, ints, ptrs, i64s, i64s, ptrs, C.c_void_p]
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fq3hip.h")).read(), flags=re.S)
    declared = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % NAME, hdr).group(1).split(",")
    assert len(declared) == len(got) and declared[1].split() == ["int", "B"] and declared[-1].split() == ["void*", "stream"]
    assert declared[-2].split() == ["int64_t*", "const*", "n_bytes_dev"]       # host array of device pointers
    assert _lib.FQ3_STAGE_GROUP_MAX == audio_out.GROUP_MAX == 32
    lib.fq3_abi_version.restype = C.c_int
    assert lib.fq3_abi_version() == 5                                # additive: the version stays


def test_range_checks_come_before_any_hip_call():
    lib = _lib.load()
    fn = getattr(lib, NAME)
    one_p, one_l, one_i = (C.c_void_p * 1)(None), (C.c_int64 * 1)(0), (C.c_int * 1)(0)
    full = [one_p, 1, one_p, one_l, one_i, one_p, one_l, one_l, one_p, None]
    for B in (-1, 33, 1 << 20):
        assert fn(*(full[:1] + [B] + full[2:])) == _lib.FQ3_EINVAL, B
        assert b"32" in lib.fq3_last_error() and NAME.encode() in lib.fq3_last_error()
    for at in (0, 2, 3, 4, 5, 6, 7, 8):                              # every array
        args = list(full)
        args[at] = None
        assert fn(*args) == _lib.FQ3_EINVAL, at
        assert b"null array" in lib.fq3_last_error()
    assert fn(*full) == _lib.FQ3_EINVAL and b"row 0: null object" in lib.fq3_last_error()      # a null object in the array
    assert fn(*([None, 0] + [None] * (len(full) - 2))) == 0          # B == 0: nothing to do


def test_the_same_object_twice_is_refused_before_it_is_read():
    """the duplicate check compares pointers only, so any two equal non-null entries reach it -- here the address of a host buffer
    that is large enough to be read as an object, should the order of the checks ever change"""
    lib = _lib.load()
    fake = (C.c_uint8 * 256)()
    two_p = (C.c_void_p * 2)(C.addressof(fake), C.addressof(fake))
    none_p, two_l, two_i = (C.c_void_p * 2)(None, None), (C.c_int64 * 2)(0, 0), (C.c_int * 2)(0, 0)
    assert getattr(lib, NAME)(two_p, 2, none_p, two_l, two_i, none_p, two_l, two_l, none_p, None) == _lib.FQ3_EINVAL
    assert b"rows 0 and 1 are the same object" in lib.fq3_last_error()


def test_python_group_path_answers_without_a_gpu():
    assert audio_out.push_group([], [], []) == [] and audio_out.push_group_host([], [], []) == []
