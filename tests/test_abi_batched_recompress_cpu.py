"""CPU checks of the batched recompression at the drop-in boundary: rc_lowrank_recompress_batched_f64 / _f32 are declared in
include/rusty_compression_amd.h, exported by the built library, reject a null context before touching a device, are reachable from
Python and through the C++ mirror's recompress_batched overloads."""
import ctypes
import os

import rusty_compression_amd as rc
from rusty_compression_amd import _lib
from tests.test_abi_cpu import build_cpp_mirror_examples

SYMBOLS = [f"rc_lowrank_recompress_batched_{s}" for s in ("f64", "f32")]


def test_batched_recompress_symbols_are_declared_and_exported():
    declared = set(_lib.declared_symbols())
    lib = _lib.lib()
    for s in SYMBOLS:
        assert s in declared, s
        assert hasattr(lib, s), s
    for s in ("c64", "c32"):  # real scalars only
        assert f"rc_lowrank_recompress_batched_{s}" not in declared


def test_batched_recompress_entry_points_reject_a_null_context():
    lib = _lib.lib()
    none = _lib.mat(None)
    zero = ctypes.c_int64(0)
    for s in SYMBOLS:
        assert getattr(lib, s)(ctypes.c_void_p(None), none, zero, none, zero, None, zero, none, zero, None, ctypes.c_int32(0), ctypes.c_int64(1),
                               ctypes.c_double(0.0), none, zero, None, none, zero, None) == _lib.RC_INVALID_ARGUMENT


def test_python_names_exist():
    for name in ("lowrank_recompress_batched", "column_id_to_svd_batched", "two_sided_id_to_svd_batched", "svd_add_batched"):
        assert callable(getattr(rc, name)), name
        assert name in rc.__all__, name


def test_cpp_mirror_reaches_the_batched_recompress(tmp_path):
    exe = build_cpp_mirror_examples(tmp_path, "batched_recompress_example.cpp")
    assert os.path.exists(exe)
