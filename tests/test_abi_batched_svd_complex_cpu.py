"""CPU checks of the batched complex truncated SVD at the drop-in boundary: rc_svd_rank_batched_c64 / _c32 are declared in
include/rusty_compression_amd.h, exported by the built library, reachable through the C++ mirror's svd_rank_batched<c64> /
<c32>, and reject a null context before touching a device."""
import ctypes
import os

from rusty_compression_amd import _lib
from tests.test_abi_cpu import build_cpp_mirror_examples

SYMBOLS = ["rc_svd_rank_batched_c64", "rc_svd_rank_batched_c32"]


def test_complex_batched_svd_symbols_are_declared_and_exported():
    declared = set(_lib.declared_symbols())
    lib = _lib.lib()
    for s in SYMBOLS:
        assert s in declared, s
        assert hasattr(lib, s), s


def test_complex_batched_svd_entry_points_reject_a_null_context():
    lib = _lib.lib()
    none = _lib.mat(None)
    for s in SYMBOLS:
        assert getattr(lib, s)(ctypes.c_void_p(None), none, ctypes.c_int64(0), ctypes.c_int32(0), ctypes.c_int64(1), ctypes.c_double(0.0), none,
                               ctypes.c_int64(0), None, none, ctypes.c_int64(0), None) == _lib.RC_INVALID_ARGUMENT


def test_cpp_mirror_reaches_the_complex_batched_svd(tmp_path):
    exe = build_cpp_mirror_examples(tmp_path, "batched_svd_complex_example.cpp")
    assert os.path.exists(exe)
