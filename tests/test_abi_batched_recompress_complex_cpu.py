"""CPU checks of the batched recompression of complex factors at the drop-in boundary: rc_lowrank_recompress_complex_batched_c64 / _c32
are declared in include/rusty_compression_amd.h, exported by the built library and present in the Rust binding's ffi.rs, reject a null
context before touching a device, are reachable from Python and through the C++ mirror's recompress_batched overloads for c64 and c32."""
import ctypes
import os

import rusty_compression_amd as rc
from rusty_compression_amd import _lib
from tests.test_abi_cpu import build_cpp_mirror_examples

SYMBOLS = [f"rc_lowrank_recompress_complex_batched_{s}" for s in ("c64", "c32")]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_complex_batched_recompress_symbols_are_declared_exported_and_bound():
    declared = set(_lib.declared_symbols())
    lib = _lib.lib()
    with open(os.path.join(ROOT, "bindings", "rust", "src", "ffi.rs")) as f:
        ffi = f.read()
    for s in SYMBOLS:
        assert s in declared, s
        assert hasattr(lib, s), s
        assert f"pub fn {s}(" in ffi, s


def test_complex_batched_recompress_entry_points_reject_a_null_context():
    lib = _lib.lib()
    none = _lib.mat(None)
    zero = ctypes.c_int64(0)
    for s, tol in zip(SYMBOLS, (ctypes.c_double(0.0), ctypes.c_float(0.0))):  # tol has the real type of the data
        assert getattr(lib, s)(ctypes.c_void_p(None), none, zero, none, zero, None, zero, none, zero, None, ctypes.c_int32(0), ctypes.c_int64(1),
                               tol, none, zero, None, none, zero, None) == _lib.RC_INVALID_ARGUMENT


def test_python_names_exist():
    for name in ("lowrank_recompress_batched_complex", "column_id_to_svd_batched_complex", "two_sided_id_to_svd_batched_complex",
                 "svd_add_batched_complex"):
        assert callable(getattr(rc, name)), name
        assert name in rc.__all__, name


def test_cpp_mirror_reaches_the_complex_batched_recompress(tmp_path):
    exe = build_cpp_mirror_examples(tmp_path, "batched_recompress_complex_example.cpp")
    assert os.path.exists(exe)
