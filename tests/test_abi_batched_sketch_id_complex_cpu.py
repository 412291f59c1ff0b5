"""CPU checks of the batched sketched column ID of complex tall blocks at the drop-in boundary: rc_sketch_column_id_rank_complex_batched_c64 /
_c32 are declared in include/rusty_compression_amd.h, exported by the built library and present in the Rust binding's ffi.rs, reject a null
context before touching a device, are reachable from Python and through the C++ mirror's column_id_rank_batched overload that takes a
test matrix, for c64 and c32."""
import ctypes
import os

import rusty_compression_amd as rc
from rusty_compression_amd import _lib
from tests.test_abi_cpu import build_cpp_mirror_examples

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = [f"rc_sketch_column_id_rank_complex_batched_{s}" for s in ("c64", "c32")]


def test_complex_batched_sketch_id_symbols_are_declared_exported_and_bound():
    declared = set(_lib.declared_symbols())
    lib = _lib.lib()
    with open(os.path.join(ROOT, "bindings", "rust", "src", "ffi.rs")) as f:
        ffi = f.read()
    for s in SYMBOLS:
        assert s in declared, s
        assert hasattr(lib, s), s
        assert f"pub fn {s}(" in ffi, s


def test_complex_batched_sketch_id_entry_points_reject_a_null_context():
    lib = _lib.lib()
    none = _lib.mat(None)
    zero = ctypes.c_int64(0)
    for s in SYMBOLS:  # the argument list of rc_sketch_column_id_rank_batched_f64
        assert getattr(lib, s)(ctypes.c_void_p(None), none, zero, none, zero, ctypes.c_int32(0), ctypes.c_int64(1), ctypes.c_double(0.0), none, zero,
                               none, zero, none, zero, None, None) == _lib.RC_INVALID_ARGUMENT


def test_python_name_exists():
    assert callable(rc.sketch_column_id_rank_batched_complex)
    assert "sketch_column_id_rank_batched_complex" in rc.__all__


def test_cpp_mirror_reaches_the_complex_batched_sketch_id(tmp_path):
    exe = build_cpp_mirror_examples(tmp_path, "batched_sketch_id_complex_example.cpp")
    assert os.path.exists(exe)
