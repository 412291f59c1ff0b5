"""CPU checks of the mixed-storage calls at the drop-in boundary: rc_lowrank_apply_mixed_batched_f64 / _c64,
rc_block_operator_apply_mixed_f64 / _c64, rc_demote_batched_f64 / _c64 and rc_promote_batched_f32 / _c32 are declared in
include/rusty_compression_amd.h, exported by the built library, present in the generated Rust bindings, reject a null context before
touching a device, and are reachable from Python and through the C++ mirror."""
import ctypes
import os
import re

import rusty_compression_amd as rc
from rusty_compression_amd import _lib
from tests.test_abi_cpu import build_cpp_mirror_examples

APPLY = ["rc_lowrank_apply_mixed_batched_f64", "rc_lowrank_apply_mixed_batched_c64"]
OPERATOR = ["rc_block_operator_apply_mixed_f64", "rc_block_operator_apply_mixed_c64"]
DEMOTE = ["rc_demote_batched_f64", "rc_demote_batched_c64"]
PROMOTE = ["rc_promote_batched_f32", "rc_promote_batched_c32"]
SYMBOLS = APPLY + OPERATOR + DEMOTE + PROMOTE


def test_mixed_symbols_are_declared_exported_and_bound_for_rust():
    declared = set(_lib.declared_symbols())
    lib = _lib.lib()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ffi = set(re.findall(r"pub fn (rc_\w+)", open(os.path.join(root, "bindings", "rust", "src", "ffi.rs")).read()))
    assert len(SYMBOLS) == 8
    for s in SYMBOLS:
        assert s in declared, s
        assert hasattr(lib, s), s
        assert s in ffi, s


def test_mixed_entry_points_reject_a_null_context():
    lib = _lib.lib()
    null, none, zero, i0 = ctypes.c_void_p(None), _lib.mat(None), ctypes.c_int64(0), ctypes.c_int32(0)
    for s in APPLY:
        assert getattr(lib, s)(null, none, zero, none, zero, None, zero, none, zero, None, i0, none, zero, none, zero) == _lib.RC_INVALID_ARGUMENT
    for s in OPERATOR:
        assert getattr(lib, s)(null, none, zero, none, zero, None, zero, none, zero, None, i0, none, zero, i0, None, None, i0, None, None, none, none,
                               i0, i0) == _lib.RC_INVALID_ARGUMENT
    for s in DEMOTE:
        assert getattr(lib, s)(null, none, zero, i0, none, zero, None) == _lib.RC_INVALID_ARGUMENT
    for s in PROMOTE:
        assert getattr(lib, s)(null, none, zero, i0, none, zero) == _lib.RC_INVALID_ARGUMENT


def test_reserved_f32_names_are_exported_and_refuse():
    """Every _f64 entry point of the header has an _f32 one (tests/test_abi_cpu.py); for these three stems it is declared, exported and refused."""
    declared = set(_lib.declared_symbols())
    lib = _lib.lib()
    null, none, zero, i0 = ctypes.c_void_p(None), _lib.mat(None), ctypes.c_int64(0), ctypes.c_int32(0)
    for s in ("rc_lowrank_apply_mixed_batched_f32", "rc_block_operator_apply_mixed_f32", "rc_demote_batched_f32"):
        assert s in declared and hasattr(lib, s), s
    assert lib.rc_lowrank_apply_mixed_batched_f32(null, none, zero, none, zero, None, zero, none, zero, None, i0, none, zero, none, zero) == _lib.RC_INVALID_ARGUMENT
    assert lib.rc_block_operator_apply_mixed_f32(null, none, zero, none, zero, None, zero, none, zero, None, i0, none, zero, i0, None, None, i0, None, None, none,
                                                 none, i0, i0) == _lib.RC_INVALID_ARGUMENT
    assert lib.rc_demote_batched_f32(null, none, zero, i0, none, zero, None) == _lib.RC_INVALID_ARGUMENT


def test_python_names_exist():
    for name in ("lowrank_apply_batched_mixed", "block_operator_apply_mixed", "demote_batched", "promote_batched", "MixedBlockLowRankOperator"):
        assert callable(getattr(rc, name)), name
        assert name in rc.__all__, name
    assert issubclass(rc.MixedBlockLowRankOperator, rc.Operator)
    for method in ("matmat", "conj_matmat", "matmat_raw", "conj_matmat_raw"):
        assert callable(getattr(rc.MixedBlockLowRankOperator, method)), method


def test_cpp_mirror_reaches_the_mixed_calls(tmp_path):
    exe = build_cpp_mirror_examples(tmp_path, "batched_apply_mixed_example.cpp")
    assert os.path.exists(exe)
