"""CPU checks of the batched range step at the drop-in boundary: rc_sketch_range_step_batched_f64 / _f32 are declared in
include/rusty_compression_amd.h, exported by the built library, present in the generated Rust FFI (real scalars only), reject a null
context before touching a device, the four Python names are exported, and the C++ mirror's range_step_batched /
column_id_rank_power_batched build.  Then the conditions on the host model (tests/range_step_ref.py) that guard the inputs of the GPU
tests: one round of power iteration cuts the error of the sketched ID on the slowly decaying blocks to at most 0.65 of the one-pass
error, and on the tolerance example the rank rule reaches the cap only when P is orthonormalised."""
import ctypes
import os

import numpy as np
import pytest

import rusty_compression_amd as rc
from rusty_compression_amd import _lib
from tests import range_step_ref as ref
from tests.test_abi_cpu import build_cpp_mirror_examples

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = [f"rc_sketch_range_step_batched_{s}" for s in ("f64", "f32")]
NAMES = ("sketch_range_step_batched", "sketch_power_omega_batched", "sketch_column_id_rank_power_batched", "sketch_svd_rank_power_batched")


def test_range_step_symbols_are_declared_exported_and_bound():
    declared = set(_lib.declared_symbols())
    lib = _lib.lib()
    with open(os.path.join(ROOT, "bindings", "rust", "src", "ffi.rs")) as f:
        ffi = f.read()
    for s in SYMBOLS:
        assert s in declared, s
        assert hasattr(lib, s), s
        assert f"pub fn {s}(" in ffi, s
    for s in ("c64", "c32"):  # real scalars only
        assert f"rc_sketch_range_step_batched_{s}" not in declared
        assert f"rc_sketch_range_step_batched_{s}" not in ffi
        assert not hasattr(lib, f"rc_sketch_range_step_batched_{s}")


def test_range_step_entry_points_reject_a_null_context():
    lib = _lib.lib()
    none = _lib.mat(None)
    zero = ctypes.c_int64(0)
    for s in SYMBOLS:
        assert getattr(lib, s)(ctypes.c_void_p(None), none, zero, none, zero, ctypes.c_int32(0), none, zero, none, zero, none, zero,
                               None) == _lib.RC_INVALID_ARGUMENT


def test_python_names_exist():
    for name in NAMES:
        assert callable(getattr(rc, name)), name
        assert name in rc.__all__, name


def test_cpp_mirror_reaches_the_range_step(tmp_path):
    exe = build_cpp_mirror_examples(tmp_path, "batched_range_step_example.cpp")
    assert os.path.exists(exe)


@pytest.mark.parametrize("m,n,l,k", ref.DECAY_CASES)
def test_host_model_one_round_cuts_the_error(m, n, l, k):
    a = ref.decaying(m + n, m, n)
    om = ref.gaussian(m + n + l, l, m)
    e0, r0, _ = ref.column_id(a, om, k)
    e1, r1, _ = ref.column_id_power(a, om, k)
    print(f"model {m}x{n} l={l} k={k}: best {ref.best_rank(a, k):.3f} q=0 {e0:.3f} q=1 {e1:.3f} ratio {e1 / e0:.3f}")
    assert r0 == r1 == k
    assert e1 <= 0.65 * e0


def test_host_model_rank_rule_needs_an_orthonormal_p():
    m, n, l, k = ref.TOL_CASE
    a = ref.decaying(m + n, m, n, ref.TOL_SIGMA_MIN)
    om = ref.gaussian(m + n + l, l, m)
    cap = min(k, l, n)
    e1, r1, ratios = ref.column_id_power(a, om, k, ref.TOL, 1)
    e1u, r1u, _ = ref.column_id_power(a, om, k, ref.TOL, 1, orthonormalise_p=False)
    print(f"model tolerance example: q=1 err {e1:.3f} rank {r1}; P not orthonormalised err {e1u:.3f} rank {r1u}")
    assert r1 == cap
    assert r1u < cap
    # the GPU test compares ranks with this model: no ratio of the model sits within 1e-6 (relative) of the tolerance
    assert np.min(np.abs(ratios / ref.TOL - 1.0)) > 1e-6
