"""CPU checks of the batched sketch product and the randomized SVD of wide blocks at the drop-in boundary:
rc_sketch_product_batched_f64 / _f32 are declared in include/rusty_compression_amd.h, exported by the built library, present in the Rust
binding's ffi.rs, reject a null context before touching a device, are reachable from Python (sketch_product_batched,
sketch_range_step_large_batched, sketch_svd_rank_large_batched) and through the C++ mirror.

No context exists without a device, so the entry points' own argument checks are exercised in tests/test_gpu_batched_sketch_product.py.
Here the host model of tests/range_step_ref.py is held to the conditions that make the GPU accuracy cases of
tests/test_gpu_batched_sketch_svd_large.py meaningful: at every case the model reaches rank k and a second range step lowers its error,
and at the tolerance case its rank is 22 with no singular-value ratio close to the tolerance."""
import ctypes
import os

import numpy as np
import pytest

import rusty_compression_amd as rc
from rusty_compression_amd import _lib
from tests import range_step_ref as ref
from tests import sketch_large_cases as cases
from tests.test_abi_cpu import build_cpp_mirror_examples

SYMBOLS = [f"rc_sketch_product_batched_{s}" for s in ("f64", "f32")]
# svd_power's relative error of tests/range_step_ref.py's host model after one and two range steps on the blocks and test matrices of
# tests/sketch_large_cases.py (its seeds), to 4 digits
MODEL_ERRORS = {(600, 700, 40, 32): (0.4302, 0.2991), (130, 1100, 24, 16): (0.0676, 0.0575), (700, 600, 40, 32): (0.4189, 0.3036)}


def test_sketch_product_symbols_are_declared_exported_and_bound():
    declared = set(_lib.declared_symbols())
    lib = _lib.lib()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ffi = open(os.path.join(root, "bindings", "rust", "src", "ffi.rs")).read()
    for s in SYMBOLS:
        assert s in declared, s
        assert hasattr(lib, s), s
        assert f"pub fn {s}(" in ffi, s
    for s in ("c64", "c32"):  # real scalars only; the complex twins are a change of their own
        for name in (f"rc_sketch_product_batched_{s}", f"rc_sketch_product_complex_batched_{s}"):
            assert name not in declared and name not in ffi
            assert not hasattr(lib, name)


def test_sketch_product_entry_points_reject_a_null_context():
    lib = _lib.lib()
    none = _lib.mat(None)
    zero = ctypes.c_int64(0)
    for s in SYMBOLS:
        assert getattr(lib, s)(ctypes.c_void_p(None), none, zero, none, zero, ctypes.c_int32(0), none, zero) == _lib.RC_INVALID_ARGUMENT


def test_python_names_exist():
    for name in ("sketch_product_batched", "sketch_range_step_large_batched", "sketch_svd_rank_large_batched"):
        assert callable(getattr(rc, name)), name
        assert name in rc.__all__, name


def test_cpp_mirror_reaches_the_sketch_product_and_the_large_svd(tmp_path):
    exe = build_cpp_mirror_examples(tmp_path, "batched_sketch_product_example.cpp")
    assert os.path.exists(exe)


@pytest.mark.parametrize("case", cases.CASES)
def test_host_model_reaches_rank_k_and_a_second_step_helps(case):
    m, n, l, k = case
    a, om = cases.block_and_omega(case)
    assert a.shape == (m, n) and om.shape == (l, m)
    (e1, r1), (e2, r2) = ref.svd_power(a, om, k, 0.0, 1), ref.svd_power(a, om, k, 0.0, 2)
    print(f"host model {m}x{n} l={l} k={k}: one step {e1:.4f} (rank {r1}), two steps {e2:.4f} (rank {r2}), best rank-{k} {ref.best_rank(a, k):.4f}")
    assert r1 == k and r2 == k
    assert e2 < e1
    want1, want2 = MODEL_ERRORS[case]
    assert abs(e1 - want1) < 5e-4 and abs(e2 - want2) < 5e-4  # the recorded figures, so that a change of the generators is noticed


def test_host_model_tolerance_case_has_rank_22_and_a_gap():
    m, n, l, k = cases.TOL_CASE
    a, om = cases.block_and_omega(cases.TOL_CASE, cases.TOL_SIGMA_MIN)
    err, rank = ref.svd_power(a, om, k, cases.TOL, 1)
    ratios = cases.model_singular_ratios(a, om, 1)[:k]
    gap = float(np.min(np.abs(ratios / cases.TOL - 1.0)))
    print(f"tolerance case {m}x{n} l={l} tol={cases.TOL}: model rank {rank}, error {err:.3e}, nearest s_j / s_0 is {gap:.3f} (relative) from tol")
    assert rank == cases.TOL_RANK
    assert int(np.sum(ratios >= cases.TOL)) == rank  # the ratios descend: the rule's first failure is the count of those above tol
    assert gap > 1e-3
