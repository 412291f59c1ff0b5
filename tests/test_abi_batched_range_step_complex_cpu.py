"""CPU checks of the complex batched range step at the drop-in boundary: rc_sketch_range_step_complex_batched_c64 / _c32 are declared in
include/rusty_compression_amd.h with the real call's argument list and one trailing int32_t p_conj, exported by the built library and present
in the generated Rust FFI, while rc_sketch_range_step_batched_c64 / _c32 stay absent (callers tell builds apart by the symbol); a null
context is rejected before a device is touched; the four Python names are exported and their dtype errors fire without a device; the C++
mirror's complex overloads build.  Then the conditions on the host model (tests/range_step_ref_complex.py) that guard the inputs of the
GPU tests: one round of power iteration cuts the error of the sketched ID on the slowly decaying complex blocks to at most 0.65 of the
one-pass error at the pinned seeds, the conj(P) route gives the error of orthonormalising P and conjugating afterwards, and on the
tolerance example the rank rule reaches the cap only when P is orthonormalised."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import rusty_compression_amd as rc
from rusty_compression_amd import _lib
from tests import range_step_ref_complex as ref
from tests.test_abi_cpu import build_cpp_mirror_examples

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = [f"rc_sketch_range_step_complex_batched_{s}" for s in ("c64", "c32")]
NAMES = ("sketch_range_step_batched_complex", "sketch_power_omega_batched_complex", "sketch_column_id_rank_power_batched_complex",
         "sketch_svd_rank_power_batched_complex")
ARGS = ("rc_context *ctx, rc_matrix a, int64_t a_batch_stride, rc_matrix omega, int64_t omega_batch_stride, int32_t count, rc_matrix y, "
        "int64_t y_batch_stride, rc_matrix q, int64_t q_batch_stride, rc_matrix p, int64_t p_batch_stride, int64_t *ranks")


def declaration(text, name):
    mt = re.search(r"rc_status\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
    return " ".join(mt.group(1).split()) if mt else None


def test_complex_range_step_symbols_are_declared_exported_and_bound():
    declared = set(_lib.declared_symbols())
    lib = _lib.lib()
    with open(os.path.join(ROOT, "bindings", "rust", "src", "ffi.rs")) as f:
        ffi = f.read()
    with open(os.path.join(ROOT, "include", "rusty_compression_amd.h")) as f:
        header = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    for s in SYMBOLS:
        assert s in declared, s
        assert hasattr(lib, s), s
        assert f"pub fn {s}(" in ffi, s
        # the real call's arguments, one for one, then p_conj
        assert declaration(header, s) == ARGS + ", int32_t p_conj", s
        assert re.search(r"pub fn " + s + r"\([^)]*ranks: \*mut i64, p_conj: i32\) -> rc_status;", ffi), s
    for s in ("f64", "f32"):
        assert declaration(header, f"rc_sketch_range_step_batched_{s}") == ARGS
    for s in ("c64", "c32"):  # the complex twin lives under the _complex_batched_ stem only
        assert f"rc_sketch_range_step_batched_{s}" not in declared
        assert f"rc_sketch_range_step_batched_{s}" not in ffi
        assert not hasattr(lib, f"rc_sketch_range_step_batched_{s}")


def test_complex_range_step_entry_points_reject_a_null_context():
    lib = _lib.lib()
    none = _lib.mat(None)
    zero = ctypes.c_int64(0)
    for s in SYMBOLS:
        for conj in (0, 1):
            assert getattr(lib, s)(ctypes.c_void_p(None), none, zero, none, zero, ctypes.c_int32(0), none, zero, none, zero, none, zero,
                                   None, ctypes.c_int32(conj)) == _lib.RC_INVALID_ARGUMENT


def test_python_names_exist_and_reject_real_and_mismatched_data():
    for name in NAMES:
        assert callable(getattr(rc, name)), name
        assert name in rc.__all__, name
    real = torch.zeros((2, 30, 20), dtype=torch.float64)
    with pytest.raises(TypeError):
        rc.sketch_range_step_batched_complex(real, k=4)
    with pytest.raises(TypeError):
        rc.sketch_power_omega_batched_complex(real, 4, 1)
    for its in (0, 1):
        with pytest.raises(TypeError):
            rc.sketch_column_id_rank_power_batched_complex(real, 4, power_iterations=its)
        with pytest.raises(TypeError):
            rc.sketch_svd_rank_power_batched_complex(real, 4, power_iterations=its)


def test_cpp_mirror_reaches_the_complex_range_step(tmp_path):
    exe = build_cpp_mirror_examples(tmp_path, "batched_range_step_complex_example.cpp")
    assert os.path.exists(exe)


@pytest.mark.parametrize("m,n,l,k", ref.DECAY_CASES)
def test_host_model_one_round_cuts_the_error(m, n, l, k):
    a, om = ref.case_data((m, n, l, k))
    e0, r0, _ = ref.column_id(a, om, k)
    e1, r1, _ = ref.column_id_power(a, om, k)
    e1c = ref.column_id_power(a, om, k, conj_first=False)[0]
    print(f"model {m}x{n} l={l} k={k} seed {ref.SEEDS[(m, n, l, k)]}: best {ref.best_rank(a, k):.3f} q=0 {e0:.3f} q=1 {e1:.3f} ratio {e1 / e0:.3f}; "
          f"orthonormalise then conjugate {e1c:.6f} against {e1:.6f}")
    assert r0 == r1 == k
    assert e1 <= 0.65 * e0
    # the two routes to U^H span the same rows: the errors agree far below the digits anybody prints
    assert abs(e1c - e1) <= 1e-9 * e1


def test_host_model_basis_has_orthonormal_rows_and_reproduces_the_sketch():
    m, n, l, k = ref.DECAY_CASES[2]
    a, om = ref.case_data((m, n, l, k))
    q, p = ref.range_step(a, om)
    y = om @ a
    assert np.linalg.norm(q @ q.conj().T - np.eye(l)) <= 1e-13
    assert np.linalg.norm(y - (y @ q.conj().T) @ q) <= 1e-13 * np.linalg.norm(y)
    assert np.allclose(p, a @ q.conj().T, rtol=0, atol=1e-14)
    om1 = ref.power_omega(a, om, 1)
    assert np.linalg.norm(om1 @ om1.conj().T - np.eye(l)) <= 1e-13  # U^H of an orthonormal basis U of p's columns
    assert np.linalg.norm(p - om1.conj().T @ (om1 @ p)) <= 1e-12 * np.linalg.norm(p)


def test_host_model_rank_rule_needs_an_orthonormal_p():
    m, n, l, k = ref.TOL_CASE
    a, om = ref.case_data(ref.TOL_CASE, ref.TOL_SIGMA_MIN)
    cap = min(k, l, n)
    e1, r1, ratios = ref.column_id_power(a, om, k, ref.TOL, 1)
    e1u, r1u, _ = ref.column_id_power(a, om, k, ref.TOL, 1, orthonormalise_p=False)
    print(f"model tolerance example: q=1 err {e1:.3f} rank {r1}; P not orthonormalised err {e1u:.3f} rank {r1u}")
    assert r1 == cap
    assert r1u < cap
    # the GPU test compares ranks with this model: no ratio of the model sits within 1e-6 (relative) of the tolerance
    assert np.min(np.abs(ratios / ref.TOL - 1.0)) > 1e-6
