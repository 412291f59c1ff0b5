"""CPU checks of the complex batched residual norms at the drop-in boundary: rc_lowrank_residual_batched_c64 / _c32 are declared in
include/rusty_compression_amd.h, exported by the built library, present in the generated Rust FFI, reject a null context before touching a
device, are reachable from Python and through the C++ mirror's residual_batched overloads; and the error bound the GPU tests hold the kernel
to (tests/residual_ref_complex.py) is not vacuous: the contract's arithmetic emulated in NumPy stays inside it, a rebuild one rank short
does not."""
import ctypes
import os

import numpy as np
import pytest

import rusty_compression_amd as rc
from oracle import ref_lapack as o
from rusty_compression_amd import _lib
from tests import residual_ref_complex as rrc
from tests.test_abi_cpu import build_cpp_mirror_examples

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = [f"rc_lowrank_residual_batched_{s}" for s in ("c64", "c32")]
NAMES = ("lowrank_residual_batched_complex", "column_id_residual_batched_complex", "two_sided_id_residual_batched_complex",
         "svd_residual_batched_complex")


def test_complex_batched_residual_symbols_are_declared_exported_and_bound():
    declared = set(_lib.declared_symbols())
    lib = _lib.lib()
    with open(os.path.join(ROOT, "bindings", "rust", "src", "ffi.rs")) as f:
        ffi = f.read()
    for s in SYMBOLS:
        assert s in declared, s
        assert hasattr(lib, s), s
        assert f"pub fn {s}(" in ffi, s


def test_complex_batched_residual_entry_points_reject_a_null_context():
    lib = _lib.lib()
    none = _lib.mat(None)
    zero = ctypes.c_int64(0)
    for s in SYMBOLS:
        assert getattr(lib, s)(ctypes.c_void_p(None), none, zero, none, zero, none, zero, None, zero, none, zero, None, ctypes.c_int32(0), none, zero,
                               None, None) == _lib.RC_INVALID_ARGUMENT


def test_python_names_exist():
    for name in NAMES:
        assert callable(getattr(rc, name)), name
        assert name in rc.__all__, name


def test_cpp_mirror_reaches_the_complex_batched_residual(tmp_path):
    exe = build_cpp_mirror_examples(tmp_path, "batched_residual_complex_example.cpp")
    assert os.path.exists(exe)


def test_chain_length():
    assert rrc.chain_length(1, 1) == 24 and rrc.chain_length(32, 64) == 24 and rrc.chain_length(33, 65) == 72
    assert rrc.chain_length(65536, 512) == 16 * 2048 * 8 + 8


@pytest.mark.parametrize("dtype", [np.complex128, np.complex64])
@pytest.mark.parametrize("mode", ["none", "mid", "s", "both"])
@pytest.mark.parametrize("m,n,K,r", [(1030, 300, 40, 40), (33, 17, 17, 5)])
def test_the_bound_holds_for_the_contract_arithmetic_and_not_one_rank_short(m, n, K, r, mode, dtype):
    """Complex blocks with the decaying spectrum of the sketch tests (a real block of that spectrum with unit-modulus row and column
    phases, which keep its singular values) and their truncated-SVD factors (mid: a unitary core folded into right).  The contract's
    arithmetic, emulated in the block's own precision, meets every bound; the same rebuild with r - 1 terms misses the elementwise bound
    and the bound on err by far: the r-th singular value is 0.05 (1030 x 300, r = 40) and 3e-3 (33 x 17, r = 5)."""
    rng = np.random.default_rng(7 * m + n)
    a = o.random_approximate_low_rank_matrix((m, n), 1.0, 1e-10, rng)
    a = np.exp(2j * np.pi * rng.uniform(size=m))[:, None] * a * np.exp(2j * np.pi * rng.uniform(size=n))[None, :]
    u, sv, vh = np.linalg.svd(a, full_matrices=False)
    q = np.linalg.qr(rng.standard_normal((K, K)) + 1j * rng.standard_normal((K, K)))[0]
    left = u[:, :K] if mode in ("s", "both") else u[:, :K] * sv[:K]
    mid = q if mode in ("mid", "both") else None
    right = q.conj().T @ vh[:K] if mid is not None else vh[:K]
    s = sv[:K] if mode in ("s", "both") else None
    if mode == "both":  # left mid diag(s) right with the core to the left of s: right takes diag(1 / s) q^H diag(s) vh
        right = (q.conj().T * (1.0 / sv[:K])[None, :]) @ (sv[:K, None] * vh[:K])
    cast = lambda x: None if x is None else x.astype(dtype)  # noqa: E731
    a, left, mid, right = cast(a), cast(left), cast(mid), cast(right)
    s = None if s is None else s.astype(rrc.real_dtype(dtype))
    L = rrc.chain_length(m, n)
    _, e_ref = rrc.reference(a, left, right, mid, s, r)
    B, err_bound, nrm_bound = rrc.bound(a, left, right, mid, s, r, dtype, L)
    err, nrm, e = rrc.emulate(a, left, right, mid, s, r)
    assert err.dtype == rrc.real_dtype(dtype) and nrm.dtype == rrc.real_dtype(dtype) and e.dtype == np.dtype(dtype)
    gap = np.abs(e.astype(np.complex128) - e_ref)
    print(f"{m}x{n} K={K} r={r} {mode} {np.dtype(dtype).name}: max |e - e_ref| / B = {np.max(gap / B):.3e}, "
          f"|err - ref| / bound = {abs(float(err) - np.linalg.norm(e_ref)) / err_bound:.3e}")
    assert np.all(gap <= B)
    assert abs(float(err) - np.linalg.norm(e_ref)) <= err_bound
    assert abs(float(nrm) - np.linalg.norm(a.astype(np.complex128))) <= nrm_bound
    short_err, _, short_e = rrc.emulate(a, left, right, mid, s, r - 1)
    assert not np.all(np.abs(short_e.astype(np.complex128) - e_ref) <= B)
    assert abs(float(short_err) - np.linalg.norm(e_ref)) > err_bound
