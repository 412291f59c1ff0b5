"""The five small products of the tall-skinny QR chain, formed inside the kernels next to them ("The
small products folded"):  r = R2 R1 in the second k_chol_inv;  w = R2^-1 Q2 and top = Q1[:k, :] w where Q2 is formed
(k_qrcp_small_q2's epilogue, or k_small_products behind k_qrcp_small);  small = R2^-1 Vc as a role of k_rsvd_id_tails (or
k_small_products from svd_finish).  Each was a one-tile GEMM with two K slabs plus the slab reduction.

1. the launches are gone from every path;  2. with the second CholeskyQR pass forced (RC_CHOLQR_SKIP=0, a worker process) the
pairs of paths that promise equal bits still give them;  3. on inputs whose second pass is far from the identity by their data,
the factorizations are held to LAPACK.

Entry-wise distance to LAPACK in test 3.  The inputs have cond 1e4 (30 in f32), no tolerance of the project covers max |Q -
Q_lapack| and max |R - R_lapack| there, so the bound is four times what the library measured BEFORE the products were folded
(two-slab GEMMs), on the same inputs, same machine -- only the summation order of the five products changed:

    case          before: max|dQ|  max|dR|      folded: max|dQ|  max|dR|
    48_nt2        3.932e-13  3.331e-16         3.931e-13  3.331e-16
    72_k64        1.221e-13  2.784e-16         1.221e-13  2.784e-16
    133_k128      2.963e-13  3.296e-16         2.963e-13  3.469e-16
    139_full      2.310e-13  4.337e-16         2.307e-13  4.372e-16
    72_k64_f32    3.772e-07  1.192e-07         3.818e-07  1.192e-07

The pivots compared are the first k (a factorization truncated at k < n leaves the other n - k columns in its own order, before
the fold as after it; LAPACK's full factorization goes on pivoting), and column j >= k of R is held against LAPACK's column of
the same index.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import rusty_compression_amd as rc
from oracle import ref_lapack as o
from tests.helpers import ROOT, npy
from tests.small_product_cases import (QR_CASES, SVD_CASE, compute_svd_at, op_names, pivoted_qr_at, qr_case_input, qr_identities,
                                       small_products_left, svd_case_input)

pytestmark = pytest.mark.gpu

# max |Q - Q_lapack|, max |R - R_lapack| of the library before the fold (see above)
BEFORE_FOLD = {
    "48_nt2": (3.932e-13, 3.331e-16),
    "72_k64": (1.221e-13, 2.784e-16),
    "133_k128": (2.963e-13, 3.296e-16),
    "139_full": (2.310e-13, 4.337e-16),
    "72_k64_f32": (3.772e-07, 1.192e-07),
}


def _rsvd_id_names(fused):
    """The stage timers' names of one rc_rsvd_id_f64 of a 1024 x 1024 Gaussian, k = 128, p = 5, hint 4, 4 slots."""
    import ctypes

    from rusty_compression_amd import _lib

    lib = _lib.lib()
    m = n = 1024
    k, p = 128, 5
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        ctx = _lib.Context(torch.cuda.current_device(), st.cuda_stream)
        a = rc.random_gaussian((m, n), rc.Rng(31), torch.float64)
        mk = lambda r, c: torch.zeros((r, c), dtype=torch.float64, device="cuda")  # noqa: E731
        b = dict(range_q=mk(m, k), u=mk(m, k), s=torch.zeros(k, dtype=torch.float64, device="cuda"), vt=mk(k, n), qr_q=mk(m, k), qr_r=mk(k, n),
                 qr_ind=torch.zeros(n, dtype=torch.int64, device="cuda"), id_c=mk(m, k), id_z=mk(k, n))
        o_ = _lib.rc_rsvd_id_out(_lib.mat(b["range_q"]), _lib.mat(b["u"]), ctypes.c_void_p(b["s"].data_ptr()), _lib.mat(b["vt"]), _lib.mat(b["qr_q"]),
                                 _lib.mat(b["qr_r"]), ctypes.c_void_p(b["qr_ind"].data_ptr()), _lib.mat(b["id_c"]), _lib.mat(b["id_z"]))
        st.synchronize()
        ctx.set_option(_lib.RC_OPT_CONCURRENCY_HINT, 4)
        ctx.set_option(_lib.RC_OPT_KERNEL_SLOTS, 4)
        ctx.set_option(_lib.RC_OPT_FUSED_CONSUMERS, fused)
        lib.rc_profile_enable(ctx._h, 1)
        lib.rc_profile_reset(ctx._h)
        ctx.call("rc_rsvd_id_f64", _lib.mat(a), ctypes.c_int64(k), ctypes.c_int64(p), _lib.mat(None), ctypes.c_uint64(25), ctypes.byref(o_))
        names = op_names(ctx, lib)
        lib.rc_profile_enable(ctx._h, 0)
        ctx.synchronize()
        assert ctx.get_health() == 0
        ctx.close()
    return names


@pytest.mark.parametrize("fused", [1, 0])
def test_no_small_product_launch_in_rsvd_id(fused):
    """1024 x 1024, k = 128, p = 5 (the smallest shape the fused path takes): no GEMM or slab reduction with M, N, K <= 144."""
    names = _rsvd_id_names(fused)
    assert any("k_gemm_mfma" in nm for nm in names), names          # the timers did see the products that remain
    assert any("tails" in nm for nm in names) == bool(fused), names
    assert any("small_tri_product" in nm for nm in names) == (not fused), names  # (fused: a role of the tails launch)
    assert not small_products_left(names), small_products_left(names)


def test_no_small_product_launch_in_pivoted_qr():
    """rc_pivoted_qr_f64 of 1024 x 133, k = 128: Q2 on several workgroups (hint 1) and inside k_qrcp_small (hint 8, 8 slots)."""
    a = np.random.default_rng(133).standard_normal((1024, 133))
    runs = pivoted_qr_at(a, 128, [(1, 8), (8, 8)])
    for key, (_, _, _, names) in runs.items():
        assert any("k_gemm_mfma" in nm for nm in names), names
        assert not small_products_left(names), (key, small_products_left(names))


def test_non_skip_arithmetic_forced():
    """RC_CHOLQR_SKIP=0 in a fresh process (tests/small_product_folds_worker.py): fused consumers on against off and hint 1
    against hint 8, bit for bit, with every second pass factoring; then the QR identities against LAPACK."""
    env = dict(os.environ, RC_CHOLQR_SKIP="0")
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "small_product_folds_worker.py")], cwd=ROOT, env=env, capture_output=True,
                         text=True, timeout=300)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("RESULT ")]
    assert len(lines) == 1, res.stdout[-2000:]
    assert json.loads(lines[0][7:]) == [], lines[0]


@pytest.mark.parametrize("case", QR_CASES, ids=[c[0] for c in QR_CASES])
def test_non_skip_arithmetic_by_data_qr(case):
    """Graded inputs (second pass far from the identity): pivots, orthogonality, residual, triangle and signs of LAPACK; hint 1 and
    hint 8 the same bits; entry-wise distance to LAPACK at most four times what it was before the fold."""
    name, m, n, k, lo, dtype = case
    a = qr_case_input(case)
    runs = pivoted_qr_at(a, k, [(1, 8), (8, 8)])
    (q1, r1, i1, n1), (q8, r8, i8, n8) = runs[(1, 8)], runs[(8, 8)]
    assert not small_products_left(n1) and not small_products_left(n8)
    assert any("qrcp_small_q2" in nm for nm in n1) == (64 < n <= 144), n1   # Q2 spread at hint 1 ...
    assert not any("qrcp_small_q2" in nm for nm in n8), n8                   # ... and inside k_qrcp_small at hint 8
    assert np.array_equal(i1, i8)
    assert np.array_equal(r1, r8), float(np.abs(r1 - r8).max())
    assert np.array_equal(q1, q8), float(np.abs(q1 - q8).max())
    dq, dr = qr_identities(a, k, q1, r1, i1, o.pivoted_qr(a))
    print("DIST %s max|dQ| %.3e max|dR| %.3e" % (name, dq, dr))
    bq, br = BEFORE_FOLD[name]
    assert dq <= 4 * bq and dr <= 4 * br, (dq, bq, dr, br)


def test_non_skip_arithmetic_by_data_svd():
    """rc_compute_svd_f64 of the graded 1024 x 128 matrix: small = R2^-1 Uc by its own launch."""
    a = svd_case_input()
    runs = compute_svd_at(a, [(1, 8), (8, 8)])
    (u1, s1, v1, n1), (u8, s8, v8, n8) = runs[(1, 8)], runs[(8, 8)]
    for names in (n1, n8):
        assert any("small_tri_product" in nm for nm in names), names
        assert not small_products_left(names), small_products_left(names)
    assert np.array_equal(u1, u8) and np.array_equal(s1, s8) and np.array_equal(v1, v8)
    r_ = a.shape[1]
    assert np.abs(u1.T @ u1 - np.eye(r_)).max() <= 1e-12
    assert np.abs(v1 @ v1.T - np.eye(r_)).max() <= 1e-12
    assert np.all(np.diff(s1) <= 0)
    assert np.linalg.norm((u1 * s1) @ v1 - a) / np.linalg.norm(a) <= 1e-12
