"""Edge cases of the complex instantiations (c32 / c64) and the general GEMM contract of all four scalar types.

The complex paths run kernels of their own (rc_complex.hip: the Householder chain, the one-sided Jacobi SVD, the 4M product) and
tests/test_gpu_complex.py reaches them only at 100 x 50 / 50 x 100.  Here every check is against a plain high-precision reference
(numpy in complex128 / float64, or the SciPy-LAPACK oracle: zgeqp3 / zungqr / zgesdd / ztrtrs) at the shapes and inputs where
such kernels go wrong: both branches of the complex SVD (direct Jacobi and QR first) with odd cores, exactly zero and clustered
singular values, degenerate shapes and exact pivot ties, tall inputs past the 1 024-thread stride loops, strided input views, and
every op / alpha / beta / C layout of rc_gemm_*.  Tolerances: TOLC (tests/test_gpu_complex.py) and TOL (tests/helpers.py).
"""
import ctypes

import numpy as np
import pytest
import torch

import rusty_compression_amd as rc
from oracle import ref_lapack as o
from rusty_compression_amd import _lib, batch
from tests.gemm_cases import dev as _dev, gemm as _gemm, tdt as _tdt, view as _view
from tests.helpers import agreed_pivot_prefix, is_permutation, npy, rel, stable_prefix
from tests.test_gpu_complex import TOLC

pytestmark = pytest.mark.gpu
CT = rc.CompressionType
CDT = [np.complex128, np.complex64]


def _mat(dtype, shape, smin, seed):
    return o.random_approximate_low_rank_matrix(shape, 1.0, smin, np.random.default_rng(seed), dtype)


def _orth_cols(u):
    u = np.asarray(u).astype(np.complex128)
    return float(np.abs(u.conj().T @ u - np.eye(u.shape[1])).max()) if u.shape[1] else 0.0


# ------------------------------------------------------------------------------------------------ GEMM
def _op(x, op):
    return x if op == 0 else (x.T if op == 1 else x.conj().T)


def _gemm_case(dtype, opa, opb, m, k, n, alpha, beta, ckind, rng, tol):
    cplx = np.dtype(dtype).kind == "c"
    a = o.random_gaussian((m, k) if opa == 0 else (k, m), rng, dtype)
    b = o.random_gaussian((k, n) if opb == 0 else (n, k), rng, dtype)
    wide = np.complex128 if cplx else np.float64
    prod = _op(a.astype(wide), opa) @ _op(b.astype(wide), opb)
    if beta == 0:
        c0 = np.full((m, n), np.nan, dtype=dtype)          # beta = 0 must not read C
        want = alpha * prod
    else:
        c0 = o.random_gaussian((m, n), rng, dtype)
        want = alpha * prod + beta * c0.astype(wide)
    cv, buf = _view(c0, ckind, fill=complex(np.nan, np.nan) if beta == 0 else None)
    border = None if ckind != "P" else buf.clone()
    _gemm(opa, opb, alpha, _dev(a), _dev(b), beta, cv)
    got = npy(cv)
    case = (np.dtype(dtype).name, opa, opb, m, k, n, alpha, beta, ckind)
    assert np.all(np.isfinite(got)), case
    assert rel(got, want) <= tol, (case, rel(got, want))
    if border is not None:      # nothing outside the view was written
        inner = torch.zeros_like(buf, dtype=torch.bool)
        inner[1:n + 1, 2:m + 2] = True
        same = (buf == border) | (torch.isnan(buf) & torch.isnan(border))
        assert bool(torch.all(same | inner)), case


def _ab_pairs(dtype):
    if np.dtype(dtype).kind == "c":
        return [(1.0, 0.0), (-1.0, 1.0), (complex(0.3, -0.7), complex(1.1, 0.2))]
    return [(1.0, 0.0), (-1.0, 1.0), (0.3, 1.1)]


def _ops(dtype):
    return [(x, y) for x in range(3) for y in range(3)] if np.dtype(dtype).kind == "c" else [(x, y) for x in range(2) for y in range(2)]


@pytest.mark.parametrize("dtype", [np.complex128, np.complex64, np.float64, np.float32])
def test_gemm_every_op_alpha_beta_and_c_layout(dtype):
    """rc_gemm_*: every op pair (complex: none / transpose / conjugate transpose; real: trans flags), alpha / beta in
    {(1, 0), (-1, 1), general}, beta = 0 over a C full of NaN, and C as a row-major, transposed and padded odd-ld view."""
    rng = np.random.default_rng(11)
    tol = 1e-13 if np.dtype(dtype) in (np.dtype(np.complex128), np.dtype(np.float64)) else 3e-6
    for opa, opb in _ops(dtype):
        for alpha, beta in _ab_pairs(dtype):
            for ckind in ("C", "T", "P"):
                for (m, k, n) in ((1, 1, 1), (37, 29, 41)):
                    _gemm_case(dtype, opa, opb, m, k, n, alpha, beta, ckind, rng, tol)
        # ragged and (f64) transposed-problem shapes: N <= 144 under M > 144 runs as C^T = B^T A^T
        for (m, k, n) in ((513, 129, 257), (300, 64, 100)):
            alpha, beta = _ab_pairs(dtype)[2]
            _gemm_case(dtype, opa, opb, m, k, n, alpha, beta, "P" if (opa + opb) % 2 else "T", rng, tol)
            _gemm_case(dtype, opa, opb, m, k, n, 1.0, 0.0, "C", rng, tol)


@pytest.mark.parametrize("dtype", [np.complex128, np.complex64, np.float64, np.float32])
def test_gemm_deep_k_applies_beta_exactly_once(dtype):
    """512 x 8192 x 69: the product splits K (the complex 4M product accumulates four real GEMMs with beta = 1); beta C must enter
    the result exactly once.  C is large against A B, so a beta applied twice or dropped cannot hide in the rounding."""
    rng = np.random.default_rng(12)
    cplx = np.dtype(dtype).kind == "c"
    wide = np.complex128 if cplx else np.float64
    tol = 1e-13 if np.dtype(dtype) in (np.dtype(np.complex128), np.dtype(np.float64)) else 2e-5
    m, k, n = 512, 8192, 69
    for opa, opb in ((0, 0), (1, 0), (2, 2) if cplx else (1, 1)):
        a = o.random_gaussian((m, k) if opa == 0 else (k, m), rng, dtype)
        b = o.random_gaussian((k, n) if opb == 0 else (n, k), rng, dtype)
        prod = _op(a.astype(wide), opa) @ _op(b.astype(wide), opb)
        alpha, beta = _ab_pairs(dtype)[2]
        c0 = (100.0 * o.random_gaussian((m, n), rng, dtype)).astype(dtype)
        for ckind in ("C", "T"):
            cv, _ = _view(c0, ckind)
            _gemm(opa, opb, alpha, _dev(a), _dev(b), beta, cv)
            got = npy(cv).astype(wide)
            want = alpha * prod + beta * c0.astype(wide)
            assert rel(got, want) <= tol, (opa, opb, ckind, rel(got, want))
            # the part that is beta C alone: subtracting alpha A B leaves beta C to rounding, not beta^2 C or 0
            assert rel(got - alpha * prod, beta * c0.astype(wide)) <= 50 * tol, (opa, opb, ckind)


@pytest.mark.parametrize("dtype", [np.complex128, np.complex64, np.float64, np.float32])
def test_gemm_empty_inner_dimension_is_beta_c(dtype):
    """K = 0: C <- beta C as BLAS does (both paths), C <- 0 for beta = 0 even over NaN, C unchanged for beta = 1."""
    rng = np.random.default_rng(13)
    dt = _tdt(dtype)
    m, n = 7, 5
    for alpha, beta in _ab_pairs(dtype) + [(complex(2.0, 1.0) if np.dtype(dtype).kind == "c" else 2.0, 0.0)]:
        for ckind in ("C", "T", "P"):
            c0 = o.random_gaussian((m, n), rng, dtype)
            if beta == 0:
                c0[:] = np.nan
            cv, _ = _view(c0, ckind)
            a = torch.empty((m, 0), dtype=dt, device="cuda")
            b = torch.empty((0, n), dtype=dt, device="cuda")
            _gemm(0, 0, alpha, a, b, beta, cv)
            want = np.zeros((m, n)) if beta == 0 else beta * c0.astype(np.complex128)
            got = npy(cv)
            assert np.all(np.isfinite(got)) and rel(got, want) <= 1e-6 * (beta != 0), (alpha, beta, ckind)
            if beta == 1:
                assert np.array_equal(got, c0)


# ------------------------------------------------------------------------------------------------ SVD: both branches, odd cores
SVD_SHAPES = [(64, 64), (65, 65), (100, 70), (70, 100), (33, 17), (17, 33), (1, 1), (1, 7), (7, 1), (2, 2),   # direct Jacobi
              (101, 37), (37, 101), (300, 45)]                                                                # QR first, odd r


@pytest.mark.parametrize("dtype", CDT)
@pytest.mark.parametrize("shape", SVD_SHAPES)
def test_complex_svd_both_branches_and_odd_cores_match_zgesdd(dtype, shape):
    t = TOLC[np.dtype(dtype)]
    a = _mat(dtype, shape, 1e-10 if dtype == np.complex128 else 1e-4, 400 + 7 * shape[0] + shape[1])
    svd = rc.SVD.compute_from(a)
    u, s, vt = npy(svd.u), npy(svd.s), npy(svd.vt)
    so = o.compute_svd(a)[1]
    r = min(shape)
    assert u.shape == (shape[0], r) and vt.shape == (r, shape[1]) and s.dtype == t["real"]
    assert np.all(s[:-1] >= s[1:])
    assert np.abs(s - so).max() <= t["sval"] * so[0], np.abs(s - so).max() / so[0]
    assert rel((u * s) @ vt, a) <= t["recon"] * 10
    lead = int((so > so[0] * (1e-6 if dtype == np.complex128 else 1e-2)).sum())
    assert _orth_cols(u[:, :lead]) <= t["orth"] * 10
    assert _orth_cols(vt[:lead].conj().T) <= t["orth"] * 10


@pytest.mark.parametrize("dtype", CDT)
def test_complex_fused_rsvd_id_with_odd_k(dtype):
    """rc_rsvd_id_c* at k = 25, p = 6 (odd Jacobi core) against the separate complex calls and the oracle."""
    t = TOLC[np.dtype(dtype)]
    rng = np.random.default_rng(31)
    m, n, k, p = 300, 190, 25, 6
    an = o.random_approximate_low_rank_matrix((m, n), 1.0, 1e-8 if dtype == np.complex128 else 1e-4, rng, dtype)
    omn = o.random_gaussian((n, k + p), rng, dtype)
    a, om = _dev(an), _dev(omn)
    out, bufs = _rsvd_id(a, k, p, om)
    q1 = rc.sample_range_by_rank(a, k, p, om)
    svd1 = rc.SVD.compute_from_range_estimate(q1, a)
    qr1 = rc.QR.compute_from_range_estimate(q1, a)
    cid1 = qr1.column_id()
    oq = o.sample_range_by_rank(an, k, p, lambda s: omn)
    osvd = o.SVD.compute_from_range_estimate(oq, an)
    oqr = o.QR.compute_from_range_estimate(oq, an)
    rq, u, sv, vt, qq, qr_, ind, c_, z_ = (npy(x) for x in bufs)
    assert rel(rq, npy(q1)) <= t["factor"] and rel(rq, oq) <= t["factor"] * 10
    assert np.abs(sv - npy(svd1.s)).max() <= t["sval"] * 10 * sv[0]
    assert np.abs(sv - osvd.s).max() <= t["sval"] * 10 * osvd.s[0]
    assert rel((u * sv) @ vt, osvd.to_mat()) <= t["factor"] * 10
    assert _orth_cols(u) <= t["orth"] * 10 and _orth_cols(vt.conj().T) <= t["orth"] * 10
    ns = min(k, stable_prefix(oqr.r, t["real"]))
    assert np.array_equal(ind[:ns], oqr.ind[:ns]) and np.array_equal(ind[:k], npy(qr1.ind)[:k])
    assert rel(o.apply_permutation_matrix(qq @ qr_, ind, "COLINV"), oqr.to_mat()) <= t["factor"] * 10
    assert rel(c_ @ z_, npy(cid1.c) @ npy(cid1.z)) <= t["factor"] * 100
    ocid = oqr.column_id()
    assert rel(c_, ocid.c) <= t["factor"] * 10 and rel(c_ @ z_, ocid.c @ ocid.z) <= t["factor"] * 100


def _rsvd_id(a, k, p, om, ids=True):
    """rc_rsvd_id_c* into fresh buffers; ids=False leaves the QR / ID members null (skipped)."""
    m, n = a.shape
    rdt = _lib.real_dtype(a.dtype)
    e = lambda r, c: torch.empty((r, c), dtype=a.dtype, device="cuda")
    rq, u, vt, qq, qr_, c_, z_ = e(m, k), e(m, k), e(k, n), e(m, k), e(k, n), e(m, k), e(k, n)
    sv = torch.empty(k, dtype=rdt, device="cuda")
    ind = torch.empty(n, dtype=torch.int64, device="cuda")
    idm = (lambda x: _lib.mat(x)) if ids else (lambda x: _lib.mat(None))
    out = _lib.rc_rsvd_id_out(_lib.mat(rq), _lib.mat(u), ctypes.c_void_p(sv.data_ptr()), _lib.mat(vt), idm(qq), idm(qr_),
                              ctypes.c_void_p(ind.data_ptr() if ids else None), idm(c_), idm(z_))
    _lib.default_context().call(f"rc_rsvd_id_{_lib.suffix(a.dtype)}", _lib.mat(a), ctypes.c_int64(k), ctypes.c_int64(p), _lib.mat(om),
                                ctypes.c_uint64(0), ctypes.byref(out))
    torch.cuda.synchronize()
    return out, (rq, u, sv, vt, qq, qr_, ind, c_, z_)


# ------------------------------------------------------------------------------------------------ exactly zero singular values
@pytest.mark.parametrize("dtype", CDT)
@pytest.mark.parametrize("shape", [(50, 30), (128, 128), (100, 30), (30, 100), (8, 8), (1, 1)])
def test_complex_svd_with_exactly_zero_singular_values_keeps_u_orthonormal(dtype, shape):
    """Complex twin of test_svd_with_exactly_zero_singular_values_keeps_u_orthonormal: ?gesdd returns orthonormal U and V^H for
    rank-deficient input; the Jacobi core must complete the left vectors of zero singular values (direct branch: 50 x 30,
    128 x 128, 8 x 8, 1 x 1; QR first: 100 x 30, 30 x 100).  Zero columns / rows make singular values EXACTLY zero."""
    t = TOLC[np.dtype(dtype)]
    rng = np.random.default_rng(shape[0] + 3 * shape[1])
    m, n = shape
    r = min(m, n)
    a = o.random_gaussian(shape, rng, dtype)
    a[:, n // 3:] = 0
    a[m // 2:, :] = 0
    rank = min(n // 3, m // 2)
    tol = 1e-12 if dtype == np.complex128 else 2e-5
    for x, rk in ((a, rank), (np.zeros(shape, dtype=dtype), 0)):
        svd = rc.SVD.compute_from(x)
        u, s, vt = npy(svd.u), npy(svd.s), npy(svd.vt)
        assert np.all(s[rk:] == 0) and np.all(s[:rk] > 0), s
        assert np.abs(s - o.compute_svd(x)[1]).max() <= t["sval"] * max(float(s[0]), 1e-300) * 10
        assert _orth_cols(u) <= tol, ("left vectors of zero singular values complete the basis", _orth_cols(u))
        assert _orth_cols(vt.conj().T) <= tol, _orth_cols(vt.conj().T)
        assert rel((u * s) @ vt, x) <= (1e-13 if dtype == np.complex128 else 1e-5)      # (exactly 0 for the zero matrix)
        q = npy(svd.to_qr().q)       # SVD -> QR hands U on as Q
        assert _orth_cols(q) <= tol, _orth_cols(q)


@pytest.mark.parametrize("dtype", CDT)
def test_complex_fused_rsvd_id_on_exact_rank_below_k(dtype):
    """rc_rsvd_id_c* on an A whose rank (12) is below k (20): the sketch's trailing Householder vectors are exact, B = Q^H A has
    zero rows, and the SVD of B exactly zero singular values.  U and V^H stay orthonormal; the factors still reproduce A."""
    t = TOLC[np.dtype(dtype)]
    rng = np.random.default_rng(41)
    m, n, k, p, rank = 200, 150, 20, 5, 12
    an = np.zeros((m, n), dtype=dtype)
    an[:rank] = o.random_gaussian((rank, n), rng, dtype)
    omn = o.random_gaussian((n, k + p), rng, dtype)
    _, bufs = _rsvd_id(_dev(an), k, p, _dev(omn), ids=False)
    rq, u, sv, vt = (npy(x) for x in bufs[:4])
    tol = 1e-12 if dtype == np.complex128 else 2e-5
    assert np.all(sv[rank:] == 0) and np.all(sv[:rank] > 0), sv
    assert np.abs(sv[:rank] - o.compute_svd(an)[1][:rank]).max() <= t["sval"] * 10 * sv[0]
    assert _orth_cols(u) <= tol and _orth_cols(vt.conj().T) <= tol, (_orth_cols(u), _orth_cols(vt.conj().T))
    assert rel((u * sv) @ vt, an) <= t["recon"] * 10
    assert _orth_cols(rq) <= tol


# ------------------------------------------------------------------------------------------------ clustered singular values
@pytest.mark.parametrize("shape", [(64, 64), (65, 65), (100, 50), (50, 100), (40, 300)])
def test_complex_svd_of_clustered_and_repeated_singular_values(shape):
    """Complex twin of test_svd_of_clustered_and_repeated_singular_values: (near-)equal singular values through both branches of
    the complex Jacobi SVD, c64 to 1e-12 like ?gesdd, within the 60-sweep budget (no LinalgError)."""
    m, n = shape
    r = min(m, n)
    rng = np.random.default_rng(m * 1000 + n + 7)
    qa = np.linalg.qr(o.random_gaussian((m, r), rng, np.complex128))[0]
    qb = np.linalg.qr(o.random_gaussian((n, r), rng, np.complex128))[0]
    cases = {
        "1 + 1e-9 r": (qa * (1.0 + 1e-9 * rng.standard_normal(r))) @ qb.conj().T,
        "all equal": qa @ qb.conj().T,
        "two clusters": (qa * np.where(np.arange(r) % 2 == 0, 1.0, 0.5 + 1e-12 * np.arange(r))) @ qb.conj().T,
    }
    if m == n:
        cases["I + 1e-9 E"] = np.eye(n) + 1e-9 * o.random_gaussian((n, n), rng, np.complex128)
    for name, a in cases.items():
        u, s, vt = (npy(x) for x in rc.compute_svd(a))
        so = o.compute_svd(a)[1]
        assert np.abs(s - so).max() <= 1e-12 * so[0], name
        assert _orth_cols(u) <= 1e-12, (name, _orth_cols(u))
        assert _orth_cols(vt.conj().T) <= 1e-12, (name, _orth_cols(vt.conj().T))
        assert rel((u * s) @ vt, a) <= 1e-12, name


# ------------------------------------------------------------------------------------------------ degenerate inputs and ties
DEGENERATE = [(1, 1), (1, 5), (5, 1), (2, 2), (3, 7), (7, 3)]


@pytest.mark.parametrize("dtype", CDT)
def test_complex_degenerate_shapes_zero_and_rank_one(dtype):
    """1 x 1, single rows / columns, tiny wide / tall inputs, the all-zero matrix (every reflector the identity) and rank one
    through pivoted QR / LQ, SVD and the IDs, against the oracle.  The last reflector of a wide or square input has an empty
    sub-column under a non-real alpha: ?larfg still reflects, so the diagonal of R is real."""
    t = TOLC[np.dtype(dtype)]
    tol = 1e-13 if dtype == np.complex128 else 1e-5
    rng = np.random.default_rng(3)
    for shape in DEGENERATE:
        a = o.random_gaussian(shape, rng, dtype)
        q, r, ind = (npy(x) for x in rc.pivoted_qr(a))
        oq, orr, oind = o.pivoted_qr(a)
        assert np.array_equal(ind, oind), shape
        assert rel(q, oq) <= 10 * tol and rel(r, orr) <= 10 * tol, shape
        assert np.all(np.diag(r).imag == 0), (shape, np.diag(r))
        l, ql, indl = (npy(x) for x in rc.pivoted_lq(a))
        ol, oql, oindl = o.pivoted_lq(a)
        assert np.array_equal(indl, oindl) and rel(l, ol) <= 10 * tol and rel(ql, oql) <= 10 * tol, shape
        assert rel(l @ ql, a[indl, :]) <= 10 * tol, shape
        u, s, vt = (npy(x) for x in rc.compute_svd(a))
        so = o.compute_svd(a)[1]
        assert np.abs(s - so).max() <= t["sval"] * 10 * so[0], shape
        assert rel((u * s) @ vt, a) <= 10 * tol and _orth_cols(u) <= 10 * tol and _orth_cols(vt.conj().T) <= 10 * tol, shape
        qr = rc.QR.compute_from(a)
        assert rc.rel_diff_fro(qr.column_id().to_mat(), a) <= 100 * tol, shape
        assert rc.rel_diff_fro(rc.LQ.compute_from(a).row_id().to_mat(), a) <= 100 * tol, shape
        # zero matrix: identity permutation, R = 0, Q = [I; 0]; SVD: zero values, orthonormal factors
        z = np.zeros(shape, dtype=dtype)
        q, r, ind = (npy(x) for x in rc.pivoted_qr(z))
        oq, orr, oind = o.pivoted_qr(z)
        assert ind.tolist() == list(range(shape[1])) and np.array_equal(ind, oind), shape
        assert np.all(r == 0) and np.array_equal(q, np.eye(shape[0], min(shape), dtype=dtype)) and np.array_equal(q, oq), shape
        u, s, vt = (npy(x) for x in rc.compute_svd(z))
        assert np.all(s == 0) and _orth_cols(u) <= 10 * tol and _orth_cols(vt.conj().T) <= 10 * tol, shape
    # rank one: the pivot is the column of largest norm, one non-zero singular value
    x = np.outer(o.random_gaussian((40, 1), rng, dtype), o.random_gaussian((1, 30), rng, dtype)).astype(dtype)
    q, r, ind = (npy(v) for v in rc.pivoted_qr(x))
    assert ind[0] == int(np.argmax(np.linalg.norm(x.astype(np.complex128), axis=0)))
    assert ind[0] == o.pivoted_qr(x)[2][0]
    assert rel(q @ r, x[:, ind]) <= 100 * tol
    s = npy(rc.compute_svd(x)[1])
    nx = np.linalg.norm(x.astype(np.complex128))
    assert abs(s[0] - nx) <= 100 * tol * nx and s[1] <= 1e3 * tol * s[0]


@pytest.mark.parametrize("dtype", CDT)
def test_complex_pivot_ties_take_the_first_maximum_like_izamax(dtype):
    """Duplicated columns and columns times -1 are exact ties at every step (the down-dated norms are the same bits): every
    such tie takes the first maximum, as izamax does.  Columns times i are exact copies too, but |i x|^2 sums the same squares in
    another order, so their norms tie only to rounding: the pivot is then one of the tied columns, and each direction once."""
    rng = np.random.default_rng(4)
    base = o.random_gaussian((40, 6), rng, dtype)
    tol = 1e-13 if dtype == np.complex128 else 1e-5
    a = np.concatenate([base, base, -base, np.zeros((40, 3), dtype=dtype), base[:, :2]], axis=1)
    q, r, ind = o.pivoted_qr(a)
    gq, gr, gi = (npy(x) for x in rc.pivoted_qr(a))
    assert np.array_equal(gi[:6], ind[:6]) and set(gi[:6].tolist()) == set(range(6)), (gi[:6], ind[:6])
    assert rel(gq @ gr, a[:, gi]) <= 10 * tol and is_permutation(gi, a.shape[1])
    # LQ: the same rule on rows
    _, _, gil = (npy(x) for x in rc.pivoted_lq(a.T.copy()))
    assert np.array_equal(gil[:6], o.pivoted_lq(a.T.copy())[2][:6]) and np.array_equal(gil[:6], ind[:6])
    # times i, -i, -1: the first pivot is a column of the largest direction, then one column of each direction, then noise
    b = np.concatenate([np.zeros((40, 2), dtype=dtype), base * 1j, base, -1j * base, -base], axis=1)
    j0 = int(np.argmax(np.linalg.norm(base.astype(np.complex128), axis=0)))
    _, _, oi = o.pivoted_qr(b)
    gq, gr, gi = (npy(x) for x in rc.pivoted_qr(b))
    assert (gi[0] - 2) % 6 == j0 and (oi[0] - 2) % 6 == j0 and gi[0] >= 2
    assert sorted(((gi[:6] - 2) % 6).tolist()) == list(range(6)) and np.all(gi[:6] >= 2)
    assert np.abs(np.diag(gr)[6:]).max() <= 1e3 * tol * abs(gr[0, 0])
    assert rel(gq @ gr, b[:, gi]) <= 10 * tol and np.all(np.diag(gr).imag == 0)


@pytest.mark.parametrize("dtype", CDT)
def test_complex_reflector_with_zero_subcolumn_and_complex_alpha(dtype):
    """Rows 3.. of A are zero: at step 2 the sub-column under the pivot is EXACTLY zero while alpha is not real.  ?larfg must still
    reflect (tau != 0) so that R's diagonal is real; the factors equal zgeqp3's entry by entry on the determined prefix."""
    t = TOLC[np.dtype(dtype)]
    rng = np.random.default_rng(5)
    a = o.random_gaussian((7, 5), rng, dtype)
    a[3:] = 0
    qr_, jp, tau = (npy(x) for x in rc.lapack.geqp3(a))
    oqr, ojp, otau = o.geqp3_raw(a)
    assert np.array_equal(jp, ojp)
    d = np.diag(qr_)
    assert np.all(d.imag == 0) and np.all(d[:3] != 0) and np.all(d[3:] == 0), d
    assert tau[2] != 0 and otau[2] != 0                                        # the reflection happened
    assert np.all(tau[3:] == 0)
    assert rel(tau, otau) <= t["factor"] and rel(qr_, oqr) <= t["factor"]
    assert np.all(qr_[3:, 2:] == 0)                                            # no Householder vector where the column is zero
    q = npy(rc.lapack.orgqr(qr_, tau))
    assert rel(q, o.orgqr_raw(oqr, otau)) <= t["factor"] and _orth_cols(q) <= t["orth"] * 10


# ------------------------------------------------------------------------------------------------ larger shapes, QR and the IDs
@pytest.mark.parametrize("dtype", CDT)
@pytest.mark.parametrize("shape,k", [((3000, 45), 20), ((40, 2500), 20), ((257, 257), 30)])
def test_complex_qr_and_ids_at_large_and_odd_shapes(dtype, shape, k):
    """3000 rows make the 1 024-thread stride loops of k_c_qr_pivot_reflect run three times; 2500 columns a wide pivot search;
    257 x 257 an odd square.  Pivots, R and Q against zgeqp3 / zungqr, and the column, row and two-sided IDs against the oracle's
    factors (C is formed as Q R11, so it must equal A's pivot columns to factor tolerance)."""
    t = TOLC[np.dtype(dtype)]
    f = t["factor"]
    a = _mat(dtype, shape, 1e-10 if dtype == np.complex128 else 1e-4, 500 + shape[0])
    kk = min(shape)
    q, r, ind = (npy(x) for x in rc.pivoted_qr(a))
    oq, orr, oind = o.pivoted_qr(a)
    assert is_permutation(ind, shape[1])
    ns = agreed_pivot_prefix(ind[:kk], r, oind[:kk], orr, t["real"])
    if dtype == np.complex128:
        assert ns == min(kk, stable_prefix(orr, t["real"]))
    assert ns >= k
    assert np.abs(np.diag(r).imag).max() == 0
    assert rel(o.apply_permutation_matrix(r[:ns], ind, "COLINV"), o.apply_permutation_matrix(orr[:ns], oind, "COLINV")) <= f * 3
    assert _orth_cols(q) <= t["orth"] * 10
    lead = min(ns, int((np.abs(np.diag(orr)) > np.abs(orr[0, 0]) * 1e-2).sum()))
    assert rel(q[:, :lead], oq[:, :lead]) <= f * 10
    # column ID at rank k
    cid = rc.QR.compute_from(a).compress(CT.RANK(k)).column_id()
    ocid = o.QR.compute_from(a).compress("RANK", k).column_id()
    c, z, ci = npy(cid.c), npy(cid.z), npy(cid.col_ind)
    assert np.array_equal(ci[:k], ocid.col_ind[:k])
    assert rel(c, a[:, ci[:k]]) <= f * 10 and rel(c, ocid.c) <= f * 10
    assert rel(c @ z, ocid.c @ ocid.z) <= f * 100
    # row ID at rank k
    rid = rc.LQ.compute_from(a).compress(CT.RANK(k)).row_id()
    orid = o.LQ.compute_from(a).compress("RANK", k).row_id()
    x, rr, ri = npy(rid.x), npy(rid.r), npy(rid.row_ind)
    assert np.array_equal(ri[:k], orid.row_ind[:k])
    assert rel(rr, a[ri[:k], :]) <= f * 10 and rel(rr, orid.r) <= f * 10
    assert rel(x @ rr, orid.x @ orid.r) <= f * 100
    # two-sided ID from the column ID: X (k x k rows of C) at factor tolerance, not only entry by entry
    ts, ots = cid.two_sided_id(), ocid.two_sided_id()
    assert np.array_equal(npy(ts.row_ind)[:k], ots.row_ind[:k]) and np.array_equal(npy(ts.col_ind)[:k], ots.col_ind[:k])
    assert rel(npy(ts.x), ots.x) <= f * 10
    assert rel(npy(ts.x), a[np.ix_(ots.row_ind[:k], ots.col_ind[:k])]) <= f * 10
    assert rel(npy(ts.c), ots.c) <= f * 100 and rel(npy(ts.to_mat()), ots.to_mat()) <= f * 100


# ------------------------------------------------------------------------------------------------ input layouts
@pytest.mark.parametrize("dtype", CDT)
@pytest.mark.parametrize("shape", [(37, 23), (23, 37)])
def test_complex_strided_input_views_give_the_same_bits(dtype, shape):
    """A transposed view and a padded sub-view with an odd leading dimension give the same bits as the contiguous input through
    pivoted QR / LQ, compute_svd, geqp3 and the IDs, and the input (with the buffer around it) is left untouched."""
    a = _mat(dtype, shape, 1e-6, 600 + shape[0])
    k = 9
    ref = {
        "qr": rc.pivoted_qr(_dev(a)), "lq": rc.pivoted_lq(_dev(a)), "svd": rc.compute_svd(_dev(a)),
        "cid": batch.column_id_rank(_dev(a), k),
    }
    ga = _dev(a)
    gjp = torch.empty(shape[1], dtype=torch.int64, device="cuda")
    gtau = torch.empty(min(shape), dtype=ga.dtype, device="cuda")
    _lib.default_context().call(f"rc_geqp3_{_lib.suffix(ga.dtype)}", _lib.mat(ga), ctypes.c_int64(min(shape)), _lib.i64p(gjp), ctypes.c_void_p(gtau.data_ptr()))
    for kind in ("T", "P"):
        v, buf = _view(a, kind)
        before = buf.clone()
        for name, got in (("qr", rc.pivoted_qr(v)), ("lq", rc.pivoted_lq(v)), ("svd", rc.compute_svd(v)), ("cid", batch.column_id_rank(v, k))):
            for g, w in zip(got, ref[name]):
                assert torch.equal(g, w), (kind, name)
        assert torch.equal(buf, before), kind                                    # the input is read only
        # geqp3 overwrites its (strided) input in place: the same bits land in the view, nothing outside it moves
        jp = torch.empty(shape[1], dtype=torch.int64, device="cuda")
        tau = torch.empty(min(shape), dtype=v.dtype, device="cuda")
        _lib.default_context().call(f"rc_geqp3_{_lib.suffix(v.dtype)}", _lib.mat(v), ctypes.c_int64(min(shape)), _lib.i64p(jp), ctypes.c_void_p(tau.data_ptr()))
        assert torch.equal(v, ga) and torch.equal(jp, gjp) and torch.equal(tau, gtau), kind
        if kind == "P":
            inner = torch.zeros_like(buf, dtype=torch.bool)
            inner[1:shape[1] + 1, 2:shape[0] + 2] = True
            assert bool(torch.all((buf == before) | inner))
