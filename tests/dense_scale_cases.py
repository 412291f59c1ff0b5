"""Far-from-unit input scales for the dense single-factorization calls (rc_pivoted_qr_*, rc_pivoted_lq_*, rc_geqp3_*, rc_compute_svd_*,
rc_max_col_norm_*, rc_rel_diff_fro_*): the cases and the checkers, shared by tests/test_dense_scale_cases_cpu.py (the oracle passes them
at every scale, a model of unscaled norms does not) and tests/test_gpu_dense_scales.py (the device).  Host only.

The exponents, scale / descale, same_bits and in_normal_range are tests/scale_cases.py's.  A case is a unit-scale matrix `a` and an
exponent e; the call under test sees scale(a, e), which is exact.  Every checker takes `a`, e and the outputs of the call on 2^e a,
removes the scale exactly (descale of R, L, s and of the R part of a ?geqp3 result) and hands the descaled outputs to the checker the
unit-scale test of that entry point uses, with its bounds: svd_cases.check_svd with svd_cases.BOUNDS, and the live-oracle comparisons
of tests/test_gpu_parity.py, tests/test_gpu_lapack.py and tests/test_gpu_complex.py, which stand here as functions that those tests
call too.  assert_same_as_unit then holds pivots and scale-free factors to the e = 0 cell's bytes and the scaled factors to them after
descale, for the kinds in BITWISE_KINDS: the `exact` kind's noise-level outputs may go subnormal when the lowest exponent is put back.

Shapes: the smallest that reach each route of qrcp_core and svd_core (rc_api.hip) by the *_supported predicates; the route names are
the prefixes of the profile labels the routes emit."""
import numpy as np

from oracle import ref_lapack as o
from tests import scale_cases as sc
from tests import svd_cases
from tests.helpers import TOL, agreed_pivot_prefix, is_permutation, rel, stable_prefix

KINDS = sc.KINDS
BITWISE_KINDS = ("gaussian", "decay1e-3")
REAL = [np.float64, np.float32]
COMPLEX = [np.complex128, np.complex64]

# route -> (shape, k, {option name of rusty_compression_amd._lib: value}, prefix of the op: label the route must emit)
QR_ROUTES = {
    "per-step": ((60, 40), 40, {}, "op:geqp3 "),
    "per-step-truncated": ((60, 40), 20, {}, "op:geqp3 "),
    "tall": ((1024, 33), 33, {}, "op:qrcp_tall_fast "),
    "wide-coop": ((24, 256), 24, {}, "op:geqp3_wide_coop "),
    "wide-lazy": ((24, 256), 24, {"RC_OPT_WIDE_COOP_QRCP": 0}, "op:geqp3_wide_lazy "),
    "blocked-coop-panel": ((160, 144), 40, {}, "op:geqp3_blocked "),
    "blocked-step-kernels": ((160, 144), 40, {"RC_OPT_COOP_PANEL": 0}, "op:geqp3_blocked "),
}
# pivoted LQ of a is the pivoted QR of a^T: the per-step and the tall route through the transpose
LQ_ROUTES = {"per-step": ((40, 60), 40, {}, "op:geqp3 "), "tall": ((33, 1024), 33, {}, "op:qrcp_tall_fast ")}
GEQP3_ROUTES = {"per-step": QR_ROUTES["per-step"], "wide-coop": QR_ROUTES["wide-coop"], "blocked-coop-panel": QR_ROUTES["blocked-coop-panel"]}
COMPLEX_QR_SHAPES = [(60, 40), (1024, 33), (24, 256), (30, 60)]
COMPLEX_LABEL = "op:geqp3<complex> "


def svd_routes(dtype):
    """route -> (shape, label prefixes the unit cell must show)."""
    dtype = np.dtype(dtype)
    if sc.is_complex(dtype):
        return {"%dx%d" % s: (s, ("op:jacobi_svd<complex> ",)) for s in COMPLEX_QR_SHAPES}
    g = 150 if dtype == np.dtype(np.float64) else 200
    return {
        "lds-fused+householder": ((60, 30), ("op:jacobi_svd n=30", "info:jacobi_sweeps n=30", "op:geqp3 ")),
        "lds-fused+householder-transposed": ((30, 60), ("op:jacobi_svd n=30", "info:jacobi_sweeps n=30", "op:geqp3 ")),
        "lds-fused+cholqr2": ((1024, 33), ("op:jacobi_svd n=33", "info:jacobi_sweeps n=33", "op:cholqr2 ")),
        "lds-replay": ((140, 140), ("op:jacobi_svd n=140", "info:jacobi_sweeps n=140")),
        "global": ((g, g), ("op:jacobi_svd n=%d" % g,)),
    }


_CASES = {}


def cases(shape, dtype):
    """(units, cells): the three unit-scale matrices of scale_cases.kinds and the (kind index, e) of the 21 cells, the unit cell of
    each kind first (made once per shape and dtype, never changed)."""
    key = (tuple(shape), np.dtype(dtype))
    if key not in _CASES:
        units = sc.kinds(shape, dtype, 9000 + 1000 * shape[0] + shape[1] + (3 if sc.is_complex(dtype) else 0))
        for u in units:
            u.setflags(write=False)
        es = sorted(sc.exponents(dtype), key=lambda e: (e != 0, e))
        _CASES[key] = (units, [(i, e) for i in range(len(KINDS)) for e in es])
    return _CASES[key]


_ORACLE = {}


def oracle(name, a, fn):
    """fn(a), computed once per (name, matrix) and shared: the oracle's factorization of a unit-scale matrix."""
    key = (name, id(a))
    if key not in _ORACLE:
        _ORACLE[key] = (a, fn(a))  # (a is kept alive, so its id stays its own)
    return _ORACLE[key][1]


def where(err):
    """One line for a failed cell: the assertion's message, or (the checkers here are not rewritten by pytest) the line that raised."""
    import traceback

    last = traceback.extract_tb(err.__traceback__)[-1]
    msg = str(err).splitlines()[0][:200] if str(err) else ""
    return "%s:%d %s %s" % (last.filename.rsplit("/", 1)[-1], last.lineno, (last.line or "")[:120], msg)


def perturbed(a):
    """a (1 + 1e-3 g), g Gaussian: the first operand of rc_rel_diff_fro_* against a (computed once per matrix)."""
    def make(x):
        g = np.random.default_rng(x.shape[0] + x.shape[1]).standard_normal(x.shape)
        return (x * (1 + 1e-3 * g)).astype(x.dtype)
    return oracle("perturbed", a, make)


def wide_of(dtype):
    return np.complex128 if sc.is_complex(dtype) else np.float64


# ------------------------------------------------------------------------------------------------ unit-scale checkers, shared with
# the tests of the entry points (tests/test_gpu_parity.py, tests/test_gpu_lapack.py, tests/test_gpu_complex.py call them)
def check_pivoted_qr_real(a, gq, gr, gi, ref):
    """test_pivoted_qr_shapes_against_live_oracle: a full real pivoted QR against the oracle's (q, r, ind)."""
    dtype = a.dtype.type
    q, r, ind = ref
    tol = TOL[a.dtype]
    ns = agreed_pivot_prefix(gi, gr, ind, r, dtype)
    assert is_permutation(gi, a.shape[1])
    if dtype == np.float64:
        assert ns == stable_prefix(r, dtype)
    assert rel(gr[:ns, :ns], r[:ns, :ns]) <= tol["factor"]
    assert rel(gq @ gr, a[:, gi]) <= (1e-13 if dtype == np.float64 else 5e-6)
    assert np.abs(gq.T @ gq - np.eye(gq.shape[1])).max() <= (1e-13 if dtype == np.float64 else 1e-5)


def check_truncated_qr_real(a, gq, gr, gi, k, ref):
    """test_truncated_pivoted_qr_equals_the_leading_part_of_the_full_one: k steps against the leading part of the oracle's full QR."""
    q, r, ind = ref
    tol = TOL[a.dtype]
    assert np.array_equal(gi[:k], ind[:k]) and is_permutation(gi, a.shape[1])
    assert rel(gq, q[:, :k]) <= (1e-9 if a.dtype == np.float64 else 5e-2)
    assert rel(o.apply_permutation_matrix(gr, gi, "COLINV"), o.apply_permutation_matrix(r[:k], ind, "COLINV")) <= tol["factor"]


def check_pivoted_qr_complex(a, q, r, ind, ref, t):
    """test_complex_pivoted_qr_lq_match_zgeqp3, the QR half: t is that file's TOLC entry."""
    oq, orr, oind = ref
    k = min(a.shape)
    assert is_permutation(ind, a.shape[1])
    ns = agreed_pivot_prefix(ind[:k], r, oind[:k], orr, t["real"])
    assert ns == min(k, stable_prefix(orr, t["real"]))
    assert np.abs(q.conj().T @ q - np.eye(k)).max() <= t["orth"] * 10           # reference: 1e-6
    assert rel(q @ r, a[:, ind]) <= t["recon"] * 10
    assert np.abs(np.diag(r).imag).max() <= 1e-6 * np.abs(r[0, 0])               # ?geqp3: real diagonal
    # (rows of R in the original column order: past a numerical rank below k the two sides need not pivot alike)
    assert rel(r[:ns][:, np.argsort(ind)], orr[:ns][:, np.argsort(oind)]) <= t["factor"] * 3
    lead = min(ns, int((np.abs(np.diag(orr)) > np.abs(orr[0, 0]) * 1e-2).sum()))
    assert rel(q[:, :lead], oq[:, :lead]) <= t["factor"] * 10


def check_pivoted_lq_complex(a, l, ql, indl, ref, t):
    """test_complex_pivoted_qr_lq_match_zgeqp3, the LQ half."""
    ol, oql, oindl = ref
    k = min(a.shape)
    nl = agreed_pivot_prefix(indl[:k], l.conj().T, oindl[:k], ol.conj().T, t["real"])
    assert nl == min(k, stable_prefix(ol.conj().T, t["real"]))
    assert np.abs(ql @ ql.conj().T - np.eye(k)).max() <= t["orth"] * 10
    assert rel(l @ ql, a[indl, :]) <= t["recon"] * 10
    assert rel(l[np.argsort(indl)][:, :nl], ol[np.argsort(oindl)][:, :nl]) <= t["factor"] * 3  # (columns of L in the original row order)


def check_geqp3(a, f, jp, tau, q, ref, factor, recon, real):
    """test_geqp3_and_orgqr_match_lapack_output_format: the ?geqp3-format result f, jp, tau and q = ?orgqr(f, tau) against the oracle's
    raw (f, jpvt, tau); factor, recon, real: that file's FACTOR, RECON and REAL entries of a's type."""
    fo, jpo, tauo = ref
    m, n = a.shape
    k = min(m, n)
    assert is_permutation(jp, n) and tau.shape == (k,)
    r, ro = np.triu(f[:k]), np.triu(fo[:k])
    ns = agreed_pivot_prefix(jp, r, jpo, ro, real)
    assert ns >= min(k, 3), f"only {ns} pivots agree"
    # R, the reflectors and tau, entry for entry, on the columns both sides factored in the same order
    assert rel(r[:ns, :ns], ro[:ns, :ns]) <= factor
    assert rel(np.abs(np.diag(r))[:ns], np.abs(np.diag(ro))[:ns]) <= factor
    assert rel(np.tril(f[:, :ns], -1), np.tril(fo[:, :ns], -1)) <= 50 * factor   # v = x / (alpha - beta): one division more than R
    assert rel(tau[:ns], tauo[:ns]) <= 50 * factor
    # the factorization itself: A[:, jpvt] = Q R with Q from OUR reflectors through OUR ?orgqr
    assert q.shape == (m, k)
    wide = wide_of(a.dtype)
    assert rel(q.astype(wide) @ r.astype(wide), a[:, jp]) <= recon
    assert rel(q.conj().T.astype(wide) @ q.astype(wide), np.eye(k)) <= recon


def check_complex_svd(a, u, s, vt, so, t):
    """test_complex_svd_matches_zgesdd_and_reference_properties, the factor half: so is ?gesdd's s, t that file's TOLC entry."""
    r = min(a.shape)
    assert s.dtype == t["real"] and np.all(s[:-1] >= s[1:])
    assert np.abs(s - so).max() <= t["sval"] * so[0]
    assert rel((u * s) @ vt, a) <= t["recon"] * 10
    lead = int((so > so[0] * (1e-6 if a.dtype == np.complex128 else 1e-2)).sum())
    assert np.abs(u[:, :lead].conj().T @ u[:, :lead] - np.eye(lead)).max() <= t["orth"] * 10
    assert np.abs(vt[:lead] @ vt[:lead].conj().T - np.eye(lead)).max() <= t["orth"] * 10
    assert r == s.shape[0]


# the tables of tests/test_gpu_complex.py (TOLC) and tests/test_gpu_lapack.py (FACTOR, RECON, REAL), which import them from here
TOLC = {np.dtype(np.complex128): dict(factor=1e-10, sval=1e-12, orth=1e-12, recon=1e-12, real=np.float64),
        np.dtype(np.complex64): dict(factor=1e-4, sval=1e-5, orth=2e-5, recon=2e-5, real=np.float32)}
FACTOR = {np.dtype(np.float64): 1e-10, np.dtype(np.complex128): 1e-10, np.dtype(np.float32): 1e-4, np.dtype(np.complex64): 1e-4}
# A[:, jpvt] = Q R and Q^H Q = I of our own factors (backward error; the c32 Householder chain accumulates ~k eps over k steps)
RECON = {np.dtype(np.float64): 1e-12, np.dtype(np.complex128): 1e-12, np.dtype(np.float32): 1e-5, np.dtype(np.complex64): 1e-4}
REAL_OF = {np.dtype(np.float64): np.float64, np.dtype(np.complex128): np.float64, np.dtype(np.float32): np.float32, np.dtype(np.complex64): np.float32}


# ------------------------------------------------------------------------------------------------ the checkers at scale
def check_qr(a, e, q, r, ind, k):
    """rc_pivoted_qr_* on 2^e a with k = q.shape[1] steps."""
    assert np.all(np.isfinite(q)) and np.all(np.isfinite(r))
    r1 = sc.descale(r, e)
    ref = oracle("qr", a, o.pivoted_qr)
    if sc.is_complex(a.dtype):
        check_pivoted_qr_complex(a, q, r1, ind, ref, TOLC[a.dtype])
    elif k == min(a.shape):
        check_pivoted_qr_real(a, q, r1, ind, ref)
    else:  # (the steps past the numerical rank of the `exact` kind factor noise: the leading ones are what the data decides)
        ke = min(k, stable_prefix(ref[1], a.dtype))
        check_truncated_qr_real(a, q[:, :ke], r1[:ke], ind, ke, ref)


def check_lq(a, e, l, q, ind):
    """rc_pivoted_lq_* on 2^e a: the real call is the pivoted QR of a^T (rc_api.hip), so its checker is the QR's on the transposes."""
    assert np.all(np.isfinite(q)) and np.all(np.isfinite(l))
    l1 = sc.descale(l, e)
    if sc.is_complex(a.dtype):
        check_pivoted_lq_complex(a, l1, q, ind, oracle("lq", a, o.pivoted_lq), TOLC[a.dtype])
    else:
        at = oracle("t", a, lambda x: np.ascontiguousarray(x.T))
        check_pivoted_qr_real(at, q.T, l1.T, ind, oracle("qr", at, o.pivoted_qr))


def descale_geqp3(f, e, k):
    """A ?geqp3-format result with 2^-e on R (and on the trailing block of a truncated call): the reflectors below the diagonal of
    the first k columns carry no scale."""
    refl = np.tril(np.ones(f.shape, dtype=bool), -1)
    refl[:, k:] = False
    return np.where(refl, f, sc.descale(f, e))


def check_geqp3_at(a, e, f, jp, tau, q):
    assert np.all(np.isfinite(f)) and np.all(np.isfinite(tau)) and np.all(np.isfinite(q))
    dt = a.dtype
    check_geqp3(a, descale_geqp3(f, e, min(a.shape)), jp, tau, q, oracle("geqp3", a, o.geqp3_raw), FACTOR[dt], RECON[dt], REAL_OF[dt])


def check_svd(a, e, u, s, vt):
    assert np.all(np.isfinite(s))
    s1 = sc.descale(s, e)
    if sc.is_complex(a.dtype):
        check_complex_svd(a, u, s1, vt, oracle("svd", a, lambda x: o.compute_svd(x)[1]), TOLC[a.dtype])
    else:
        svd_cases.check_svd(a, u, s1, vt, a.dtype)


def assert_same_as_unit(names, unit, got):
    """Every named output of a cell (scaled factors already descaled) against the unit cell's, bit for bit."""
    for name, u, g in zip(names, unit, got):
        assert sc.same_bits(u, g), (name, float(np.max(np.abs(np.asarray(u, dtype=np.complex128) - np.asarray(g, dtype=np.complex128)))))


# ------------------------------------------------------------------------------------------------ the planted model
def unscaled_norm_qr(x):
    """The per-step pivoted Householder QR as the kernels ran it before the normalisation, in x's own precision: the column norms of
    the pivot search and the ?larfg norm are plain sums of squares in the working type, and ?larfg branches on xnorm == 0.  Returns
    (r, ind) with r the min(m, n) x n upper trapezoid in pivoted column order."""
    dt = x.dtype
    w = np.array(x, copy=True)
    m, n = w.shape
    kk = min(m, n)
    ind = np.arange(n)
    with np.errstate(all="ignore"):
        for j in range(kk):
            vn = np.sqrt(np.sum(w[j:, j:] * w[j:, j:], axis=0, dtype=dt))
            p = j + int(np.argmax(np.where(np.isnan(vn), dt.type(-1), vn)))
            if p != j:
                w[:, [j, p]] = w[:, [p, j]]
                ind[[j, p]] = ind[[p, j]]
            alpha = w[j, j]
            xnorm = np.sqrt(np.sum(w[j + 1:, j] * w[j + 1:, j], dtype=dt))
            if xnorm == 0:
                continue
            beta = -np.copysign(np.sqrt(alpha * alpha + xnorm * xnorm), alpha)
            v = np.concatenate([[dt.type(1)], w[j + 1:, j] * (dt.type(1) / (alpha - beta))]).astype(dt)
            tau = (beta - alpha) / beta
            w[j:, j + 1:] -= np.outer(v, tau * (v @ w[j:, j + 1:]))
            w[j, j] = beta
            w[j + 1:, j] = 0
    return w[:kk], ind
