"""Far-from-unit input scales for the one-workgroup batched IDs and SVDs: the cases and the checkers, shared by
tests/test_scale_cases_cpu.py (the oracle passes them at every scale, a model of unscaled norms does not) and
tests/test_gpu_batched_scales.py (the device).

A case is a unit-scale matrix `a` and an exponent e; the call under test sees 2^e a (np.ldexp: exact).  Every checker takes `a`, e and
the outputs of the call on 2^e a.  It first compares what is gathered from the input with the scaled input bit for bit, then removes the
scale exactly (ldexp by -e on the factors that carry it: C of a column ID, X of a two-sided ID, s of an SVD, Y and P of the sketched
calls) and hands the result to the family's existing oracle checker against `a`.  Descaling first matters: those checkers square in
f64 and would themselves overflow at 2^900.  assert_same_as_unit then holds the descaled outputs to the e = 0 entry of the same batch:
multiplying by a power of two commutes with every rounding while nothing leaves the normal range, so the answer for 2^e a is the answer
for a, bit for bit (LAPACK meets this: test_scale_cases_cpu.py).

Exponents: the outer ones keep every input, every output and ||A||_F inside the normal range at the shapes used; the middle magnitudes
sit where the squares of the entries start to overflow (2^62, 2^510) or go subnormal (2^-64, 2^-512).
Kinds: Gaussian; singular values 1 .. 1e-3 (the modest decay keeps the smallest kept singular value times 2^-90 normal in f32); an exact
rank-EXACT_RANK product, which the tolerance of the calls (TOLS) must cut at that rank."""
import numpy as np
import scipy.linalg

from oracle import ref_lapack as o
from tests import test_gpu_batched_id as bid
from tests import test_gpu_batched_id_complex as bidc
from tests import test_gpu_batched_range_step as brs
from tests import test_gpu_batched_sketch_id as bsi
from tests import test_gpu_batched_sketch_id_complex as bsic
from tests import test_gpu_batched_svd as bsv
from tests import test_gpu_batched_svd_complex as bsvc
from tests import test_gpu_batched_two_sided_id as bts
from tests import test_gpu_batched_two_sided_id_complex as btsc
from tests.helpers import is_permutation, stable_prefix

E32 = (-90, -64, -40, 0, 40, 62, 90)
E64 = (-900, -512, -300, 0, 300, 510, 900)
KINDS = ("gaussian", "decay1e-3", "exact")
EXACT_RANK = 5
# the tolerance of every call: test_tolerance_mode_exact_ranks_zero_and_full's.  The Gaussian and the 1e-3 kinds stay above it at every step.
TOLS = {np.dtype(np.float64): 1e-8, np.dtype(np.float32): 1e-4}

# (m, n, k) of the IDs: bid_apply<., 2> (<= 128 rows remaining), <., 4> (<= 256), <., 8> (> 256), and a wide one
ID_SHAPES = [(96, 40, 40), (200, 200, 128), (333, 77, 77), (77, 333, 33)]
# SVD: one core per Jacobi width (NE = 1, 2, 4, 8) and a wide matrix read through its transposed view
SVD_SHAPES = [(50, 12), (60, 30), (100, 50), (128, 128), (50, 100)]
# (m, n, l) of the sketched ID, from its file's SHAPES: the smallest entry with more than one column panel, row chunk and row tile whose
# working copy is in LDS, and the smallest one whose working copy is in the workspace (the entries below (257, 130, 40) are single-panel)
SKETCH_SHAPES = [(257, 130, 40), (700, 512, 128)]
# (m, n, l) of the range step, from its file's SHAPES: the smallest entry in LDS and the one entry out of LDS (f64; f32 keeps it in LDS)
STEP_SHAPES = [(70, 33, 17), (520, 130, 128)]


def real_of(dtype):
    return np.dtype(np.finfo(np.dtype(dtype)).dtype)


def is_complex(dtype):
    return np.dtype(dtype).kind == "c"


def exponents(dtype):
    return E64 if real_of(dtype) == np.dtype(np.float64) else E32


def scale(x, e):
    """2^e x, exactly (real and imaginary part on their own: no complex product that could overflow on the way)."""
    x = np.asarray(x)
    if not is_complex(x.dtype):
        return np.ldexp(x, e)
    out = np.empty_like(x)
    out.real = np.ldexp(x.real, e)
    out.imag = np.ldexp(x.imag, e)
    return out


def descale(x, e):
    return scale(x, -e)


def in_normal_range(x, dtype):
    """Every component of x is finite and zero or normal in the working type."""
    x = np.asarray(x)
    parts = (x.real, x.imag) if is_complex(x.dtype) else (x,)
    tiny = np.finfo(real_of(dtype)).tiny
    return all(np.all(np.isfinite(p)) and np.all((p == 0) | (np.abs(p) >= tiny)) for p in parts)


def kinds(shape, dtype, seed):
    """The three unit-scale matrices of a shape (complex ones as tests/test_gpu_batched_id_complex.py builds them)."""
    m, n = shape
    rng = np.random.default_rng(seed)
    r = min(EXACT_RANK, max(1, min(m, n) // 2))
    if is_complex(dtype):
        return [o.random_gaussian((m, n), rng, dtype), o.random_approximate_low_rank_matrix((m, n), 1.0, 1e-3, rng, dtype),
                (o.random_gaussian((m, r), rng, np.complex128) @ o.random_gaussian((r, n), rng, np.complex128)).astype(dtype)]
    return [rng.standard_normal((m, n)).astype(dtype), o.random_approximate_low_rank_matrix((m, n), 1.0, 1e-3, rng).astype(dtype),
            (rng.standard_normal((m, r)) @ rng.standard_normal((r, n))).astype(dtype)]


def exact_rank(shape):
    return min(EXACT_RANK, max(1, min(shape) // 2))


_BATCH = {}


def batch(shape, dtype):
    """(units, cells, stacked): the three unit matrices, the (kind index, e) of each of the 21 entries, and the [21, m, n] scaled stack
    (made once per shape and dtype, never changed)."""
    key = (tuple(shape), np.dtype(dtype))
    if key not in _BATCH:
        units = kinds(shape, dtype, 7000 + 1000 * shape[0] + shape[1] + (3 if is_complex(dtype) else 0))
        cells = [(i, e) for i in range(len(KINDS)) for e in exponents(dtype)]
        stacked = np.stack([scale(units[i], e) for i, e in cells])
        for arr in units + [stacked]:
            arr.setflags(write=False)
        _BATCH[key] = (units, cells, stacked)
    return _BATCH[key]


def unit_cell(cells, i):
    return cells.index((i, 0))


def omega(shape, l, dtype):
    """The unit-scale test matrix (l x m) of the sketched calls: only A carries the scale."""
    rng = np.random.default_rng(900 + shape[0] + l)
    return o.random_gaussian((l, shape[0]), rng, dtype) if is_complex(dtype) else rng.standard_normal((l, shape[0])).astype(dtype)


def same_bits(x, y):
    x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
    return x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes()  # bytes: a NaN equals itself, -0.0 is not 0.0


def assert_same_as_unit(names, unit, got, ind_prefix=None):
    """got (descaled) against the e = 0 entry of the same batch: ranks equal, `ind*` equal over ind_prefix entries (None: all), every other
    output bit for bit."""
    for name, u, g in zip(names, unit, got):
        if name == "ranks":
            assert int(u) == int(g), (name, int(u), int(g))
        elif name.endswith("ind"):
            k = len(u) if ind_prefix is None else ind_prefix
            assert np.array_equal(u[:k], g[:k]), name
        else:
            assert same_bits(u, g), (name, float(np.max(np.abs(np.asarray(u, dtype=np.complex128) - np.asarray(g, dtype=np.complex128)))))


def id_stable_prefix(a, ind, r, dtype):
    """stable_prefix of the R the pivots `ind` give on the unit matrix: the pivots that the data decides."""
    if r == 0:
        return 0
    mod = bidc if is_complex(dtype) else bid
    return stable_prefix(mod.r_of(a, ind, r), real_of(dtype))


# ------------------------------------------------------------------------------------------------ the family checkers
def check_column_id(a, e, c, z, ind, r, k, dtype, tol):
    """One entry of a column-ID batch run on 2^e a with tolerance tol."""
    r = int(r)
    assert is_permutation(ind, a.shape[1]) and 0 <= r <= k
    assert same_bits(c[:, :r], scale(a, e)[:, ind[:r]])  # gathered from the scaled input, bit for bit
    assert np.all(np.isfinite(z))
    mod = bidc if is_complex(dtype) else bid
    mod.check_one(a, descale(c, e), z, ind, r, k, dtype, oracle_tol=tol if r < k else None)


def check_two_sided_id(a, e, c, x, rr, row_ind, col_ind, r, k, dtype):
    r = int(r)
    assert is_permutation(row_ind, a.shape[0]) and is_permutation(col_ind, a.shape[1]) and 0 <= r <= k
    assert same_bits(x[:r, :r], scale(a, e)[row_ind[:r]][:, col_ind[:r]])
    assert np.all(np.isfinite(c)) and np.all(np.isfinite(rr))
    mod = btsc if is_complex(dtype) else bts
    mod.check_one(a, c, descale(x, e), rr, row_ind, col_ind, r, k, dtype)


def check_svd(a, e, u, s, vt, r, k, dtype):
    r = int(r)
    assert np.all(np.isfinite(u)) and np.all(np.isfinite(vt)) and np.all(np.isfinite(s))
    s1 = descale(s, e)
    if is_complex(dtype):
        ref = bsvc.check_one(a, u, s1, vt, r, dtype)
        bsvc.check_vectors(u, vt, ref.u, ref.vt, ref.s, r, dtype)
    else:
        ref = bsv.check_one(a, u, s1, vt, r, k, dtype)
        bsv.check_vectors(u, vt, ref.u, ref.vt, ref.s, r, dtype)


def check_sketch_id(a, om, e, c, z, ind, r, y, k, dtype):
    """One entry of a sketched-ID batch: the sketch under the dot-product bound of test_sketch_against_the_host, C gathered from the scaled
    input, Z's identity block and zero tails, and the error of C Z against the same algorithm on the host at the rank taken."""
    r = int(r)
    m, n = a.shape
    l = om.shape[0]
    kk = min(k, l, n)
    rd = real_of(dtype)
    assert is_permutation(ind, n) and 0 <= r <= kk
    assert same_bits(c[:, :r], scale(a, e)[:, ind[:r]]) and not np.any(c[:, r:]) and not np.any(z[r:])
    assert np.array_equal(z[:, ind[:r]][:r], np.eye(r, dtype=dtype))
    assert np.all(np.isfinite(z))
    y1 = descale(y, e).astype(np.complex128 if is_complex(dtype) else np.float64)
    u = np.finfo(rd).eps / 2
    cst = 1.0 if rd == np.dtype(np.float32) else 2.0
    if is_complex(dtype):
        om128, a128 = om.astype(np.complex128), a.astype(np.complex128)
        ore, oim, are, aim = np.abs(om128.real), np.abs(om128.imag), np.abs(a128.real), np.abs(a128.imag)
        y_ref = om128 @ a128
        for got, ref, absm in ((y1.real, y_ref.real, ore @ are + oim @ aim), (y1.imag, y_ref.imag, ore @ aim + oim @ are)):
            assert np.all(np.abs(got - ref) <= cst * (2 * m + 8) * u * absm)
        wide = np.complex128
        host = bsic.host_route
    else:
        om64, a64 = om.astype(np.float64), a.astype(np.float64)
        assert np.all(np.abs(y1 - om64 @ a64) <= cst * (m + 4) * u * (np.abs(om64) @ np.abs(a64)))
        wide = np.float64
        host = bsi.host_route
    if r > 0:
        aw = a.astype(wide)
        err = np.linalg.norm(aw - descale(c, e)[:, :r].astype(wide) @ z[:r].astype(wide)) / np.linalg.norm(aw)
        assert err <= 1.5 * host(a, om, r) + 100 * np.finfo(rd).eps, (err, host(a, om, r))


def check_range_step(a, om, e, q, p, r, y, dtype):
    """One entry of a range-step batch, the assertions of test_one_step_against_the_host: full rank, the basis against LAPACK's on the
    call's own (descaled) Y in the same precision, the projection against the f64 host product with the call's own Q."""
    r = int(r)
    m, n = a.shape
    l = om.shape[0]
    assert r == l
    assert np.all(np.isfinite(q))
    y1, p1 = descale(y, e), descale(p, e)
    u = np.finfo(dtype).eps / 2
    cst = 1.0 if np.dtype(dtype) == np.dtype(np.float32) else 2.0
    lq = scipy.linalg.qr(y1.T, mode="economic", pivoting=True)[0].T
    assert lq.dtype == np.dtype(dtype)
    orth, span = brs.basis_figures(y1, q, r)
    lorth, lspan = brs.basis_figures(y1, lq, r)
    floor = np.sqrt(l) * u
    assert orth <= brs.QR_MARGIN * lorth + floor, (orth, lorth)
    assert span <= brs.QR_MARGIN * lspan + floor, (span, lspan)
    a64, q64 = a.astype(np.float64), q.astype(np.float64)
    assert np.all(np.abs(p1.astype(np.float64) - a64 @ q64.T) <= cst * (n + 4) * u * (np.abs(a64) @ np.abs(q64.T)))
