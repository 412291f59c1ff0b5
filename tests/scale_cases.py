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
rank-EXACT_RANK product, which the tolerance of the calls (TOLS) must cut at that rank.

The calls that consume those outputs (second half of this file): a recompression case is a unit-scale (left, right, mid, s) and a carrier
that says which operand takes 2^e (CARRIERS), a residual case a unit-scale block with its factors where `a` and one factor take 2^e
(RESIDUAL_CARRIER); check_recompress and check_residual descale exactly and hand over to the families' own checkers and bounds."""
import numpy as np
import scipy.linalg

from oracle import ref_lapack as o
from tests import test_gpu_batched_id as bid
from tests import test_gpu_batched_id_complex as bidc
from tests import residual_ref as rr
from tests import residual_ref_complex as rrc
from tests import test_gpu_batched_range_step as brs
from tests import test_gpu_batched_recompress as brc
from tests import test_gpu_batched_recompress_complex as brcc
from tests import test_gpu_batched_sketch_id as bsi
from tests import test_gpu_batched_sketch_id_complex as bsic
from tests import test_gpu_batched_svd as bsv
from tests import test_gpu_batched_svd_complex as bsvc
from tests import test_gpu_batched_two_sided_id as bts
from tests import test_gpu_batched_two_sided_id_complex as btsc
from tests.helpers import is_permutation, sign_normalise, stable_prefix

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


# ------------------------------------------------------------------------------------------------ recompression: cases and checker
# which operand of left mid diag(s) right carries 2^e, and the mode (tests/test_gpu_batched_recompress.py's MODES) it runs in:
#   left:  what a column ID's C carries;  mid: a two-sided ID's X;  s: an SVD's s;
#   split: left and mid times 2^e, s and right times 2^-e: every operand is extreme and the product is at unit scale, so a kernel that
#          normalises some operands and not others goes wrong here.
CARRIERS = {"left": "none", "mid": "mid", "s": "s", "split": "both"}
RECOMPRESS_KINDS = ("gauss", "spectrum")
# (m, n, K) per family, from the families' own lists: the smallest LDS plans and a workspace plan; two stages of the left factor; both
# factors staged
RECOMPRESS_SHAPES = {"small": [(33, 17, 17), (200, 96, 40), (512, 512, 128)], "tall": [(513, 40, 8), (1100, 130, 128)],
                     "large": [(513, 600, 8), (300, 2100, 64)]}


def recompress_kinds(carrier, dtype):
    """The kinds a dtype runs.  The spectrum kind's singular values go down to 2^-30 and, computed from factors rounded to f32, below
    (1e-11 at K = 128); its left = Q diag(2^-j) has entries down to 2^-50.  2^-90 takes both below the smallest normal f32 number, where
    a power of two no longer commutes with the rounding: f32 / c32 run the Gaussian kind alone, f64 / c64 both."""
    return ("gauss",) if real_of(dtype) == np.dtype(np.float32) else RECOMPRESS_KINDS


def carry(factors, carrier, e):
    """The unit-scale (left, right, mid, s) with the carrier's operands times 2^+-e, exactly."""
    left, right, mid, s = factors
    if carrier == "left":
        return scale(left, e), right, mid, s
    if carrier == "mid":
        return left, right, scale(mid, e), s
    if carrier == "s":
        return left, right, mid, scale(s, e)
    assert carrier == "split"
    return scale(left, e), scale(right, -e), scale(mid, e), scale(s, -e)


def net_exponent(carrier, e):
    """The exponent the product, and with it s_out, carries."""
    return 0 if carrier == "split" else e


_RECOMPRESS = {}


def recompress_batch(shape, dtype, carrier):
    """(units, cells, operands, refs): the unit factors per kind, the (kind index, e) of each entry, the four stacked operands (None where
    the mode has none) and per kind (a, sigma, oracle SVD) of the unit-scale dense product (made once, never changed)."""
    key = (tuple(shape), np.dtype(dtype), carrier)
    if key not in _RECOMPRESS:
        m, n, K = shape
        mod = brcc if is_complex(dtype) else brc
        rng = np.random.default_rng(31000 + 1000 * m + 10 * n + K + list(CARRIERS).index(carrier) + (5 if is_complex(dtype) else 0))
        kinds_ = recompress_kinds(carrier, dtype)
        units = [mod.factors(rng, kind, m, n, K, CARRIERS[carrier], dtype) for kind in kinds_]
        cells = [(i, e) for i in range(len(kinds_)) for e in exponents(dtype)]
        operands = mod.stack([carry(units[i], carrier, e) for i, e in cells])
        refs = []
        for f in units:
            a, sigma = mod.dense(*f, K)
            refs.append((a, sigma, o.SVD.compute_from(a)))
        for arr in [x for f in units for x in f] + list(operands):
            if arr is not None:
                arr.setflags(write=False)
        _RECOMPRESS[key] = (units, cells, operands, refs)
    return _RECOMPRESS[key]


def check_recompress(ref, carrier, e, u, s_out, vt, r, kk, dtype, unit_out):
    """One entry of a recompression batch run on carry(unit factors, carrier, e): s_out descaled by the net exponent, exactly, then the
    family's check_block against the unit-scale dense product (ref = (a, sigma, its oracle SVD); the bounds are that file's TOL and nothing
    new), then u, vt and the rank, and the descaled s_out, against the e = 0 entry of the same batch (unit_out = (u, s_out, vt, rank)) bit
    for bit: each operand is multiplied by an exact power of two before any rounding, so the working copies are identical."""
    mod = brcc if is_complex(dtype) else brc
    a, sigma, oracle = ref
    assert np.all(np.isfinite(u)) and np.all(np.isfinite(vt)) and np.all(np.isfinite(s_out))
    s1 = descale(s_out, net_exponent(carrier, e))
    mod.check_block(a, sigma, u, s1, vt, int(r), s_out.shape[0], kk, dtype, oracle)
    assert_same_as_unit(("u", "s", "vt", "ranks"), unit_out, (u, s1, vt, r))


def host_recompress(left, right, mid, s, dtype, plain_norms=False):
    """The recompression in the working precision on the host: every operand normalised by the exact power of two of its largest
    component (as the kernels do), scipy's pivoted QR of left and of right^T (no conjugate), the core Rl mid diag(s) Rr^T, numpy's SVD of
    it, the batched sign / phase rule, and s_out = 2^(el + em + es + er) times the core's singular values.
    plain_norms: the planted model.  The same route, but the singular values are taken as the kernels took them before mid and s (for
    complex data: any operand) were normalised: the square roots of plain sums of squares, in the working type, of the columns of the
    rotated core at the scale the operands left it with.  Returns (u, s_out, vt, r) with r = K."""
    dt = np.dtype(dtype)
    rd = real_of(dt)

    def expo(x):
        if x is None:
            return 0
        mx = float(max(np.abs(x.real).max(), np.abs(x.imag).max())) if is_complex(x.dtype) else float(np.abs(x).max())
        return int(np.floor(np.log2(mx))) if mx > 0 and np.isfinite(mx) else 0

    el, er, em, es = expo(left), expo(right), expo(mid), expo(s)
    lf, rt = scale(left, -el), scale(right, -er)
    K = lf.shape[1]
    ql, rl, pl = scipy.linalg.qr(lf, mode="economic", pivoting=True)
    qr_, rr_, pr = scipy.linalg.qr(rt.T, mode="economic", pivoting=True)
    rl_full, rr_full = np.zeros_like(rl), np.zeros_like(rr_)
    rl_full[:, pl], rr_full[:, pr] = rl, rr_
    core = np.eye(K, dtype=dt) if mid is None else scale(mid, -em)
    if s is not None:
        core = core * scale(s, -es)[None, :]
    c = rl_full @ core @ rr_full.T
    assert c.dtype == dt and ql.dtype == dt and qr_.dtype == dt
    uc, sv, vh = np.linalg.svd(c)
    if plain_norms:
        with np.errstate(all="ignore"):
            gv = scale((c @ vh.conj().T).astype(dt), el + er + em + es)
            s_out = np.sqrt(np.sum((gv * gv.conj()).real.astype(rd), axis=0, dtype=rd))
    else:
        s_out = np.ldexp(sv.astype(rd), el + er + em + es)
    u, vt = (ql @ uc).astype(dt), (vh @ qr_.T).astype(dt)
    if is_complex(dt):
        for j in range(K):
            i = int(np.argmax(np.abs(u[:, j])))
            mag = np.abs(u[i, j])
            if mag > 0 and np.isfinite(mag):
                ph = np.conj(u[i, j]) / mag
                u[:, j] *= ph
                u[i, j] = mag
                vt[j] *= np.conj(ph)
    else:
        u, vt = sign_normalise(u, vt)
    return u, s_out, vt, K


# ------------------------------------------------------------------------------------------------ residual norms: cases and checker
# mode of tests/residual_ref.py -> the factor that carries 2^e beside a, as a compressor returns it: C of a column ID, s of an SVD, X of a
# two-sided ID.  The rebuild then runs at 2^e from its last product on and no intermediate leaves the range (a split-scale set whose
# diag(s) right or mid W0 overflows stays the caller's).
RESIDUAL_CARRIER = {"none": "left", "s": "s", "both": "mid"}
RESIDUAL_SHAPES = [(33, 65, 17), (257, 130, 40)]
RESIDUAL_KINDS = ("gauss", "wide_core")

_RESIDUAL = {}


def residual_batch(shape, dtype, mode):
    """(units, cells, stacked): per kind the unit-scale dict(a, left, right, mid, s) of residual_ref(_complex).gaussian_factors, the
    (kind index, e) of each entry, and the stacked operands with a and the mode's carrier times 2^e (made once, never changed)."""
    key = (tuple(shape), np.dtype(dtype), mode)
    if key not in _RESIDUAL:
        m, n, K = shape
        ref = rrc if is_complex(dtype) else rr
        rng = np.random.default_rng(47000 + 1000 * m + 10 * n + K + len(mode) + (5 if is_complex(dtype) else 0))
        units = [ref.gaussian_factors(rng, m, n, K, dtype, mode, wide_core=(kind == "wide_core")) for kind in RESIDUAL_KINDS]
        cells = [(i, e) for i in range(len(units)) for e in exponents(dtype)]
        car = RESIDUAL_CARRIER[mode]
        stacked = {}
        for name in ("a", "left", "right", "mid", "s"):
            if units[0][name] is None:
                stacked[name] = None
            else:
                stacked[name] = np.stack([scale(units[i][name], e) if name in ("a", car) else units[i][name] for i, e in cells])
                stacked[name].setflags(write=False)
        _RESIDUAL[key] = (units, cells, stacked)
    return _RESIDUAL[key]


def check_residual(f, e, err, nrm, e_out, unit_e_out, dtype):
    """One entry of a residual batch run on 2^e a and the carrier times 2^e: err, nrm and e descaled exactly, then residual_ref.bound
    against residual_ref.reference on the unit operands f (the complex twins for complex data).  The bound's 16 roundings of slack beside
    the chain length cover the three-bin accumulation: each bin is summed over a sub-chain of the single accumulator's chain, and the
    combination adds at most 5 roundings (two roots, a quotient, 1 + q^2, a product), or 3 (two scalings and a sum) and a root.
    e is unchanged arithmetic: bit for bit 2^e times the unit entry's (unit_e_out; None when the residual was not asked for).  err and nrm
    need not be: a block whose entries straddle a threshold of the scaled accumulation sums in another grouping."""
    ref = rrc if is_complex(dtype) else rr
    m, n = f["a"].shape
    K = f["left"].shape[1]
    assert np.isfinite(err) and np.isfinite(nrm)
    err1, nrm1 = float(descale(err, e)), float(descale(nrm, e))
    _, e_ref = ref.reference(f["a"], f["left"], f["right"], f["mid"], f["s"], K)
    B, err_bound, nrm_bound = ref.bound(f["a"], f["left"], f["right"], f["mid"], f["s"], K, dtype, ref.chain_length(m, n))
    wide = np.complex128 if is_complex(dtype) else np.float64
    assert abs(err1 - float(np.linalg.norm(e_ref))) <= err_bound, (err1, float(np.linalg.norm(e_ref)), err_bound)
    assert abs(nrm1 - float(np.linalg.norm(f["a"].astype(wide)))) <= nrm_bound, (nrm1, float(np.linalg.norm(f["a"].astype(wide))), nrm_bound)
    if e_out is not None:
        e1 = descale(e_out, e)
        assert np.all(np.abs(e1.astype(wide) - e_ref) <= B)
        assert same_bits(e1, unit_e_out), "e is not 2^e times the unit entry's"


def lassq_norm(x):
    """||x||_F of f64 / c128 data by the three accumulators of LAPACK 3.10's ?lassq, in f64: the host model of the kernels' accumulation."""
    v = np.asarray(x)
    v = np.concatenate([v.real.ravel(), v.imag.ravel()]) if is_complex(v.dtype) else v.ravel()
    v = v.astype(np.float64)
    av = np.abs(v)
    tsml, tbig, ssml, sbig = 2.0 ** -511, 2.0 ** 486, 2.0 ** 537, 2.0 ** -538
    big, sml = v[av >= tbig] * sbig, v[(av < tsml)] * ssml
    med = v[(av >= tsml) & (av < tbig)]
    abig, asml, amed = float(np.sum(big * big)), float(np.sum(sml * sml)), float(np.sum(med * med))
    if abig > 0:
        return np.sqrt(abig + (amed * sbig) * sbig) / sbig
    if asml > 0:
        if amed > 0:
            lo, hi = sorted((np.sqrt(amed), np.sqrt(asml) / ssml))
            return hi * np.sqrt(1 + (lo / hi) ** 2)
        return np.sqrt(asml) / ssml
    return np.sqrt(amed)
