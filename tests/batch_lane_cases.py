"""The multi-lane batch column ID (rc_batch_column_id_*, batch.batch_column_id_packed): the inputs and the per-slot checker, shared by
tests/test_batch_lane_cases_cpu.py (LAPACK in the input's own precision, standing in for the device, passes the checker on every case,
and every input has the property its test relies on) and tests/test_gpu_batch_lanes.py (the device).

Inputs, all seeded and made with NumPy on the host:
  graded(m, n)    Gaussian whose columns are scaled by a shuffled geomspace(1, 0.25, n): the pivot order is decided by the data, not
                  by the order of the columns or by the 1 % scatter of Gaussian column norms;
  redo_trigger()  X, 192 x 640, the matrix the optimistic pass of the batch must redo (see its docstring).

The checker (check_slot) holds one slot (C, Z, ind) to the reference sequence QR::compute_from(a) -> compress(RANK(k)) -> column_id()
of oracle/ref_lapack.py run in f64 on the f64 (c128) cast of the input.  Pivots: at every step where the data decides -- the runner-up
of the f64 factorization stays PIVOT_MARGIN below the pivot -- the slot's pivots must be the oracle's (helpers.agreed_pivot_prefix
returns k); a matrix with a closer call somewhere is additionally held to the near-tie proof helpers.greedy_pivot_slack on every pivot,
bounded as tests/test_gpu_batched_id.py bounds it, and agreed_pivot_prefix still asserts that its first disagreement is a near tie.
Factors: Z and C Z of every slot against the f64 ID on the slot's own pivots (id_on_pivots), and against the oracle's column_id() where
the pivots are the oracle's, all to TOL[dtype]["factor"]."""
import numpy as np
import scipy.linalg

from oracle import ref_lapack as o
from tests.helpers import TOL, agreed_pivot_prefix, greedy_pivot_slack, is_permutation, rel, stable_prefix

REAL = (np.float64, np.float32)
COMPLEX = (np.complex128, np.complex64)

# How far below the pivot the runner-up's partial norm must stay, relatively, for the pivot to count as decided by the data.  ?geqp3
# trusts a down-dated norm until (vn1 / vn2)^2 <= tol3z = sqrt(eps), so the norms it compares carry a relative error of up to
# eps / tol3z = sqrt(eps): 3.5e-4 in f32, 1.5e-8 in f64.  The margin is about three times that in f32 and helpers' own f64 tie tolerance.
PIVOT_MARGIN = {np.dtype(np.float64): 1e-6, np.dtype(np.float32): 1e-3}
# helpers.greedy_pivot_slack's bound and the run it is applied over: tests/test_gpu_batched_id.py's TIE and SLACK_FLOOR
TIE = {np.dtype(np.float64): 1e-6, np.dtype(np.float32): 5e-3}
SLACK_FLOOR = {np.dtype(np.float64): 1e-4, np.dtype(np.float32): 1e-2}

# the redo trigger: rank and column count of the low-rank group, the generic columns, the rank asked for
X_SHAPE, X_RANK, X_LOW, X_K = (192, 640), 10, 480, 40


def real_of(dtype):
    return np.dtype(np.finfo(np.dtype(dtype)).dtype)


def is_complex(dtype):
    return np.dtype(dtype).kind == "c"


def wide_of(dtype):
    return np.complex128 if is_complex(dtype) else np.float64


def _gaussian(rng, shape, dtype):
    if is_complex(dtype):
        return o.random_gaussian(shape, rng, np.complex128)
    return rng.standard_normal(shape)


def graded(m, n, dtype, seed):
    """G(m, n): Gaussian, columns scaled by a shuffled geomspace(1, 0.25, n)."""
    rng = np.random.default_rng(seed)
    g = _gaussian(rng, (m, n), dtype)
    scale = np.geomspace(1.0, 0.25, n)
    rng.shuffle(scale)
    a = (g * scale).astype(dtype)
    a.setflags(write=False)
    return a


def redo_trigger(dtype, seed):
    """X(192, 640): X_LOW columns from a rank-X_RANK subspace with norms linspace(4, 2), 160 generic columns with norms
    linspace(1, 0.5), shuffled; k = X_K.  For m = 192 a cooperative panel of the blocked QRCP takes at most 480 candidates, and the 480
    largest norms are exactly the low-rank group: after X_RANK steps their residuals collapse while every excluded column is of order
    one, so the first panel has to end early and the optimistic schedule's check fails.  Returns (x, low): low marks the low-rank columns."""
    m, n = X_SHAPE
    rng = np.random.default_rng(seed)
    basis = np.linalg.qr(rng.standard_normal((m, X_RANK)))[0]
    lowc = basis @ rng.standard_normal((X_RANK, X_LOW))
    lowc *= np.linspace(4.0, 2.0, X_LOW) / np.linalg.norm(lowc, axis=0)
    gen = rng.standard_normal((m, n - X_LOW))
    gen *= np.linspace(1.0, 0.5, n - X_LOW) / np.linalg.norm(gen, axis=0)
    perm = rng.permutation(n)
    x = np.concatenate([lowc, gen], axis=1)[:, perm].astype(dtype)
    low = (np.arange(n) < X_LOW)[perm]
    x.setflags(write=False)
    return x, low


# ------------------------------------------------------------------------------------------------ the oracle
_ORACLE = {}


def oracle(a, k):
    """(full, cid, margins) of the f64 / c128 cast of a, computed once per matrix and never changed: the full pivoted QR, the rank-k
    column ID of the reference sequence, and per step j < k how far the runner-up's partial norm stays below the pivot's, relatively."""
    key = (a.shape, a.dtype.str, k, a.tobytes())
    if key not in _ORACLE:
        aw = np.asarray(a, dtype=wide_of(a.dtype))
        full = o.QR.compute_from(aw)
        cid = full.compress("RANK", k).column_id()
        _ORACLE[key] = (full, cid, pivot_margins(aw, full.r, full.ind, k))
    return _ORACLE[key]


def pivot_margins(aw, r, ind, k):
    """From the factorization A[:, ind] = Q R in f64: the partial norm of column c at step j is sqrt(||A[:, ind[c]]||^2 - sum_{i<j} |R[i, c]|^2),
    the pivot's own is |R[j, j]|.  Returns (|R[j, j]| - the largest other partial norm) / |R[j, j]| for j < k (1 at a last column)."""
    vn2 = (np.abs(aw[:, ind]) ** 2).sum(axis=0)
    out = []
    for j in range(k):
        rest = np.sqrt(np.maximum(vn2[j + 1:], 0.0))
        d = abs(r[j, j])
        out.append(float((d - rest.max()) / d) if rest.size else 1.0)
        vn2 = vn2 - np.abs(r[j]) ** 2
    return out


def pivots_decided(a, k):
    """Every one of the first k pivots of a is decided by the data at the accuracy of a's own precision."""
    return min(oracle(a, k)[2]) >= PIVOT_MARGIN[real_of(a.dtype)]


def r_of(a, ind, k):
    """R (k x n, pivoted order) of A[:, ind] in f64 / c128: what the slot's pivots factor, up to the phases of its rows."""
    return np.linalg.qr(np.asarray(a, dtype=wide_of(a.dtype))[:, ind], mode="r")[:k]


# ------------------------------------------------------------------------------------------------ the checker
def check_slot(c, z, ind, a, k):
    """One slot (C, Z, ind) of a batch against the oracle; every relative bound is TOL[dtype]["factor"] of tests/helpers.py.  Returns
    whether the slot took the oracle's pivots on all of ind[:k] (False: a near tie broken the other way, proven to be one above)."""
    m, n = a.shape
    rd = real_of(a.dtype)
    tol = TOL[rd]["factor"]
    c, z, ind = np.asarray(c), np.asarray(z), np.asarray(ind)
    assert c.shape == (m, k) and z.shape == (k, n) and ind.shape == (n,)
    assert c.dtype == a.dtype and z.dtype == a.dtype
    assert is_permutation(ind, n)
    assert np.all(np.isfinite(c)) and np.all(np.isfinite(z))
    assert rel(c, a[:, ind[:k]]) <= tol
    assert np.array_equal(z[:, ind[:k]], np.eye(k, dtype=a.dtype))
    full, cid, margins = oracle(a, k)
    assert stable_prefix(full.r, rd) >= k
    mine = r_of(a, ind, k)
    agreed = agreed_pivot_prefix(ind[:k], mine, full.ind[:k], full.r[:k], rd)  # asserts that a first disagreement is a near tie
    if min(margins) >= PIVOT_MARGIN[rd]:
        assert agreed == k, f"pivot {agreed} of {k} differs from the oracle's although the data decides it (margin {margins[agreed]:.2e})"
    else:
        d = np.abs(np.diag(full.r)[:k])
        ns = min(k, int(np.sum(d >= SLACK_FLOOR[rd] * d[0])))
        aw = np.asarray(a, dtype=wide_of(a.dtype))
        slack = greedy_pivot_slack_any(aw, mine, ind, ns)
        assert max(slack or [0.0]) <= TIE[rd], f"pivot {int(np.argmax(slack))} is not the largest remaining column: slack {max(slack):.2e}"
    # the f64 ID on the slot's OWN pivots holds Z and C Z of every slot, whichever near-tied pivots it took ...
    wide = wide_of(a.dtype)
    c_own, z_own = id_on_pivots(a, ind, k)
    assert rel(z, z_own) <= tol, rel(z, z_own)
    assert rel(c.astype(wide) @ z.astype(wide), c_own @ z_own) <= tol
    if agreed == k:  # ... and with the oracle's pivots that is the oracle's own column_id()
        assert rel(z, cid.z) <= tol, rel(z, cid.z)
        assert rel(c.astype(wide) @ z.astype(wide), cid.c @ cid.z) <= tol
    return agreed == k


def id_on_pivots(a, ind, k):
    """(C, Z) of the rank-k column ID that the pivots `ind` give, in f64 / c128: C = A[:, ind[:k]], Z = [I | R11^-1 R12] P^T with R of
    A[:, ind] = Q R (QRTraits::column_id's formula on a factorization made here, independent of the call under test)."""
    aw = np.asarray(a, dtype=wide_of(a.dtype))
    ind = np.asarray(ind)
    r = r_of(a, ind, k)
    zp = np.zeros((k, aw.shape[1]), dtype=aw.dtype)
    zp[:, :k] = np.eye(k)
    if k < aw.shape[1]:
        zp[:, k:] = scipy.linalg.solve_triangular(r[:, :k], r[:, k:])
    z = np.empty_like(zp)
    z[:, ind] = zp
    return aw[:, ind[:k]], z


def greedy_pivot_slack_any(aw, r, ind, k):
    """helpers.greedy_pivot_slack, which squares real entries, extended to complex data by the same formula on moduli."""
    if not np.iscomplexobj(aw):
        return greedy_pivot_slack(aw, r, ind, k)
    vn2 = (np.abs(aw[:, ind]) ** 2).sum(axis=0)
    slack = []
    for j in range(k):
        rest = np.sqrt(np.maximum(vn2[j:], 0.0))
        mx = float(rest.max())
        slack.append((mx - abs(r[j, j])) / mx if mx > 0 else 0.0)
        vn2 = vn2 - np.abs(r[j]) ** 2
    return slack


def oracle_slot(a, k):
    """The reference sequence in a's own precision: (C, Z, ind) as a slot of the batch holds them."""
    cid = o.QR.compute_from(a).compress("RANK", k).column_id()
    return cid.c, cid.z, cid.col_ind


# ------------------------------------------------------------------------------------------------ the cases
# case -> (m, n, k); the seeds of its matrices follow in the functions below
A_SHAPE = (160, 192, 40)            # two panels, the second of 8 steps
A_SCHEDULES = [(1, 1), (1, 8), (3, 8), (5, 2), (9, 4)]  # (count, lanes)
B_KINDS = "GXGXXGX"                 # mixed redo: the X are redone, the G verified
C_SHAPE = (160, 160, 159)           # five panels per matrix
D_SHAPE = (160, 128, 128)           # k == n
E_SHAPES = [(96, 80, 20), (200, 150, 5)]     # not blocked-eligible: m, n < 128; k < 8
F_SHAPES = [(128, 512, 32), (1024, 128, 32), (64, 512, 16)]  # short-wide cooperative, tall-skinny, short-wide with m < 128
H_SHAPES = [(96, 70, 20), (200, 150, 33)]    # complex


def seed_of(tag, m, n, i):
    return 100000 * (ord(tag) - ord("A") + 1) + 100 * m + n + 7919 * i


def case_a(dtype, count):
    m, n, _ = A_SHAPE
    return [graded(m, n, dtype, seed_of("A", m, n, i)) for i in range(count)]


def case_b(dtype):
    """[(matrix, is_x), ...]: seven 192 x 640 matrices, G and X by B_KINDS, distinct seeds."""
    m, n = X_SHAPE
    out = []
    for i, kind in enumerate(B_KINDS):
        a = redo_trigger(dtype, seed_of("B", m, n, i))[0] if kind == "X" else graded(m, n, dtype, seed_of("B", m, n, i))
        out.append((a, kind == "X"))
    return out


def pinned_slots_per_lane():
    """State slots a lane's pinned buffer holds for the optimistic pass: c->pinned_size (rc_common.hpp; qrb_begin allocates 1 << 16 bytes)
    over sizeof(QrbState) (kernels_qrblk.hip: 160 bytes)."""
    return 65536 // 160


def case_c_count():
    panels = -(-C_SHAPE[2] // 32)  # kNB = 32 steps per panel
    assert panels == 5
    return pinned_slots_per_lane() // panels + 3


def case_c(count):
    m, n, _ = C_SHAPE
    return [graded(m, n, np.float32, seed_of("C", m, n, i)) for i in range(count)]


def case_c_flush_at():
    """Index of the first matrix of case C that finds no pinned slots left: the one issued after the mid-call flush."""
    return pinned_slots_per_lane() // 5


def case_shape(tag, shape, dtype, count):
    m, n, _ = shape
    return [graded(m, n, dtype, seed_of(tag, m, n, i)) for i in range(count)]
