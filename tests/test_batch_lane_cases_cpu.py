"""tests/batch_lane_cases.py on the host: (a) LAPACK in the input's own precision, standing in for the device, passes the per-slot checker
on every case of tests/test_gpu_batch_lanes.py, so a failure there is the library's and not the reference's or the bound's; (b) every
constructed input has the property its test relies on -- the redo trigger's structure, pivots that the data decides, the slot arithmetic
of the flush case; (c) the checker rejects slots that are wrong in the ways a scheduling bug makes them wrong."""
import numpy as np
import pytest

from oracle import ref_lapack as o
from tests import batch_lane_cases as bl
from tests.helpers import TOL, stable_prefix

ALL = list(bl.REAL) + list(bl.COMPLEX)


def own_precision_passes(a, k):
    bl.check_slot(*bl.oracle_slot(a, k), a, k)


# ------------------------------------------------------------------------------------------------ (a) the oracle as the call under test
@pytest.mark.parametrize("dtype", bl.REAL)
def test_the_oracle_passes_the_checker_on_the_blocked_cases(dtype):
    m, n, k = bl.A_SHAPE
    for a in bl.case_a(dtype, max(c for c, _ in bl.A_SCHEDULES)):
        assert a.shape == (m, n) and a.dtype == np.dtype(dtype)
        own_precision_passes(a, k)
    for a, _ in bl.case_b(dtype):
        own_precision_passes(a, bl.X_K)


def test_the_oracle_passes_the_checker_around_the_flush():
    count = bl.case_c_count()
    mats = bl.case_c(count)
    at = bl.case_c_flush_at()
    for i in (0, at - 2, at - 1, at, at + 1, at + 2, count - 1):
        own_precision_passes(mats[i], bl.C_SHAPE[2])


@pytest.mark.parametrize("dtype", bl.REAL)
def test_the_oracle_passes_the_checker_off_the_blocked_route(dtype):
    for a in bl.case_shape("D", bl.D_SHAPE, dtype, 3):
        own_precision_passes(a, bl.D_SHAPE[2])
        c, z, ind = bl.oracle_slot(a, bl.D_SHAPE[2])  # k == n: Z is a permuted identity and C Z is the matrix
        assert np.array_equal(np.sort(z, axis=1)[:, -1], np.ones(z.shape[0])) and np.count_nonzero(z) == z.shape[0]
    for shape in bl.E_SHAPES:
        for a in bl.case_shape("E", shape, dtype, 5):
            own_precision_passes(a, shape[2])
    for shape in bl.F_SHAPES:
        for a in bl.case_shape("F", shape, dtype, 3):
            own_precision_passes(a, shape[2])


@pytest.mark.parametrize("dtype", bl.COMPLEX)
def test_the_oracle_passes_the_checker_on_the_complex_cases(dtype):
    for shape in bl.H_SHAPES:
        for a in bl.case_shape("H", shape, dtype, 5):
            assert a.dtype == np.dtype(dtype) and np.abs(a.imag).max() > 0
            own_precision_passes(a, shape[2])


# ------------------------------------------------------------------------------------------------ (b) the inputs are what they say
@pytest.mark.parametrize("dtype", bl.REAL)
def test_the_redo_trigger_has_its_structure(dtype):
    m, n = bl.X_SHAPE
    cap = 8 * 64 - 32  # candidates a cooperative panel takes at most: qrb_issue's min(cw, 8 * kCoopWgs - 32), kCoopWgs = 64
    assert cap == bl.X_LOW
    assert (4 << 20) // (np.dtype(dtype).itemsize * m) >= cap  # the candidate budget (RC_QRCP_CAND_MB = 4) asks for more than the cap
    for i, (x, is_x) in enumerate(bl.case_b(dtype)):
        if not is_x:
            continue
        x2, low = bl.redo_trigger(dtype, bl.seed_of("B", m, n, i))
        assert np.array_equal(x, x2) and low.sum() == bl.X_LOW
        x64 = x.astype(np.float64)
        nrm = np.linalg.norm(x64, axis=0)
        assert set(np.argsort(-nrm)[:cap]) == set(np.nonzero(low)[0])  # the panel's candidates are exactly the low-rank group
        assert nrm[low].min() > 1.9 and nrm[~low].max() < 1.1 and nrm[~low].min() > 0.45
        s = np.linalg.svd(x64[:, low], compute_uv=False)
        assert s[bl.X_RANK] <= 1e-5 * s[0]  # rank X_RANK to the precision of the storage
        # after X_RANK steps nothing is left of the candidates, and every column the panel left out is still of order one
        full = o.QR.compute_from(x)
        assert low[full.ind[:bl.X_RANK]].all() and not low[full.ind[bl.X_RANK:bl.X_K]].any()
        q = full.q[:, :bl.X_RANK].astype(np.float64)
        resid = np.linalg.norm(x64 - q @ (q.T @ x64), axis=0)
        assert resid[low].max() <= 1e-5 and resid[~low].min() >= 0.4
        assert stable_prefix(full.r, dtype) >= bl.X_K


def test_the_data_decides_the_pivots_where_the_exact_comparison_is_made():
    """f64: every case is compared pivot by pivot.  f32 / c64: the listed matrices are (the others carry the near-tie proof)."""
    for dtype in (np.float64, np.complex128):
        mats = []
        if dtype == np.float64:
            mats += [(a, bl.A_SHAPE[2]) for a in bl.case_a(dtype, 9)] + [(a, bl.X_K) for a, _ in bl.case_b(dtype)]
            mats += [(a, bl.D_SHAPE[2]) for a in bl.case_shape("D", bl.D_SHAPE, dtype, 3)]
            mats += [(a, s[2]) for s in bl.E_SHAPES for a in bl.case_shape("E", s, dtype, 5)]
            mats += [(a, s[2]) for s in bl.F_SHAPES for a in bl.case_shape("F", s, dtype, 3)]
        else:
            mats += [(a, s[2]) for s in bl.H_SHAPES for a in bl.case_shape("H", s, dtype, 5)]
        for a, k in mats:
            assert bl.pivots_decided(a, k), (a.shape, k, min(bl.oracle(a, k)[2]))
    e0, e1 = bl.E_SHAPES
    assert [bl.pivots_decided(a, e0[2]) for a in bl.case_shape("E", e0, np.float32, 5)] == [False, True, False, True, True]
    assert [bl.pivots_decided(a, e1[2]) for a in bl.case_shape("E", e1, np.float32, 5)] == [True, True, False, True, True]
    h0 = bl.H_SHAPES[0]
    assert [bl.pivots_decided(a, h0[2]) for a in bl.case_shape("H", h0, np.complex64, 5)] == [True, False, False, True, True]


def test_the_flush_case_overruns_one_lane_by_three_matrices():
    assert bl.pinned_slots_per_lane() == 409
    assert bl.case_c_count() == 84 and bl.case_c_flush_at() == 81
    mats = bl.case_c(3)
    assert len({a.tobytes() for a in mats}) == 3 and mats[0].dtype == np.float32 and mats[0].shape == bl.C_SHAPE[:2]


def test_graded_columns_span_the_factor_four():
    a = bl.graded(4000, 64, np.float64, 1)
    nrm = np.sort(np.linalg.norm(a, axis=0))
    assert 3.5 <= nrm[-1] / nrm[0] <= 4.5
    assert not np.array_equal(np.argsort(-np.linalg.norm(a, axis=0)), np.arange(64))  # shuffled: not the order of the columns


# ------------------------------------------------------------------------------------------------ (c) the checker rejects wrong slots
def rejected(c, z, ind, a, k):
    try:
        bl.check_slot(c, z, ind, a, k)
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize("dtype", bl.REAL)
def test_the_checker_rejects_the_slots_a_scheduling_bug_would_leave(dtype):
    m, n, k = bl.A_SHAPE
    a, b = bl.case_a(dtype, 2)
    c, z, ind = bl.oracle_slot(a, k)
    assert not rejected(c, z, ind, a, k)
    assert rejected(*bl.oracle_slot(b, k), a, k)  # a neighbour's result in this slot
    # a half-factored matrix: the first panel's 32 pivots, the last 8 positions never pivoted (the columns as they stood)
    half = o.QR.compute_from(a).compress("RANK", 32).column_id()
    rest = [j for j in range(n) if j not in set(ind[:32])]
    stale_ind = np.concatenate([ind[:32], rest])
    zs = np.zeros_like(z)
    zs[:32] = half.z
    zs[np.arange(32, k), stale_ind[32:k]] = 1
    assert rejected(a[:, stale_ind[:k]], zs, stale_ind, a, k)
    z2 = z.copy()
    z2[:, ind[k:]] *= 1 + 10 * TOL[np.dtype(dtype)]["factor"]  # the solved block of Z off by ten times the tolerance
    assert rejected(c, z2, ind, a, k)
    ind2 = ind.copy()
    ind2[[0, 1]] = ind2[[1, 0]]
    assert rejected(c, z, ind2, a, k)  # C and Z no longer belong to the permutation reported
    ind3 = ind.copy()
    ind3[-1] = ind3[0]
    assert rejected(c, z, ind3, a, k)  # not a permutation


def pivots_with_one_tie_broken_the_other_way(a, k):
    """Greedy pivots of a in f64 that take the runner-up at the step where the first two partial norms are closest: what a correct
    implementation in a's precision may legitimately return.  (position of the swap, full permutation)"""
    w = np.array(a, dtype=bl.wide_of(a.dtype))
    at = int(np.argmin(bl.oracle(a, k)[2]))
    left = list(range(a.shape[1]))
    ind = []
    for j in range(k):
        nrm = np.linalg.norm(w[:, left], axis=0)
        order = np.argsort(-nrm)
        p = left[order[1 if j == at else 0]]
        q = w[:, p] / np.linalg.norm(w[:, p])
        w = w - np.outer(q, q.conj() @ w)
        ind.append(p)
        left.remove(p)
    return at, np.array(ind + left)


@pytest.mark.parametrize("dtype", [np.float32, np.complex64])
def test_a_slot_with_a_tie_broken_the_other_way_is_held_to_the_id_of_its_own_pivots(dtype):
    if bl.is_complex(dtype):
        shape = bl.H_SHAPES[1]
        a = bl.case_shape("H", shape, dtype, 1)[0]
    else:
        shape = bl.A_SHAPE
        a = bl.case_a(dtype, 1)[0]
    k = shape[2]
    assert not bl.pivots_decided(a, k)
    at, ind = pivots_with_one_tie_broken_the_other_way(a, k)
    full = bl.oracle(a, k)[0]
    assert np.array_equal(ind[:at], full.ind[:at]) and ind[at] != full.ind[at] and ind[at + 1] == full.ind[at]
    c = a[:, ind[:k]]
    z = bl.id_on_pivots(a, ind, k)[1].astype(dtype)
    assert bl.check_slot(c, z, ind, a, k) is False  # accepted, on the branch of the other pivots
    tail = ind[k:]
    z12_off = z.copy()
    z12_off[:, tail] *= 1 + 10 * TOL[bl.real_of(dtype)]["factor"]  # the solved block off by ten times the tolerance
    assert rejected(c, z12_off, ind, a, k)
    z12_zero = z.copy()
    z12_zero[:, tail] = 0  # right C, right identity block, nothing solved
    assert rejected(c, z12_zero, ind, a, k)
    other = bl.oracle_slot(a, k)[1]  # the Z of the oracle's pivots does not belong to these
    assert rejected(c, other, ind, a, k)
