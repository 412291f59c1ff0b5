"""Batched column ID of many small same-shaped matrices (rc_column_id_rank_batched_*, batch.column_id_rank_batched).

Per matrix the reference sequence QR::compute_from(a) -> compress(.) -> column_id() (src/qr.rs:187-200, :270-309;
examples/interpolative_decomposition.rs:25-32), checked against the SciPy-LAPACK oracle, the committed cfg1 golden vectors
and the lone call rc_column_id_rank_*; plus the contract of the batch itself (independence of the neighbours, layouts,
graph capture, argument checks, containment of non-finite input)."""
import ctypes

import numpy as np
import pytest
import torch

import rusty_compression_amd as rc
from oracle import ref_lapack as o
from rusty_compression_amd import _lib
from rusty_compression_amd.batch import column_id_rank
from tests.helpers import TOL, agreed_pivot_prefix, batched_launch, golden, greedy_pivot_slack, is_permutation, npy, rel, stable_prefix

pytestmark = pytest.mark.gpu

TIE = {np.dtype(np.float64): 1e-6, np.dtype(np.float32): 5e-3}
SLACK_FLOOR = {np.dtype(np.float64): 1e-4, np.dtype(np.float32): 1e-2}


def batched(a, k, tol=0.0):
    c, z, ind, ranks = rc.column_id_rank_batched(a, k, tol)
    torch.cuda.synchronize()
    return npy(c), npy(z), npy(ind), npy(ranks)


def decaying(rng, m, n, dtype, lo=1e-10):
    return o.random_approximate_low_rank_matrix((m, n), 1.0, lo, rng).astype(dtype)


def r_of(a, ind, k):
    """R (k x n, pivoted order) of A[:, ind] in f64: what the batched call factored, up to the signs of its rows."""
    return np.linalg.qr(np.asarray(a, dtype=np.float64)[:, ind], mode="r")[:k]


def check_one(a, c, z, ind, r, k, dtype, oracle_tol=None):
    """One matrix of a batch against the oracle: pivots, C bit for bit, Z's identity block, the reconstruction C Z."""
    m, n = a.shape
    assert is_permutation(ind, n)
    assert 0 <= r <= k
    assert np.array_equal(c[:, :r], a[:, ind[:r]])
    assert np.array_equal(z[:, ind[:r]][:r], np.eye(r, dtype=dtype))
    assert not np.any(c[:, r:]) and not np.any(z[r:])
    full = o.QR.compute_from(a)
    ref = full.compress_qr_rank(r) if oracle_tol is None else full.compress_qr_tolerance(oracle_tol)
    assert ref.rank() == r
    if r == 0:
        return
    mine = r_of(a, ind, r)
    agreed = agreed_pivot_prefix(ind, mine, ref.ind, ref.r, dtype)
    # greedy_pivot_slack recomputes the partial norms in f64 as ||a||^2 - sum r_ij^2: it resolves the tie tolerance only while
    # the partial norms stay above ~sqrt(eps_f64 / tie) of the column norms, so it is applied over that leading run
    d = np.abs(np.diag(ref.r)[:r]).astype(np.float64)
    ns = min(stable_prefix(ref.r, dtype), int(np.sum(d >= SLACK_FLOOR[np.dtype(dtype)] * d[0])))
    assert max(greedy_pivot_slack(a, mine, ind, ns) or [0.0]) <= TIE[np.dtype(dtype)]
    if agreed == r:  # same pivots: the same factors as the oracle's column_id
        oc = ref.column_id()
        assert rel(c[:, :r] @ z[:r], oc.c @ oc.z) <= TOL[np.dtype(dtype)]["factor"]
    # whichever near-tied pivots were taken, C Z reproduces A as well as the oracle's rank-r ID does (to the working precision)
    err = np.linalg.norm(a - c[:, :r] @ z[:r]) / np.linalg.norm(a)
    oerr = np.linalg.norm(a - ref.column_id().to_mat()) / np.linalg.norm(a)
    assert err <= 1.5 * oerr + 100 * np.finfo(dtype).eps


# ---------------------------------------------------------------- 1. golden cfg1 inside a batch of strangers
@pytest.mark.parametrize("tag,k,tol", [("rank32", 32, 0.0), ("tol1e4", 128, 1e-4)])
def test_golden_cfg1_at_several_positions(tag, k, tol):
    g = golden("cfg1_id.npz")
    a0 = golden("cfg1_sketch_rsvd.npz")["a"]
    rng = np.random.default_rng(11)
    batch = rng.standard_normal((7, 512, 256))
    slots = (0, 3, 6)
    for s in slots:
        batch[s] = a0
    c, z, ind, ranks = batched(torch.from_numpy(batch).cuda(), k, tol)
    r = int(g[f"{tag}_rank"])
    assert r == (32 if tag == "rank32" else 117)
    for s in slots:
        assert ranks[s] == r
        assert np.array_equal(ind[s][:r], g[f"{tag}_ind"][:r])
        assert rel(c[s][:, :r], g[f"{tag}_c"]) <= 1e-10
        # Z solves R11 Z12 = R12 with cond(R11) ~ 1/tol: compare through the action on A's columns
        assert rel(c[s][:, :r] @ z[s][:r], g[f"{tag}_c"] @ g[f"{tag}_z"]) <= 1e-10
        assert np.array_equal(c[s], c[slots[0]]) and np.array_equal(z[s], z[slots[0]])


# ---------------------------------------------------------------- 2. oracle parity across shapes
SHAPES = [(96, 40, 1), (40, 96, 40), (200, 200, 128), (333, 77, 77), (77, 333, 33), (512, 512, 128), (17, 500, 17), (500, 9, 5)]


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("m,n,k", SHAPES)
def test_oracle_parity_across_shapes(m, n, k, dtype):
    rng = np.random.default_rng(m * 1000 + n + k)
    mats = [rng.standard_normal((m, n)).astype(dtype), decaying(rng, m, n, dtype), decaying(rng, m, n, dtype, 1e-3)]
    c, z, ind, ranks = batched(torch.from_numpy(np.stack(mats)).cuda(), k)
    kk = min(k, m, n)
    assert c.shape == (3, m, kk) and z.shape == (3, kk, n)
    for i, a in enumerate(mats):
        assert ranks[i] == kk
        check_one(a, c[i], z[i], ind[i], int(ranks[i]), kk, dtype)


# ---------------------------------------------------------------- 3. tolerance mode
@pytest.mark.parametrize("dtype,tol", [(np.float64, 1e-8), (np.float32, 1e-4)])
def test_tolerance_mode_exact_ranks_zero_and_full(dtype, tol):
    rng = np.random.default_rng(3)
    m, n, k = 150, 120, 64
    mats = []
    for rank in (5, 17, 40):
        mats.append((rng.standard_normal((m, rank)) @ rng.standard_normal((rank, n))).astype(dtype))
    mats.append(np.zeros((m, n), dtype=dtype))
    mats += [rng.standard_normal((m, n)).astype(dtype) for _ in range(2)]
    c, z, ind, ranks = batched(torch.from_numpy(np.stack(mats)).cuda(), k, tol)
    assert not np.isnan(c).any() and not np.isnan(z).any()
    assert list(ranks) == [5, 17, 40, 0, k, k]
    for i, a in enumerate(mats):
        r = int(ranks[i])
        assert is_permutation(ind[i], n)
        assert not np.any(c[i][:, r:]) and not np.any(z[i][r:])
        if r == 0:
            continue
        if r < k:  # the oracle's own compress(ADAPTIVE(tol)) stops at the same rank
            check_one(a, c[i], z[i], ind[i], r, k, dtype, oracle_tol=tol)
        else:
            check_one(a, c[i], z[i], ind[i], r, k, dtype)


# ---------------------------------------------------------------- 4. independence of position and neighbours
def test_bits_independent_of_position_and_neighbours():
    rng = np.random.default_rng(4)
    m, n, k = 64, 48, 16
    x = decaying(rng, m, n, np.float64)
    alone, probe = batched_launch(lambda: batched(torch.from_numpy(x[None]).cuda(), k, 1e-6))
    big = torch.from_numpy(rng.standard_normal((2 * probe["slots"] + 37, m, n))).cuda()  # slots: the persistent grid of this shape
    big[5] *= 1e-3  # different neighbours, among them a tiny one
    for s in (len(big) // 2, len(big) - 1):
        b = big.clone()
        b[s] = torch.from_numpy(x)
        got, lab = batched_launch(lambda: batched(b, k, 1e-6))
        assert lab["count"] > 2 * lab["grid"]  # both positions are some workgroup's second or third matrix
        for u, v in zip(alone, got):
            assert np.array_equal(u[0], v[s])


# ---------------------------------------------------------------- 5. layouts
def test_layouts_give_the_same_bits():
    rng = np.random.default_rng(5)
    cnt, m, n, k = 9, 70, 50, 20
    base = torch.from_numpy(rng.standard_normal((cnt, m, n))).cuda()
    ref = batched(base.contiguous(), k)
    transposed = base.transpose(1, 2).contiguous().transpose(1, 2)      # every matrix column-major
    padded = torch.zeros((cnt, m + 3, n + 5), dtype=base.dtype, device=base.device)
    padded[:, :m, :n] = base
    last = base.permute(1, 2, 0).contiguous().permute(2, 0, 1)          # a [m, n, count] array
    for view in (transposed, padded[:, :m, :n], last):
        got = batched(view, k)
        for u, v in zip(ref, got):
            assert np.array_equal(u, v)
    # a_batch_stride = 0: count identical results
    same = base[2:3].expand(6, m, n)
    assert same.stride(0) == 0
    got = batched(same, k)
    for u, v in zip(ref, got):
        for i in range(6):
            assert np.array_equal(v[i], u[2])


# ---------------------------------------------------------------- 6. graph capture
def test_graph_capture_replays_the_eager_bits():
    rng = np.random.default_rng(6)
    cnt, m, n, k = 33, 128, 96, 24
    lib = _lib.lib()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        a = torch.from_numpy(rng.standard_normal((cnt, m, n))).cuda()
        eager = batched(a, k, 1e-9)
        ctx = _lib.Context(torch.cuda.current_device(), st.cuda_stream)
        c = torch.zeros((cnt, m, k), dtype=a.dtype, device=a.device)
        z = torch.zeros((cnt, k, n), dtype=a.dtype, device=a.device)
        ind = torch.zeros((cnt, n), dtype=torch.int64, device=a.device)
        ranks = torch.zeros(cnt, dtype=torch.int64, device=a.device)
        st.synchronize()
        args = (_lib.rc_matrix(a.data_ptr(), m, n, a.stride(1), a.stride(2)), ctypes.c_int64(a.stride(0)), ctypes.c_int32(cnt), ctypes.c_int64(k),
                ctypes.c_double(1e-9), _lib.mat(c[0]), ctypes.c_int64(m * k), _lib.mat(z[0]), ctypes.c_int64(k * n), _lib.i64p(ind), _lib.i64p(ranks))
        ctx.check(lib.rc_column_id_rank_batched_f64(ctx._h, *args))  # eager once: sizes the workspace
        ctx.synchronize()
        ctx.get_health()
        for t in (c, z, ind, ranks):
            t.zero_()
        st.synchronize()
        graph = ctypes.c_void_p(None)
        ctx.check(lib.rc_graph_begin_capture(ctx._h))
        ctx.check(lib.rc_column_id_rank_batched_f64(ctx._h, *args))
        ctx.check(lib.rc_graph_end_capture(ctx._h, ctypes.byref(graph)))
        try:
            ctx.check(lib.rc_graph_launch(ctx._h, graph))
            ctx.synchronize()
            for u, v in zip(eager, (c, z, ind, ranks)):
                assert np.array_equal(u, npy(v))
            assert ctx.get_health() == 0
        finally:
            ctx.check(lib.rc_graph_destroy(ctx._h, graph))
            ctx.close()


# ---------------------------------------------------------------- 7. agreement with the lone call
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_agrees_with_the_lone_call(dtype):
    rng = np.random.default_rng(7)
    m, n, k = 300, 180, 40
    mats = [decaying(rng, m, n, dtype) for _ in range(3)] + [rng.standard_normal((m, n)).astype(dtype) for _ in range(2)]
    c, z, ind, ranks = batched(torch.from_numpy(np.stack(mats)).cuda(), k)
    for i, a in enumerate(mats):
        lc, lz, lind = (npy(t) for t in column_id_rank(torch.from_numpy(a).cuda(), k))
        lr = r_of(a, lind, k)
        agreed = agreed_pivot_prefix(ind[i], r_of(a, ind[i], k), lind, lr, dtype)
        if agreed == k:
            assert np.array_equal(ind[i][:k], lind[:k])
            assert rel(c[i] @ z[i], lc @ lz) <= TOL[np.dtype(dtype)]["factor"]


# ---------------------------------------------------------------- 8. arguments
def _call(a, cnt, k, tol, c, cbs, z, zbs, dtype=torch.float64):
    """One raw call; a, c and z are [2, rows, cols] buffers so that even a call the checks let through stays inside them."""
    ctx = _lib.default_context()
    fn = getattr(_lib.lib(), f"rc_column_id_rank_batched_{_lib.suffix(dtype)}")
    ind = torch.empty((2, a.shape[2]), dtype=torch.int64, device="cuda")
    ranks = torch.empty(2, dtype=torch.int64, device="cuda")
    return fn(ctx._h, _lib.mat(a[0]), ctypes.c_int64(a.stride(0)), ctypes.c_int32(cnt), ctypes.c_int64(k), ctypes.c_double(tol), _lib.mat(c[0]),
              ctypes.c_int64(cbs), _lib.mat(z[0]), ctypes.c_int64(zbs), _lib.i64p(ind), _lib.i64p(ranks))


def test_argument_checks():
    dev = "cuda"
    e = lambda r, c: torch.zeros((2, r, c), dtype=torch.float64, device=dev)  # noqa: E731
    INVALID = 5
    assert _call(e(520, 130), 2, 8, 0.0, e(520, 8), 520 * 8, e(8, 130), 8 * 130) == INVALID        # m > 512
    assert _call(e(130, 520), 2, 8, 0.0, e(130, 8), 130 * 8, e(8, 520), 8 * 520) == INVALID        # n > 512
    a = e(200, 200)
    assert _call(a, 2, 129, 0.0, e(200, 129), 200 * 129, e(129, 200), 129 * 200) == INVALID  # k > 128
    assert _call(a, 2, 0, 0.0, e(200, 1), 200, e(1, 200), 200) == INVALID                    # k < 1
    assert _call(a, 2, 16, 1.0, e(200, 16), 200 * 16, e(16, 200), 16 * 200) == INVALID       # tol >= 1
    assert _call(a, 2, 16, -1e-3, e(200, 16), 200 * 16, e(16, 200), 16 * 200) == INVALID     # tol < 0
    assert _call(a, 2, 16, 0.0, e(200, 16), 200 * 16 - 1, e(16, 200), 16 * 200) == INVALID   # C of two matrices overlap
    assert _call(a, 2, 16, 0.0, e(200, 16), 200 * 16, e(16, 200), 15 * 200) == INVALID       # Z of two matrices overlap
    assert _call(a, 2, 16, 0.0, e(200, 15), 200 * 15, e(16, 200), 16 * 200) == INVALID       # wrong C shape
    assert _call(a, 2, 16, 0.0, e(200, 16), 200 * 16, e(16, 199), 16 * 199) == INVALID       # wrong Z shape
    msg = _lib.lib().rc_last_error_message(_lib.default_context()._h).decode()
    assert "z" in msg
    assert _call(a, 0, 16, 0.0, e(200, 16), 200 * 16, e(16, 200), 16 * 200) == 0            # count = 0: nothing to do
    with pytest.raises(AssertionError, match="rc_column_id_rank_"):  # RC_INVALID_ARGUMENT: the reference asserts
        rc.column_id_rank_batched(torch.zeros((1, 600, 10), dtype=torch.float64, device=dev), 4)
    c, z, ind, ranks = rc.column_id_rank_batched(torch.zeros((0, 30, 20), dtype=torch.float32, device=dev), 8)
    assert c.shape == (0, 30, 8) and z.shape == (0, 8, 20) and ind.shape == (0, 20) and ranks.shape == (0,)


# ---------------------------------------------------------------- 9. containment of non-finite input
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_nan_stays_in_its_matrix(dtype):
    rng = np.random.default_rng(9)
    cnt, m, n, k = 12, 90, 70, 30
    clean = torch.from_numpy(rng.standard_normal((cnt, m, n))).to(dtype).cuda()
    ref = batched(clean, k, 1e-5)
    bad = clean.clone()
    bad[4, 17, 23] = float("nan")
    bad[8, :, 5] = float("inf")
    got = batched(bad, k, 1e-5)
    for i in range(cnt):
        assert is_permutation(got[2][i], n) and 0 <= got[3][i] <= k
        if i in (4, 8):
            continue
        for u, v in zip(ref, got):
            assert np.array_equal(u[i], v[i])
