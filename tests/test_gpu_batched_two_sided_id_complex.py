"""Batched two-sided ID of many small same-shaped COMPLEX matrices (rc_two_sided_id_rank_batched_c64 / _c32,
batch.two_sided_id_rank_batched).

Per matrix the reference sequence QR::compute_from(a) -> compress(.) -> column_id() -> two_sided_id() on complex data (an LQ of C,
i.e. the pivoted QR of C^H, then row_id(); src/col_interp_decomp.rs:116-125), checked against the SciPy-LAPACK oracle, the batched
complex column ID (phase 1, bit for bit) and the lone chain rc_column_id_rank_c* + rc_column_id_two_sided_c*; plus the contract of
the batch itself (independence of the neighbours, layouts, graph capture, conjugation symmetry, argument checks, containment of
non-finite input)."""
import ctypes

import numpy as np
import pytest
import torch

import rusty_compression_amd as rc
from oracle import ref_lapack as o
from rusty_compression_amd import _lib
from rusty_compression_amd.batch import column_id_rank
from tests.helpers import TOL, agreed_pivot_prefix, batched_launch, is_permutation, npy, rel

pytestmark = pytest.mark.gpu

C64, C32 = np.complex128, np.complex64


def real_of(dtype):
    return np.dtype(np.float64) if np.dtype(dtype) == np.dtype(C64) else np.dtype(np.float32)


def two_sided(a, k, tol=0.0):
    out = rc.two_sided_id_rank_batched(a, k, tol)
    torch.cuda.synchronize()
    return tuple(npy(t) for t in out)  # c, x, r, row_ind, col_ind, ranks


def gaussian(rng, m, n, dtype):
    return o.random_gaussian((m, n), rng, dtype)


def decaying(rng, m, n, dtype, lo=1e-10):
    return o.random_approximate_low_rank_matrix((m, n), 1.0, lo, rng, dtype)


def phased(rng, m, n, dtype, lo=1e-10):
    """A real decaying spectrum times random unit-modulus column phases."""
    a = o.random_approximate_low_rank_matrix((m, n), 1.0, lo, rng, np.float64)
    return (a * np.exp(2j * np.pi * rng.random(n))[None, :]).astype(dtype)


def row_r(a, col_ind, row_ind, r):
    """R (r x m, pivoted order) of C^H[:, row_ind] in c128, C = A[:, col_ind[:r]]: what phase 2 factored."""
    ch = np.asarray(a, dtype=np.complex128)[:, col_ind[:r]].conj().T
    return np.linalg.qr(ch[:, row_ind], mode="r")[:r]


def check_identities(a, c, x, rr, row_ind, col_ind, r, k, dtype):
    """The exact part of the contract: permutations, X gathered from A, c's identity rows, zero padding."""
    m, n = a.shape
    assert is_permutation(row_ind, m) and is_permutation(col_ind, n)
    assert 0 <= r <= k
    assert c.shape == (m, k) and x.shape == (k, k) and rr.shape == (k, n)
    assert np.array_equal(x[:r, :r], a[row_ind[:r]][:, col_ind[:r]])
    assert np.array_equal(c[row_ind[:r], :r], np.eye(r, dtype=dtype))
    assert not np.any(c[:, r:]) and not np.any(x[r:]) and not np.any(x[:, r:]) and not np.any(rr[r:])


def check_one(a, c, x, rr, row_ind, col_ind, r, k, dtype):
    """One matrix of a batch: the identities, row pivots against the oracle's LQ of C, and the reconstruction c x r."""
    check_identities(a, c, x, rr, row_ind, col_ind, r, k, dtype)
    if r == 0:
        return
    lq = o.LQ.compute_from(a[:, col_ind[:r]])
    agreed_pivot_prefix(row_ind, row_r(a, col_ind, row_ind, r), lq.ind, lq.l.T, real_of(dtype))  # a disagreement must be a near tie
    err = np.linalg.norm(a - c[:, :r] @ x[:r, :r] @ rr[:r]) / np.linalg.norm(a)
    ots = o.QR.compute_from(a).compress_qr_rank(r).column_id().two_sided_id()
    oerr = np.linalg.norm(a - ots.to_mat()) / np.linalg.norm(a)
    assert err <= 1.5 * oerr + 100 * np.finfo(real_of(dtype)).eps


# ---------------------------------------------------------------- 1. phase 1 is the batched complex column ID, bit for bit
# In LDS: c64 64 x 48, 96 x 96; c32 128 x 128.  Workspace: c64 128 x 128, and 512 x 256, 200 x 512 for both.
PHASE1 = {
    C64: [(64, 48, 16, 0.0), (96, 96, 64, 1e-6), (128, 128, 128, 0.0), (512, 256, 32, 1e-5), (200, 512, 100, 0.0)],
    C32: [(64, 48, 48, 0.0), (128, 128, 128, 1e-4), (512, 256, 32, 0.0), (200, 512, 100, 1e-3)],
}


@pytest.mark.parametrize("dtype,m,n,k,tol", [(d, *s) for d in (C64, C32) for s in PHASE1[d]])
def test_phase1_is_the_batched_column_id_bit_for_bit(dtype, m, n, k, tol):
    rng = np.random.default_rng(m + 7 * n + k)
    mats = [phased(rng, m, n, dtype), gaussian(rng, m, n, dtype), decaying(rng, m, n, dtype, 1e-4)]
    a = torch.from_numpy(np.stack(mats)).cuda()
    c, x, rr, row_ind, col_ind, ranks = two_sided(a, k, tol)
    cc, z, ind, cranks = (npy(t) for t in rc.column_id_rank_batched(a, k, tol))
    assert np.array_equal(col_ind, ind)
    assert np.array_equal(ranks, cranks)
    assert np.array_equal(rr, z)
    for i, ai in enumerate(mats):
        check_identities(ai, c[i], x[i], rr[i], row_ind[i], col_ind[i], int(ranks[i]), min(k, m, n), dtype)


# ---------------------------------------------------------------- 2. oracle parity across shapes
SHAPES = {
    C64: [(64, 48, 16), (96, 96, 96), (128, 128, 64), (512, 256, 32), (200, 512, 100), (1, 40, 1), (40, 1, 1), (30, 30, 30)],
    C32: [(64, 48, 48), (128, 128, 128), (512, 256, 32), (200, 512, 100), (1, 40, 1), (40, 1, 1)],
}


@pytest.mark.parametrize("dtype,m,n,k", [(d, *s) for d in (C64, C32) for s in SHAPES[d]])
def test_oracle_parity_across_shapes(dtype, m, n, k):
    rng = np.random.default_rng(m * 1000 + n + k + (1 if dtype == C64 else 8))
    mats = [gaussian(rng, m, n, dtype), phased(rng, m, n, dtype)]
    if min(m, n) > 1:
        mats.append(decaying(rng, m, n, dtype, 1e-3))
    c, x, rr, row_ind, col_ind, ranks = two_sided(torch.from_numpy(np.stack(mats)).cuda(), k)
    kk = min(k, m, n)
    assert c.shape == (len(mats), m, kk) and x.shape == (len(mats), kk, kk) and rr.shape == (len(mats), kk, n)
    for i, a in enumerate(mats):
        assert ranks[i] == kk
        check_one(a, c[i], x[i], rr[i], row_ind[i], col_ind[i], kk, kk, dtype)


# ---------------------------------------------------------------- 3. agreement with the lone chain
@pytest.mark.parametrize("dtype", [C64, C32])
@pytest.mark.parametrize("m,n,k", [(64, 48, 16), (300, 180, 40)])
def test_agrees_with_the_lone_chain(dtype, m, n, k):
    rng = np.random.default_rng(14 + m)
    mats = [phased(rng, m, n, dtype) for _ in range(2)] + [decaying(rng, m, n, dtype)] + [gaussian(rng, m, n, dtype) for _ in range(2)]
    a = torch.from_numpy(np.stack(mats)).cuda()
    c, x, rr, row_ind, col_ind, ranks = two_sided(a, k)
    bc, bz, bind, _ = rc.column_id_rank_batched(a, k)
    rd = real_of(dtype)
    tol = TOL[rd]["factor"]
    checked = 0
    for i, ai in enumerate(mats):
        r = int(ranks[i])
        # the lone column ID at rank r takes the same column pivots on the agreed prefix
        lc, lz, lind = (npy(t) for t in column_id_rank(a[i], r))
        agreed_cols = agreed_pivot_prefix(col_ind[i], np.linalg.qr(ai.astype(np.complex128)[:, col_ind[i]], mode="r")[:r], lind,
                                          np.linalg.qr(ai.astype(np.complex128)[:, lind], mode="r")[:r], rd)
        if agreed_cols == r:
            assert np.array_equal(col_ind[i][:r], lind[:r])
        # the lone two-sided call started from the batch's own C
        lone = rc.ColumnID(bc[i][:, :r].contiguous(), bz[i][:r].contiguous(), bind[i].clone()).two_sided_id()
        lrow = npy(lone.row_ind)
        agreed = agreed_pivot_prefix(row_ind[i], row_r(ai, col_ind[i], row_ind[i], r), lrow, row_r(ai, col_ind[i], lrow, r), rd)
        assert np.array_equal(npy(lone.r), rr[i][:r]) and np.array_equal(npy(lone.col_ind), col_ind[i])
        if agreed == r:
            checked += 1
            assert np.array_equal(row_ind[i][:r], lrow[:r])
            assert rel(c[i][:, :r], npy(lone.c)) <= tol
            assert rel(x[i][:r, :r], npy(lone.x)) <= tol
        # c x r reproduces A to within the column ID's own error
        err = np.linalg.norm(ai - c[i][:, :r] @ x[i][:r, :r] @ rr[i][:r]) / np.linalg.norm(ai)
        cerr = np.linalg.norm(ai - bc[i].cpu().numpy() @ bz[i].cpu().numpy()) / np.linalg.norm(ai)
        assert err <= 1.5 * cerr + 100 * np.finfo(rd).eps
    assert checked >= 3


# ---------------------------------------------------------------- 4. tolerance mode
@pytest.mark.parametrize("dtype,tol", [(C64, 1e-8), (C32, 1e-4)])
def test_tolerance_mode_exact_ranks_zero_and_full(dtype, tol):
    rng = np.random.default_rng(15)
    m, n, k = 150, 120, 64
    mats = [(gaussian(rng, m, rank, np.complex128) @ gaussian(rng, rank, n, np.complex128).conj()).astype(dtype) for rank in (5, 17, 40)]
    mats.append(np.zeros((m, n), dtype=dtype))
    mats += [gaussian(rng, m, n, dtype) for _ in range(2)]
    c, x, rr, row_ind, col_ind, ranks = two_sided(torch.from_numpy(np.stack(mats)).cuda(), k, tol)
    assert np.isfinite(c).all() and np.isfinite(x).all() and np.isfinite(rr).all()
    assert list(ranks) == [5, 17, 40, 0, k, k]
    for i, a in enumerate(mats):
        r = int(ranks[i])
        check_identities(a, c[i], x[i], rr[i], row_ind[i], col_ind[i], r, k, dtype)
        if r == 0:
            assert np.array_equal(row_ind[i], np.arange(m))
            assert not np.any(c[i]) and not np.any(x[i]) and not np.any(rr[i])
            continue
        if r < k:  # exact low rank: c x r reproduces A to the working precision
            err = np.linalg.norm(a - c[i][:, :r] @ x[i][:r, :r] @ rr[i][:r]) / np.linalg.norm(a)
            assert err <= 1e4 * np.finfo(real_of(dtype)).eps
        else:
            check_one(a, c[i], x[i], rr[i], row_ind[i], col_ind[i], r, k, dtype)


@pytest.mark.parametrize("dtype", [C64, C32])
def test_tolerance_between_two_singular_values(dtype):
    """A spectrum falling by 10x per singular value, with complex singular vectors: tol = 10^-4.5 cuts it between s_4 and s_5."""
    rng = np.random.default_rng(32)
    m, n, k = 90, 70, 40
    u = o.random_orthogonal_matrix((m, 10), rng, np.complex128)
    vh = o.random_orthogonal_matrix((10, n), rng, np.complex128)
    a = ((u * 10.0 ** -np.arange(10)) @ vh).astype(dtype)
    tol = 10 ** -4.5
    c, x, rr, row_ind, col_ind, ranks = two_sided(torch.from_numpy(a[None]).cuda(), k, tol)
    r = int(ranks[0])
    assert r == o.QR.compute_from(a).compress_qr_tolerance(tol).rank()
    assert 4 <= r <= 6
    check_one(a, c[0], x[0], rr[0], row_ind[0], col_ind[0], r, k, dtype)


# ---------------------------------------------------------------- 5. independence of position and neighbours
def test_bits_independent_of_position_and_neighbours():
    rng = np.random.default_rng(16)
    m, n, k = 64, 48, 16
    a = phased(rng, m, n, C64)
    alone, probe = batched_launch(lambda: two_sided(torch.from_numpy(a[None]).cuda(), k, 1e-6))
    big = torch.from_numpy(gaussian(rng, (2 * probe["slots"] + 37) * m, n, C64).reshape(-1, m, n)).cuda()  # slots: this shape's persistent grid
    big[5] *= 1e-3  # different neighbours, among them a tiny one
    for s in (len(big) // 2, len(big) - 1):
        b = big.clone()
        b[s] = torch.from_numpy(a)
        got, lab = batched_launch(lambda: two_sided(b, k, 1e-6))
        assert lab["count"] > 2 * lab["grid"]  # both positions are some workgroup's second or third matrix
        for u, v in zip(alone, got):
            assert np.array_equal(u[0], v[s])


# ---------------------------------------------------------------- 6. layouts
def _raw(a, k, tol, pad):
    """One raw c64 call with every output batch stride padded by `pad` elements; returns the outputs as [count, ...] arrays."""
    cnt, m, n = a.shape
    kk = min(k, m, n)
    dev = a.device
    cb, xb, rb = m * kk + pad, kk * kk + pad, kk * n + pad
    c, x, r = (torch.full((cnt, s), 7.0 + 3.0j, dtype=a.dtype, device=dev) for s in (cb, xb, rb))
    row_ind = torch.empty((cnt, m), dtype=torch.int64, device=dev)
    col_ind = torch.empty((cnt, n), dtype=torch.int64, device=dev)
    ranks = torch.empty(cnt, dtype=torch.int64, device=dev)
    ctx = _lib.default_context()
    ctx.check(_lib.lib().rc_two_sided_id_rank_batched_c64(
        ctx._h, _lib.rc_matrix(a.data_ptr(), m, n, a.stride(1), a.stride(2)), ctypes.c_int64(a.stride(0)), ctypes.c_int32(cnt), ctypes.c_int64(k),
        ctypes.c_double(tol), _lib.rc_matrix(c.data_ptr(), m, kk, kk, 1), ctypes.c_int64(cb), _lib.rc_matrix(x.data_ptr(), kk, kk, kk, 1),
        ctypes.c_int64(xb), _lib.rc_matrix(r.data_ptr(), kk, n, n, 1), ctypes.c_int64(rb), _lib.i64p(row_ind), _lib.i64p(col_ind), _lib.i64p(ranks)))
    torch.cuda.synchronize()
    c, x, r = npy(c), npy(x), npy(r)
    assert (c[:, m * kk:] == 7.0 + 3.0j).all() and (x[:, kk * kk:] == 7.0 + 3.0j).all() and (r[:, kk * n:] == 7.0 + 3.0j).all()  # padding untouched
    return (c[:, :m * kk].reshape(cnt, m, kk), x[:, :kk * kk].reshape(cnt, kk, kk), r[:, :kk * n].reshape(cnt, kk, n), npy(row_ind), npy(col_ind),
            npy(ranks))


@pytest.mark.parametrize("dtype,m,n", [(C64, 70, 50), (C64, 140, 100), (C32, 70, 50)])
def test_layouts_give_the_same_bits(dtype, m, n):
    rng = np.random.default_rng(17)
    cnt, k = 9, 20
    base = torch.from_numpy(gaussian(rng, cnt * m, n, dtype).reshape(cnt, m, n)).cuda()
    ref = two_sided(base.contiguous(), k)
    transposed = base.transpose(1, 2).contiguous().transpose(1, 2)      # every matrix column-major
    padded = torch.zeros((cnt, m + 3, n + 5), dtype=base.dtype, device=base.device)
    padded[:, :m, :n] = base
    last = base.permute(1, 2, 0).contiguous().permute(2, 0, 1)          # a [m, n, count] array
    for view in (transposed, padded[:, :m, :n], last):
        got = two_sided(view, k)
        for u, v in zip(ref, got):
            assert np.array_equal(u, v)
    if dtype == C64:
        for u, v in zip(ref, _raw(base, k, 0.0, 13)):                   # padded output batch strides
            assert np.array_equal(u, v)
    same = base[2:3].expand(6, m, n)  # a_batch_stride = 0: count identical results
    assert same.stride(0) == 0
    got = two_sided(same, k)
    for u, v in zip(ref, got):
        for i in range(6):
            assert np.array_equal(v[i], u[2])


# ---------------------------------------------------------------- 7. graph capture
def test_graph_capture_replays_the_eager_bits():
    rng = np.random.default_rng(18)
    cnt, m, n, k = 33, 128, 96, 24
    lib = _lib.lib()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        a = torch.from_numpy(gaussian(rng, cnt * m, n, C64).reshape(cnt, m, n)).cuda()
        eager = two_sided(a, k, 1e-9)
        ctx = _lib.Context(torch.cuda.current_device(), st.cuda_stream)
        c = torch.zeros((cnt, m, k), dtype=a.dtype, device=a.device)
        x = torch.zeros((cnt, k, k), dtype=a.dtype, device=a.device)
        r = torch.zeros((cnt, k, n), dtype=a.dtype, device=a.device)
        row_ind = torch.zeros((cnt, m), dtype=torch.int64, device=a.device)
        col_ind = torch.zeros((cnt, n), dtype=torch.int64, device=a.device)
        ranks = torch.zeros(cnt, dtype=torch.int64, device=a.device)
        outs = (c, x, r, row_ind, col_ind, ranks)
        st.synchronize()
        args = (_lib.rc_matrix(a.data_ptr(), m, n, a.stride(1), a.stride(2)), ctypes.c_int64(a.stride(0)), ctypes.c_int32(cnt), ctypes.c_int64(k),
                ctypes.c_double(1e-9), _lib.mat(c[0]), ctypes.c_int64(m * k), _lib.mat(x[0]), ctypes.c_int64(k * k), _lib.mat(r[0]), ctypes.c_int64(k * n),
                _lib.i64p(row_ind), _lib.i64p(col_ind), _lib.i64p(ranks))
        ctx.check(lib.rc_two_sided_id_rank_batched_c64(ctx._h, *args))  # eager once: sizes the workspace
        ctx.synchronize()
        ctx.get_health()
        for t in outs:
            t.zero_()
        st.synchronize()
        graph = ctypes.c_void_p(None)
        ctx.check(lib.rc_graph_begin_capture(ctx._h))
        ctx.check(lib.rc_two_sided_id_rank_batched_c64(ctx._h, *args))
        ctx.check(lib.rc_graph_end_capture(ctx._h, ctypes.byref(graph)))
        try:
            ctx.check(lib.rc_graph_launch(ctx._h, graph))
            ctx.synchronize()
            for u, v in zip(eager, outs):
                assert np.array_equal(u, npy(v))
            assert ctx.get_health() == 0
        finally:
            ctx.check(lib.rc_graph_destroy(ctx._h, graph))
            ctx.close()


# ---------------------------------------------------------------- 8. conjugation symmetry
@pytest.mark.parametrize("dtype,m,n,k,tol", [(C64, 64, 48, 16, 0.0), (C64, 200, 160, 60, 1e-7), (C32, 128, 128, 64, 1e-4), (C32, 300, 90, 40, 0.0)])
def test_conjugate_input_gives_conjugate_factors(dtype, m, n, k, tol):
    """conj(A) gives the same permutations and ranks and the elementwise conjugate of c, x and r, bit for bit: a misplaced
    conjugate on the row side (C^T instead of C^H, Z2^T instead of Z2^H) breaks it."""
    rng = np.random.default_rng(m + n + k + 1)
    mats = np.stack([phased(rng, m, n, dtype), gaussian(rng, m, n, dtype), decaying(rng, m, n, dtype, 1e-6)])
    c, x, rr, row_ind, col_ind, ranks = two_sided(torch.from_numpy(mats).cuda(), k, tol)
    cc, xc, rc_, row_c, col_c, ranks_c = two_sided(torch.from_numpy(np.conj(mats)).cuda(), k, tol)
    assert np.array_equal(row_ind, row_c) and np.array_equal(col_ind, col_c) and np.array_equal(ranks, ranks_c)
    assert np.array_equal(np.conj(c), cc) and np.array_equal(np.conj(x), xc) and np.array_equal(np.conj(rr), rc_)


# ---------------------------------------------------------------- 9. arguments
def _call(a, cnt, k, tol, c, cbs, x, xbs, r, rbs, null=None, dtype=torch.complex128):
    """One raw call; a, c, x and r are [2, rows, cols] buffers so that even a call the checks let through stays inside them.
    null names one output pointer to pass as NULL."""
    ctx = _lib.default_context()
    row_ind = torch.empty((2, a.shape[1]), dtype=torch.int64, device="cuda")
    col_ind = torch.empty((2, a.shape[2]), dtype=torch.int64, device="cuda")
    ranks = torch.empty(2, dtype=torch.int64, device="cuda")
    ptr = lambda name, t: _lib.i64p(None) if null == name else _lib.i64p(t)  # noqa: E731
    mat = lambda name, t: _lib.rc_matrix(None, t.shape[1], t.shape[2], t.stride(1), t.stride(2)) if null == name else _lib.mat(t[0])  # noqa: E731
    fn = getattr(_lib.lib(), f"rc_two_sided_id_rank_batched_{_lib.suffix(dtype)}")
    return fn(ctx._h, mat("a", a), ctypes.c_int64(a.stride(0)), ctypes.c_int32(cnt), ctypes.c_int64(k), ctypes.c_double(tol), mat("c", c), ctypes.c_int64(cbs),
              mat("x", x), ctypes.c_int64(xbs), mat("r", r), ctypes.c_int64(rbs), ptr("row_ind", row_ind), ptr("col_ind", col_ind), ptr("ranks", ranks))


@pytest.mark.parametrize("dtype", [torch.complex128, torch.complex64])
def test_argument_checks(dtype):
    e = lambda r, c: torch.zeros((2, r, c), dtype=dtype, device="cuda")  # noqa: E731
    call = lambda *args, **kw: _call(*args, dtype=dtype, **kw)  # noqa: E731
    INVALID = 5
    assert call(e(520, 130), 2, 8, 0.0, e(520, 8), 520 * 8, e(8, 8), 64, e(8, 130), 8 * 130) == INVALID         # m > 512
    assert call(e(130, 520), 2, 8, 0.0, e(130, 8), 130 * 8, e(8, 8), 64, e(8, 520), 8 * 520) == INVALID         # n > 512
    a = e(200, 150)
    ok = lambda k: (e(200, k), 200 * k, e(k, k), k * k, e(k, 150), k * 150)  # noqa: E731
    assert call(a, 2, 16, 0.0, *ok(16)) == 0                                                                 # the baseline passes
    assert call(a, 2, 129, 0.0, *ok(129)) == INVALID                                                         # k > 128
    assert call(a, 2, 0, 0.0, *ok(1)) == INVALID                                                             # k < 1
    assert call(a, 2, 16, 1.0, *ok(16)) == INVALID                                                           # tol >= 1
    assert call(a, 2, 16, -1e-3, *ok(16)) == INVALID                                                         # tol < 0
    assert call(a, -1, 16, 0.0, *ok(16)) == INVALID                                                          # count < 0
    assert call(a, 2, 16, 0.0, e(200, 16), 200 * 16 - 1, e(16, 16), 256, e(16, 150), 16 * 150) == INVALID    # C of two matrices overlap
    assert call(a, 2, 16, 0.0, e(200, 16), 200 * 16, e(16, 16), 255, e(16, 150), 16 * 150) == INVALID        # X of two matrices overlap
    assert call(a, 2, 16, 0.0, e(200, 16), 200 * 16, e(16, 16), 256, e(16, 150), 15 * 150) == INVALID        # R of two matrices overlap
    assert call(a, 2, 16, 0.0, e(200, 15), 200 * 15, e(16, 16), 256, e(16, 150), 16 * 150) == INVALID        # wrong C shape
    assert call(a, 2, 16, 0.0, e(200, 16), 200 * 16, e(16, 15), 256, e(16, 150), 16 * 150) == INVALID        # wrong X shape
    assert call(a, 2, 16, 0.0, e(200, 16), 200 * 16, e(16, 16), 256, e(16, 149), 16 * 149) == INVALID        # wrong R shape
    msg = _lib.lib().rc_last_error_message(_lib.default_context()._h).decode()
    assert "two_sided_id_rank_batched: c must be 200 x 16, x 16 x 16 and r 16 x 150" in msg
    for name in ("a", "c", "x", "r", "row_ind", "col_ind", "ranks"):
        assert call(a, 2, 16, 0.0, *ok(16), null=name) == INVALID, name                                     # null pointer
    assert call(a, 0, 16, 0.0, *ok(16)) == 0                                                                 # count = 0: nothing to do
    with pytest.raises(AssertionError, match="two_sided_id_rank_batched"):  # RC_INVALID_ARGUMENT: the reference asserts
        rc.two_sided_id_rank_batched(torch.zeros((1, 600, 10), dtype=dtype, device="cuda"), 4)
    out = rc.two_sided_id_rank_batched(torch.zeros((0, 30, 20), dtype=dtype, device="cuda"), 8)
    assert [tuple(t.shape) for t in out] == [(0, 30, 8), (0, 8, 8), (0, 8, 20), (0, 30), (0, 20), (0,)]


# ---------------------------------------------------------------- 10. containment of non-finite input
@pytest.mark.parametrize("dtype", [C64, C32])
def test_nan_stays_in_its_matrix(dtype):
    rng = np.random.default_rng(19)
    cnt, m, n, k = 12, 90, 70, 30
    clean = torch.from_numpy(gaussian(rng, cnt * m, n, dtype).reshape(cnt, m, n)).cuda()
    ref = two_sided(clean, k, 1e-5)
    bad = clean.clone()
    bad[4, :, 23] = complex(float("nan"), 1.0)
    bad[8, :, 5] = complex(0.0, float("inf"))
    got = two_sided(bad, k, 1e-5)
    for i in range(cnt):
        assert is_permutation(got[3][i], m) and is_permutation(got[4][i], n) and 0 <= got[5][i] <= k
        if i in (4, 8):
            continue
        for u, v in zip(ref, got):
            assert np.array_equal(u[i], v[i])
