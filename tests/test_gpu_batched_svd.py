"""Batched truncated SVD of many small same-shaped matrices (rc_svd_rank_batched_*, batch.svd_rank_batched).

Per matrix the reference sequence SVD::compute_from(a) -> compress(.) (src/compute_svd.rs:18-27, src/svd.rs:60-101), checked
against the SciPy-LAPACK oracle, the committed qrcp_* golden vectors and the lone call rc_compute_svd_*; plus the contract of the
batch itself (sign convention, independence of the neighbours, layouts, graph capture, health word, argument checks, containment of
non-finite input)."""
import ctypes

import numpy as np
import pytest
import torch

import rusty_compression_amd as rc
from oracle import ref_lapack as o
from rusty_compression_amd import _lib
from tests.helpers import TOL, batched_launch, golden, npy, sign_normalise

pytestmark = pytest.mark.gpu

GAP = {np.dtype(np.float64): 1e-3, np.dtype(np.float32): 1e-2}
INVALID = 5


def batched(a, k, tol=0.0):
    u, s, vt, ranks = rc.svd_rank_batched(a, k, tol)
    torch.cuda.synchronize()
    return npy(u), npy(s), npy(vt), npy(ranks)


def decaying(rng, m, n, dtype, lo=1e-10):
    return o.random_approximate_low_rank_matrix((m, n), 1.0, lo, rng).astype(dtype)


def with_spectrum(rng, m, n, s, dtype):
    """Q1 diag(s) Q2^T with Haar-random orthonormal factors (p = len(s) = min(m, n))."""
    q1, _ = np.linalg.qr(rng.standard_normal((m, len(s))))
    q2, _ = np.linalg.qr(rng.standard_normal((n, len(s))))
    return ((q1 * np.asarray(s)) @ q2.T).astype(dtype)


def gaps(s):
    """Distance of each singular value to its nearest other one, relative to s_0."""
    s = np.asarray(s, dtype=np.float64)
    d = np.full(len(s), np.inf)
    if len(s) > 1:
        diff = np.abs(np.diff(s))
        d[:-1] = np.minimum(d[:-1], diff)
        d[1:] = np.minimum(d[1:], diff)
    return d / max(s[0], np.finfo(np.float64).tiny)


def check_signs(u, vt, r):
    """The contract's sign rule on the kept columns: the first largest-|.| entry of u[:, j] is positive."""
    for j in range(r):
        i = int(np.argmax(np.abs(u[:, j])))
        assert u[i, j] > 0, (j, i, u[i, j])
    nu, nvt = sign_normalise(u[:, :r], vt[:r])
    assert np.array_equal(nu, u[:, :r]) and np.array_equal(nvt, vt[:r])


def check_vectors(u, vt, gu, gvt, s_ref, r, dtype):
    """Kept triplets with a gap >= GAP against reference vectors (sign-normalised), to 200 eps / min(gap, 1)."""
    eps = np.finfo(dtype).eps
    g = gaps(s_ref)
    gu, gvt = sign_normalise(gu[:, :r], gvt[:r])
    checked = 0
    for j in range(r):
        if g[j] < GAP[np.dtype(dtype)]:
            continue
        top = np.sort(np.abs(gu[:, j]))[::-1]
        if len(top) > 1 and top[0] - top[1] < 1e-2 * top[0]:  # two entries of almost the same size: the sign rule is fragile
            continue
        bound = 200 * eps / min(g[j], 1.0)
        assert np.abs(u[:, j] - gu[:, j]).max() <= bound, (j, np.abs(u[:, j] - gu[:, j]).max(), bound)
        assert np.abs(vt[j] - gvt[j]).max() <= bound, (j, np.abs(vt[j] - gvt[j]).max(), bound)
        checked += 1
    return checked


def check_one(a, u, s, vt, r, k, dtype):
    """One matrix against the f64 oracle: all p singular values, orthonormality, the truncation error, zero tails, signs."""
    m, n = a.shape
    t = TOL[np.dtype(dtype)]
    ref = o.SVD.compute_from(a.astype(np.float64))
    assert s.shape == (min(m, n),)
    assert np.all(np.diff(s.astype(np.float64)) <= 0), "singular values not descending"
    s0 = max(ref.s[0], np.finfo(np.float64).tiny)
    assert np.abs(s.astype(np.float64) - ref.s).max() <= t["sval"] * s0
    assert not np.any(u[:, r:]) and not np.any(vt[r:])
    if r == 0:
        return ref
    ur, vr = u[:, :r].astype(np.float64), vt[:r].astype(np.float64)
    assert np.abs(ur.T @ ur - np.eye(r)).max() <= t["orth"] * 4
    assert np.abs(vr @ vr.T - np.eye(r)).max() <= t["orth"] * 4
    err = np.linalg.norm(a.astype(np.float64) - (ur * s[:r].astype(np.float64)) @ vr, 2)
    tail = ref.s[r] if r < len(ref.s) else 0.0
    assert abs(err - tail) <= t["recon"] * s0 * 4, (err, tail)
    check_signs(u, vt, r)
    return ref


# ---------------------------------------------------------------- 1. goldens inside a batch of strangers
GOLDENS = [f"qrcp_{d}_{shape}_{s}.npz" for d in ("f64", "f32") for shape in ("thin", "thick") for s in ("s5", "s10")]


@pytest.mark.parametrize("name", GOLDENS)
def test_goldens_at_several_positions(name):
    g = golden(name)
    a0 = g["a"]
    dtype = a0.dtype
    t = TOL[np.dtype(dtype)]
    m, n = a0.shape
    p = min(m, n)
    rng = np.random.default_rng(1)
    batch = rng.standard_normal((7, m, n)).astype(dtype)
    slots = (0, 3, 6)
    for sl in slots:
        batch[sl] = a0
    u, s, vt, ranks = batched(torch.from_numpy(batch).cuda(), p)
    for sl in slots:
        assert ranks[sl] == p
        assert np.abs(s[sl].astype(np.float64) - g["s"]).max() <= t["sval"] * g["s"][0]
        rec = (u[sl].astype(np.float64) * s[sl].astype(np.float64)) @ vt[sl].astype(np.float64)
        assert np.linalg.norm(rec - a0) / np.linalg.norm(a0) <= t["recon"] * 4
        assert check_vectors(u[sl], vt[sl], g["u"], g["vt"], g["s"], p, dtype) >= 3
        check_signs(u[sl], vt[sl], p)
        for x, y in zip((u, s, vt), (u, s, vt)):
            assert np.array_equal(x[sl], y[slots[0]])


# ---------------------------------------------------------------- 2. oracle parity across shapes
SHAPES = [(1, 1), (1, 7), (7, 1), (33, 17), (64, 64), (128, 128), (200, 96), (512, 128), (128, 512)]


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("m,n", SHAPES)
def test_oracle_parity_across_shapes(m, n, dtype):
    rng = np.random.default_rng(m * 1000 + n)
    p = min(m, n)
    mats = [rng.standard_normal((m, n)).astype(dtype), decaying(rng, m, n, dtype, 1e-6), decaying(rng, m, n, dtype, 1e-3)]
    a = torch.from_numpy(np.stack(mats)).cuda()
    for k in sorted({1, max(1, p // 3), p, 128}):
        u, s, vt, ranks = batched(a, k)
        kk = min(k, p)
        assert u.shape == (3, m, kk) and s.shape == (3, p) and vt.shape == (3, kk, n)
        for i, x in enumerate(mats):
            assert ranks[i] == kk
            ref = check_one(x, u[i], s[i], vt[i], kk, kk, dtype)
            check_vectors(u[i], vt[i], ref.u, ref.vt, ref.s, kk, dtype)


# ---------------------------------------------------------------- 3. rank rule
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_rank_rule_matches_compress_svd_tolerance(dtype):
    rng = np.random.default_rng(3)
    m, n = 90, 60
    # s_j = 10^(-j / 2): every ratio s_j / s_0 is at least a factor 10^(1/4) away from the tolerances below
    spec = 10.0 ** (-0.5 * np.arange(n))
    if dtype == np.float32:
        spec = np.maximum(spec, 1e-6)
    mats = [with_spectrum(rng, m, n, spec, dtype) for _ in range(3)]
    a = torch.from_numpy(np.stack(mats)).cuda()
    for tol in (10.0 ** -1.25, 10.0 ** -3.75, 10.0 ** -5.25):
        for k in (4, 40):
            u, s, vt, ranks = batched(a, k, tol)
            for i, x in enumerate(mats):
                full = o.SVD.compute_from(x.astype(np.float64))
                try:
                    want = min(full.compress_svd_tolerance(tol).rank(), k)
                except o.CompressionError:
                    want = k
                assert ranks[i] == want, (tol, k, ranks[i], want)
                check_one(x, u[i], s[i], vt[i], int(ranks[i]), k, dtype)


@pytest.mark.parametrize("dtype,tol", [(np.float64, 1e-8), (np.float32, 1e-4)])
def test_rank_rule_edges(dtype, tol):
    rng = np.random.default_rng(4)
    m, n, k = 70, 50, 20
    rank5 = (rng.standard_normal((m, 5)) @ rng.standard_normal((5, n))).astype(dtype)
    zero = np.zeros((m, n), dtype=dtype)
    well = with_spectrum(rng, m, n, np.linspace(1.0, 0.5, n), dtype)  # no singular value crosses tol
    a = torch.from_numpy(np.stack([rank5, zero, well])).cuda()
    u, s, vt, ranks = batched(a, k, tol)
    assert list(ranks) == [5, 0, k]
    assert not np.any(u[1]) and not np.any(vt[1]) and not np.any(s[1])
    check_one(rank5, u[0], s[0], vt[0], 5, k, dtype)
    check_one(well, u[2], s[2], vt[2], k, k, dtype)
    # tol = 0: fixed rank k, whatever the spectrum (the rank-5 matrix's tail is rounding noise, but not exactly zero)
    u0, s0, vt0, r0 = batched(a[[0, 2]], k, 0.0)
    assert list(r0) == [k, k]
    check_one(well, u0[1], s0[1], vt0[1], k, k, dtype)


# ---------------------------------------------------------------- 4. the bit contract
def test_bits_independent_of_position_neighbours_and_count():
    rng = np.random.default_rng(5)
    m, n, k = 64, 48, 16
    x = decaying(rng, m, n, np.float64)
    alone, probe = batched_launch(lambda: batched(torch.from_numpy(x[None]).cuda(), k, 1e-6))
    big = torch.from_numpy(rng.standard_normal((2 * probe["slots"] + 37, m, n))).cuda()  # slots: the persistent grid of this shape
    big[5] *= 1e-3  # different neighbours, among them a tiny one
    for sl in (len(big) // 2, len(big) - 1):
        b = big.clone()
        b[sl] = torch.from_numpy(x)
        got, lab = batched_launch(lambda: batched(b, k, 1e-6))
        assert lab["count"] > 2 * lab["grid"]  # both positions are some workgroup's second or third matrix
        for v, w in zip(alone, got):
            assert np.array_equal(v[0], w[sl])


@pytest.mark.parametrize("m,n", [(70, 50), (50, 70), (128, 128)])
def test_layouts_give_the_same_bits(m, n):
    rng = np.random.default_rng(6)
    cnt, k = 5, 20
    base = torch.from_numpy(rng.standard_normal((cnt, m, n))).cuda()
    ref = batched(base.contiguous(), k)
    colmajor = base.transpose(1, 2).contiguous().transpose(1, 2)
    padded = torch.zeros((cnt, m + 3, n + 5), dtype=base.dtype, device=base.device)
    padded[:, :m, :n] = base
    last = base.permute(1, 2, 0).contiguous().permute(2, 0, 1)  # a [m, n, count] array
    for view in (colmajor, padded[:, :m, :n], last):
        got = batched(view, k)
        for v, w in zip(ref, got):
            assert np.array_equal(v, w)
    same = base[2:3].expand(4, m, n)  # a_batch_stride = 0
    assert same.stride(0) == 0
    got = batched(same, k)
    for v, w in zip(ref, got):
        for i in range(4):
            assert np.array_equal(w[i], v[2])
    if m == n:
        return
    # the transposed matrix of a non-square one has the same work orientation: the singular values bit for bit, u and vt swapped
    # up to the sign rule
    ut, st, vtt, rt = batched(base.transpose(1, 2), k)
    assert np.array_equal(st, ref[1]) and np.array_equal(rt, ref[3])
    assert np.array_equal(np.abs(ut), np.abs(ref[2].transpose(0, 2, 1))) and np.array_equal(np.abs(vtt), np.abs(ref[0].transpose(0, 2, 1)))


def _raw(a, cnt, k, tol, u, ubs, s, vt, vbs, ranks, dtype=torch.float64, ctx=None):
    ctx = ctx or _lib.default_context()
    fn = getattr(_lib.lib(), f"rc_svd_rank_batched_{_lib.suffix(dtype)}")
    return fn(ctx._h, _lib.rc_matrix(a.data_ptr(), a.shape[1], a.shape[2], a.stride(1), a.stride(2)), ctypes.c_int64(a.stride(0)), ctypes.c_int32(cnt),
              ctypes.c_int64(k), ctypes.c_double(tol), u, ctypes.c_int64(ubs), ctypes.c_void_p(s.data_ptr()), vt, ctypes.c_int64(vbs),
              _lib.i64p(ranks))


def test_output_strides_give_the_same_bits():
    rng = np.random.default_rng(7)
    cnt, m, n, k = 6, 90, 40, 12
    a = torch.from_numpy(rng.standard_normal((cnt, m, n))).cuda()
    ref = batched(a, k, 1e-3)
    ut = torch.zeros((cnt, k, m + 1), dtype=a.dtype, device=a.device)   # u column-major, padded
    vtt = torch.zeros((cnt, n, k), dtype=a.dtype, device=a.device)      # vt column-major
    s = torch.zeros((cnt, n), dtype=a.dtype, device=a.device)
    ranks = torch.zeros(cnt, dtype=torch.int64, device=a.device)
    uv = _lib.rc_matrix(ut.data_ptr(), m, k, 1, m + 1)
    vv = _lib.rc_matrix(vtt.data_ptr(), k, n, 1, k)
    assert _raw(a, cnt, k, 1e-3, uv, k * (m + 1), s, vv, n * k, ranks) == 0
    torch.cuda.synchronize()
    assert np.array_equal(npy(ut)[:, :, :m].transpose(0, 2, 1), ref[0])
    assert np.array_equal(npy(vtt).transpose(0, 2, 1), ref[2])
    assert np.array_equal(npy(s), ref[1]) and np.array_equal(npy(ranks), ref[3])


def test_graph_capture_replays_the_eager_bits():
    rng = np.random.default_rng(8)
    cnt, m, n, k = 33, 96, 128, 24
    lib = _lib.lib()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        a = torch.from_numpy(rng.standard_normal((cnt, m, n))).cuda()
        eager = batched(a, k, 1e-9)
        ctx = _lib.Context(torch.cuda.current_device(), st.cuda_stream)
        u = torch.zeros((cnt, m, k), dtype=a.dtype, device=a.device)
        s = torch.zeros((cnt, m), dtype=a.dtype, device=a.device)
        vt = torch.zeros((cnt, k, n), dtype=a.dtype, device=a.device)
        ranks = torch.zeros(cnt, dtype=torch.int64, device=a.device)
        st.synchronize()
        args = (a, cnt, k, 1e-9, _lib.mat(u[0]), m * k, s, _lib.mat(vt[0]), k * n, ranks)
        assert _raw(*args, ctx=ctx) == 0  # eager once: sizes the workspace
        ctx.synchronize()
        ctx.get_health()
        for t in (u, s, vt, ranks):
            t.zero_()
        st.synchronize()
        graph = ctypes.c_void_p(None)
        ctx.check(lib.rc_graph_begin_capture(ctx._h))
        assert _raw(*args, ctx=ctx) == 0
        ctx.check(lib.rc_graph_end_capture(ctx._h, ctypes.byref(graph)))
        try:
            ctx.check(lib.rc_graph_launch(ctx._h, graph))
            ctx.synchronize()
            for v, w in zip(eager, (u, s, vt, ranks)):
                assert np.array_equal(v, npy(w))
            assert ctx.get_health() == 0
        finally:
            ctx.check(lib.rc_graph_destroy(ctx._h, graph))
            ctx.close()


# ---------------------------------------------------------------- 5. agreement with the lone call
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_agrees_with_the_lone_call(dtype):
    rng = np.random.default_rng(9)
    m, n, k, tol = 150, 100, 80, 2.5e-4  # tol is 6 % away from the nearest ratio s_j / s_0 of the decaying spectra
    t = TOL[np.dtype(dtype)]
    mats = [decaying(rng, m, n, dtype, 1e-6) for _ in range(2)] + [rng.standard_normal((m, n)).astype(dtype)]
    u, s, vt, ranks = batched(torch.from_numpy(np.stack(mats)).cuda(), k, tol)
    for i, x in enumerate(mats):
        lone = rc.SVD.compute_from(torch.from_numpy(x).cuda())
        ls = npy(lone.s)
        assert np.abs(s[i] - ls).max() <= t["sval"] * ls[0] * 4
        comp = lone.compress_svd_tolerance(tol) if ls[-1] / ls[0] < tol else lone.compress_svd_rank(k)
        r = min(comp.rank(), k)
        assert ranks[i] == r
        lu, lvt = sign_normalise(npy(comp.u)[:, :r], npy(comp.vt)[:r])
        check_vectors(u[i], vt[i], lu, lvt, ls, r, dtype)
        rec = (u[i][:, :r].astype(np.float64) * s[i][:r]) @ vt[i][:r].astype(np.float64)
        lrec = (lu.astype(np.float64) * ls[:r]) @ lvt.astype(np.float64)
        assert np.linalg.norm(rec - lrec) / np.linalg.norm(lrec) <= (1e-8 if dtype == np.float64 else 1e-3)


# ---------------------------------------------------------------- 6. health
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_clean_inputs_leave_the_health_word_clear(dtype):
    rng = np.random.default_rng(10)
    ctx = _lib.default_context()
    ctx.synchronize()
    ctx.get_health()
    m, n, k = 128, 128, 64
    clustered = np.concatenate([np.ones(10), 0.5 * np.ones(40), 1e-3 * (1 + 1e-9 * np.arange(78))])
    mats = [with_spectrum(rng, m, n, clustered, dtype), with_spectrum(rng, m, n, np.ones(n), dtype), decaying(rng, m, n, dtype),
            rng.standard_normal((m, n)).astype(dtype)]
    u, s, vt, ranks = batched(torch.from_numpy(np.stack(mats)).cuda(), k)
    ctx.synchronize()
    assert ctx.get_health() == 0
    for i, x in enumerate(mats):
        check_one(x, u[i], s[i], vt[i], k, k, dtype)


# ---------------------------------------------------------------- 7. containment of non-finite input
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_nan_stays_in_its_matrix(dtype):
    rng = np.random.default_rng(11)
    cnt, m, n, k = 12, 90, 70, 30
    clean = torch.from_numpy(rng.standard_normal((cnt, m, n))).to(dtype).cuda()
    ref = batched(clean, k, 1e-5)
    bad = clean.clone()
    bad[4, 17, 23] = float("nan")
    bad[8, :, 5] = float("inf")
    got = batched(bad, k, 1e-5)
    for i in range(cnt):
        assert 0 <= got[3][i] <= k
        if i in (4, 8):
            continue
        for v, w in zip(ref, got):
            assert np.array_equal(v[i], w[i])
    _lib.default_context().get_health()  # whatever the bad matrices raised


# ---------------------------------------------------------------- 8. arguments
def test_argument_checks():
    e = lambda c, r, q: torch.zeros((c, r, q), dtype=torch.float64, device="cuda")  # noqa: E731
    sbuf = torch.zeros(2 * 600, dtype=torch.float64, device="cuda")
    ranks = torch.zeros(2, dtype=torch.int64, device="cuda")

    def call(a, k, tol, u, ubs, vt, vbs, cnt=2):
        return _raw(a, cnt, k, tol, _lib.mat(u[0]), ubs, sbuf, _lib.mat(vt[0]), vbs, ranks)

    assert call(e(2, 520, 100), 8, 0.0, e(2, 520, 8), 520 * 8, e(2, 8, 100), 800) == INVALID     # m > 512
    assert call(e(2, 100, 520), 8, 0.0, e(2, 100, 8), 800, e(2, 8, 520), 8 * 520) == INVALID     # n > 512
    assert call(e(2, 200, 130), 8, 0.0, e(2, 200, 8), 1600, e(2, 8, 130), 8 * 130) == INVALID    # min(m, n) > 128
    a = e(2, 200, 100)
    assert call(a, 129, 0.0, e(2, 200, 100), 20000, e(2, 100, 100), 10000) == INVALID             # k > 128
    assert call(a, 0, 0.0, e(2, 200, 1), 200, e(2, 1, 100), 100) == INVALID                       # k < 1
    assert call(a, 16, 1.0, e(2, 200, 16), 3200, e(2, 16, 100), 1600) == INVALID                  # tol >= 1
    assert call(a, 16, -1e-3, e(2, 200, 16), 3200, e(2, 16, 100), 1600) == INVALID                # tol < 0
    assert call(a, 16, 0.0, e(2, 200, 16), 3199, e(2, 16, 100), 1600) == INVALID                  # u of two matrices overlap
    assert call(a, 16, 0.0, e(2, 200, 16), 3200, e(2, 16, 100), 1599) == INVALID                  # vt of two matrices overlap
    assert call(a, 16, 0.0, e(2, 200, 15), 3000, e(2, 16, 100), 1600) == INVALID                  # wrong u shape
    assert call(a, 16, 0.0, e(2, 200, 16), 3200, e(2, 16, 99), 1584) == INVALID                   # wrong vt shape
    msg = _lib.lib().rc_last_error_message(_lib.default_context()._h).decode()
    assert "vt" in msg
    assert _lib.lib().rc_svd_rank_batched_f64(_lib.default_context()._h, _lib.mat(a[0]), ctypes.c_int64(a.stride(0)), ctypes.c_int32(2),
                                              ctypes.c_int64(16), ctypes.c_double(0.0), _lib.mat(e(2, 200, 16)[0]), ctypes.c_int64(3200),
                                              ctypes.c_void_p(None), _lib.mat(e(2, 16, 100)[0]), ctypes.c_int64(1600),
                                              _lib.i64p(ranks)) == INVALID                         # null s
    assert call(a, 16, 0.0, e(2, 200, 16), 3200, e(2, 16, 100), 1600, cnt=0) == 0                 # count = 0: nothing to do
    with pytest.raises(AssertionError, match="rc_compute_svd_"):  # RC_INVALID_ARGUMENT: the reference asserts
        rc.svd_rank_batched(torch.zeros((1, 300, 200), dtype=torch.float64, device="cuda"), 4)
    u, s, vt, r = rc.svd_rank_batched(torch.zeros((0, 30, 20), dtype=torch.float32, device="cuda"), 8)
    assert u.shape == (0, 30, 8) and s.shape == (0, 20) and vt.shape == (0, 8, 20) and r.shape == (0,)
    with pytest.raises(TypeError):
        rc.svd_rank_batched(torch.zeros((1, 8, 8), dtype=torch.complex128, device="cuda"), 4)
