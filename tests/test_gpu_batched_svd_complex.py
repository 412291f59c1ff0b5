"""Batched truncated SVD of many small same-shaped complex matrices (rc_svd_rank_batched_c64 / _c32, batch.svd_rank_batched_complex).

Per matrix the reference sequence SVD::compute_from(a) -> compress(.) on complex data, checked against the SciPy-LAPACK oracle
(zgesdd / cgesdd), the committed qrcp_* golden vectors times column phases and the lone call rc_compute_svd_c*; plus the contract of
the batch itself (phase rule, independence of the neighbours, layouts, graph capture, conjugation symmetry, health word, argument
checks, containment of non-finite input)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import rusty_compression_amd as rc
from oracle import ref_lapack as o
from rusty_compression_amd import _lib
from tests.helpers import TOL, batched_launch, golden, npy

pytestmark = pytest.mark.gpu

C64, C32 = np.complex128, np.complex64
GAP = {np.dtype(np.float64): 1e-3, np.dtype(np.float32): 1e-2}
INVALID = 5


def real_of(dtype):
    """The real dtype of a complex one: the tolerances of tests/helpers.py are keyed by it."""
    return np.dtype(np.float64) if np.dtype(dtype) == np.dtype(C64) else np.dtype(np.float32)


def batched(a, k, tol=0.0):
    u, s, vt, ranks = rc.svd_rank_batched_complex(a, k, tol)
    torch.cuda.synchronize()
    return npy(u), npy(s), npy(vt), npy(ranks)


def gaussian(rng, m, n, dtype):
    return o.random_gaussian((m, n), rng, dtype)


def decaying(rng, m, n, dtype, lo=1e-10):
    """U diag(geomspace) V^H with complex orthonormal U, V."""
    return o.random_approximate_low_rank_matrix((m, n), 1.0, lo, rng, dtype)


def with_spectrum(rng, m, n, s, dtype):
    """Q1 diag(s) Q2^H with complex Haar-random orthonormal factors (p = len(s) = min(m, n))."""
    q1, _ = np.linalg.qr(gaussian(rng, m, len(s), C64))
    q2, _ = np.linalg.qr(gaussian(rng, n, len(s), C64))
    return ((q1 * np.asarray(s)) @ q2.conj().T).astype(dtype)


def gaps(s):
    """Distance of each singular value to its nearest other one, relative to s_0."""
    s = np.asarray(s, dtype=np.float64)
    d = np.full(len(s), np.inf)
    if len(s) > 1:
        diff = np.abs(np.diff(s))
        d[:-1] = np.minimum(d[:-1], diff)
        d[1:] = np.minimum(d[1:], diff)
    return d / max(s[0], np.finfo(np.float64).tiny)


def clear_top(col):
    """The two largest moduli of a column are more than 1e-2 apart (relative): the phase rule is then not fragile."""
    top = np.sort(np.abs(col))[::-1]
    return len(top) < 2 or top[0] - top[1] >= 1e-2 * top[0]


def check_phases(u, r):
    """The contract's phase rule on the kept columns: the first largest-modulus entry is real, imaginary part exactly 0, positive."""
    for j in range(r):
        if not clear_top(u[:, j]):
            continue
        i = int(np.argmax(np.abs(u[:, j])))
        assert u[i, j].imag == 0 and u[i, j].real > 0, (j, i, u[i, j])


def check_vectors(u, vt, gu, gvt, s_ref, r, dtype):
    """Kept triplets with a gap >= GAP against reference vectors up to a unit phase, to 200 eps / min(gap, 1)."""
    rd = real_of(dtype)
    eps = np.finfo(rd).eps
    g = gaps(s_ref)
    checked = 0
    for j in range(r):
        if g[j] < GAP[rd]:
            continue
        gj = np.asarray(gu[:, j], dtype=np.complex128)
        if not clear_top(gj):  # two entries of almost the same modulus: the phase rule is fragile
            continue
        i = int(np.argmax(np.abs(gj)))
        ph = np.conj(gj[i]) / abs(gj[i])  # the phase that the rule applies to the reference column
        bound = 200 * eps / min(g[j], 1.0)
        assert np.abs(u[:, j] - gj * ph).max() <= bound, (j, np.abs(u[:, j] - gj * ph).max(), bound)
        assert np.abs(vt[j] - np.asarray(gvt[j]) * np.conj(ph)).max() <= bound
        checked += 1
    return checked


def check_one(a, u, s, vt, r, dtype):
    """One matrix against the c128 oracle: all p singular values, orthonormality, the truncation error, zero tails, phases."""
    m, n = a.shape
    t = TOL[real_of(dtype)]
    ref = o.SVD.compute_from(a.astype(np.complex128))
    assert s.shape == (min(m, n),) and s.dtype == real_of(dtype)
    assert np.all(np.diff(s.astype(np.float64)) <= 0), "singular values not descending"
    s0 = max(ref.s[0], np.finfo(np.float64).tiny)
    assert np.abs(s.astype(np.float64) - ref.s).max() <= t["sval"] * s0 * 4
    assert not np.any(u[:, r:]) and not np.any(vt[r:])
    if r == 0:
        return ref
    ur, vr = u[:, :r].astype(np.complex128), vt[:r].astype(np.complex128)
    assert np.abs(ur.conj().T @ ur - np.eye(r)).max() <= t["orth"] * 4
    assert np.abs(vr @ vr.conj().T - np.eye(r)).max() <= t["orth"] * 4
    err = np.linalg.norm(a.astype(np.complex128) - (ur * s[:r].astype(np.float64)) @ vr, 2)
    tail = ref.s[r] if r < len(ref.s) else 0.0
    assert abs(err - tail) <= t["recon"] * s0 * 4, (err, tail)
    check_phases(u, r)
    return ref


# ---------------------------------------------------------------- 1. oracle parity across shapes
SHAPES = [((1, 1), C64), ((1, 7), C64), ((7, 1), C64), ((33, 17), C64), ((17, 33), C64), ((64, 64), C64), ((96, 96), C64),
          ((128, 128), C64), ((512, 128), C64), ((128, 512), C64), ((1, 1), C32), ((1, 7), C32), ((33, 17), C32), ((17, 33), C32),
          ((64, 64), C32), ((128, 128), C32), ((512, 128), C32), ((128, 512), C32)]


@pytest.mark.parametrize("shape,dtype", SHAPES)
def test_oracle_parity_across_shapes(shape, dtype):
    m, n = shape
    rng = np.random.default_rng(m * 1000 + n)
    p = min(m, n)
    lo = 1e-6 if dtype == C64 else 1e-4
    mats = [gaussian(rng, m, n, dtype), decaying(rng, m, n, dtype, lo), decaying(rng, m, n, dtype, 1e-3)]
    a = torch.from_numpy(np.stack(mats)).cuda()
    for k in sorted({1, max(1, p // 3), p}):
        u, s, vt, ranks = batched(a, k)
        kk = min(k, p)
        assert u.shape == (3, m, kk) and s.shape == (3, p) and vt.shape == (3, kk, n)
        for i, x in enumerate(mats):
            assert ranks[i] == kk
            ref = check_one(x, u[i], s[i], vt[i], kk, dtype)
            check_vectors(u[i], vt[i], ref.u, ref.vt, ref.s, kk, dtype)


# ---------------------------------------------------------------- 2. phased real goldens among strangers
GOLDENS = [f"qrcp_{d}_{shape}_{s}.npz" for d in ("f64", "f32") for shape in ("thin", "thick") for s in ("s5", "s10")]


@pytest.mark.parametrize("name", GOLDENS)
def test_phased_goldens_at_several_positions(name):
    g = golden(name)
    a0 = g["a"]
    dtype = C64 if a0.dtype == np.float64 else C32
    t = TOL[real_of(dtype)]
    m, n = a0.shape
    p = min(m, n)
    rng = np.random.default_rng(2)
    batch = np.stack([gaussian(rng, m, n, dtype) for _ in range(7)])
    slots = (0, 3, 6)
    for sl in slots:
        batch[sl] = (a0 * np.exp(2j * np.pi * rng.random(n))[None, :]).astype(dtype)  # unit-modulus column phases keep the spectrum
    u, s, vt, ranks = batched(torch.from_numpy(batch).cuda(), p)
    for sl in slots:
        assert ranks[sl] == p
        assert np.abs(s[sl].astype(np.float64) - g["s"]).max() <= t["sval"] * g["s"][0] * 4
        rec = (u[sl].astype(np.complex128) * s[sl].astype(np.float64)) @ vt[sl].astype(np.complex128)
        assert np.linalg.norm(rec - batch[sl]) / np.linalg.norm(batch[sl]) <= t["recon"] * 4
        check_phases(u[sl], p)


# ---------------------------------------------------------------- 3. rank rule
@pytest.mark.parametrize("dtype", [C64, C32])
def test_rank_rule_matches_compress_svd_tolerance(dtype):
    rng = np.random.default_rng(3)
    m, n = 90, 60
    spec = 10.0 ** (-0.5 * np.arange(n))  # every ratio s_j / s_0 is at least a factor 10^(1/4) away from the tolerances below
    if dtype == C32:
        spec = np.maximum(spec, 1e-6)
    mats = [with_spectrum(rng, m, n, spec, dtype) for _ in range(3)]
    a = torch.from_numpy(np.stack(mats)).cuda()
    for tol in (10.0 ** -1.25, 10.0 ** -3.75, 10.0 ** -5.25):
        for k in (4, 40):
            u, s, vt, ranks = batched(a, k, tol)
            for i, x in enumerate(mats):
                full = o.SVD.compute_from(x.astype(np.complex128))
                try:
                    want = min(full.compress_svd_tolerance(tol).rank(), k)
                except o.CompressionError:
                    want = k
                assert ranks[i] == want, (tol, k, ranks[i], want)
                check_one(x, u[i], s[i], vt[i], int(ranks[i]), dtype)


@pytest.mark.parametrize("dtype,tol", [(C64, 1e-8), (C32, 1e-4)])
def test_rank_rule_edges(dtype, tol):
    rng = np.random.default_rng(4)
    m, n, k = 70, 50, 20
    rank5 = (gaussian(rng, m, 5, C64) @ gaussian(rng, 5, n, C64)).astype(dtype)
    zero = np.zeros((m, n), dtype=dtype)
    well = with_spectrum(rng, m, n, np.linspace(1.0, 0.5, n), dtype)  # no singular value crosses tol
    a = torch.from_numpy(np.stack([rank5, zero, well])).cuda()
    u, s, vt, ranks = batched(a, k, tol)
    assert list(ranks) == [5, 0, k]
    assert not np.any(u[1]) and not np.any(vt[1]) and not np.any(s[1])
    check_one(rank5, u[0], s[0], vt[0], 5, dtype)
    check_one(well, u[2], s[2], vt[2], k, dtype)
    u0, s0, vt0, r0 = batched(a[[0, 2]], k, 0.0)  # tol = 0: fixed rank k
    assert list(r0) == [k, k]
    check_one(well, u0[1], s0[1], vt0[1], k, dtype)


# ---------------------------------------------------------------- 4. the bit contract
def test_bits_independent_of_position_neighbours_and_count():
    rng = np.random.default_rng(5)
    m, n, k = 64, 48, 16
    x = decaying(rng, m, n, C64)
    alone, probe = batched_launch(lambda: batched(torch.from_numpy(x[None]).cuda(), k, 1e-6))
    big = torch.from_numpy(np.stack([gaussian(rng, m, n, C64) for _ in range(2 * probe["slots"] + 37)])).cuda()  # slots: this shape's persistent grid
    big[5] *= 1e-3  # different neighbours, among them a tiny one
    for sl in (len(big) // 2, len(big) - 1):
        b = big.clone()
        b[sl] = torch.from_numpy(x)
        got, lab = batched_launch(lambda: batched(b, k, 1e-6))
        assert lab["count"] > 2 * lab["grid"]  # both positions are some workgroup's second or third matrix
        for v, w in zip(alone, got):
            assert np.array_equal(v[0], w[sl])


@pytest.mark.parametrize("m,n,dtype", [(70, 50, C64), (50, 70, C32), (128, 128, C64)])
def test_layouts_give_the_same_bits(m, n, dtype):
    rng = np.random.default_rng(6)
    cnt, k = 5, 20
    base = torch.from_numpy(np.stack([gaussian(rng, m, n, dtype) for _ in range(cnt)])).cuda()
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


def _raw(a, cnt, k, tol, u, ubs, s, vt, vbs, ranks, dtype=torch.complex128, ctx=None):
    ctx = ctx or _lib.default_context()
    fn = getattr(_lib.lib(), f"rc_svd_rank_batched_{_lib.suffix(dtype)}")
    return fn(ctx._h, _lib.rc_matrix(a.data_ptr(), a.shape[1], a.shape[2], a.stride(1), a.stride(2)), ctypes.c_int64(a.stride(0)), ctypes.c_int32(cnt),
              ctypes.c_int64(k), ctypes.c_double(tol), u, ctypes.c_int64(ubs), ctypes.c_void_p(s.data_ptr()), vt, ctypes.c_int64(vbs),
              _lib.i64p(ranks))


@pytest.mark.parametrize("m,n", [(90, 40), (40, 90)])
def test_output_strides_give_the_same_bits(m, n):
    rng = np.random.default_rng(7)
    cnt, k = 6, 12
    a = torch.from_numpy(np.stack([gaussian(rng, m, n, C64) for _ in range(cnt)])).cuda()
    ref = batched(a, k, 1e-3)
    ut = torch.zeros((cnt, k, m + 1), dtype=a.dtype, device=a.device)   # u column-major, padded
    vtt = torch.zeros((cnt, n, k), dtype=a.dtype, device=a.device)      # vt column-major
    s = torch.zeros((cnt, min(m, n)), dtype=torch.float64, device=a.device)
    ranks = torch.zeros(cnt, dtype=torch.int64, device=a.device)
    uv = _lib.rc_matrix(ut.data_ptr(), m, k, 1, m + 1)
    vv = _lib.rc_matrix(vtt.data_ptr(), k, n, 1, k)
    assert _raw(a, cnt, k, 1e-3, uv, k * (m + 1), s, vv, n * k, ranks) == 0
    torch.cuda.synchronize()
    assert np.array_equal(npy(ut)[:, :, :m].transpose(0, 2, 1), ref[0])
    assert np.array_equal(npy(vtt).transpose(0, 2, 1), ref[2])
    assert np.array_equal(npy(s), ref[1]) and np.array_equal(npy(ranks), ref[3])


# ---------------------------------------------------------------- 5. graph capture (the lone complex SVD refuses it)
@pytest.mark.parametrize("m,n", [(96, 128), (128, 128)])
def test_graph_capture_replays_the_eager_bits(m, n):
    rng = np.random.default_rng(8)
    cnt, k = 33, 24
    lib = _lib.lib()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        a = torch.from_numpy(np.stack([gaussian(rng, m, n, C64) for _ in range(cnt)])).cuda()
        eager = batched(a, k, 1e-9)
        ctx = _lib.Context(torch.cuda.current_device(), st.cuda_stream)
        u = torch.zeros((cnt, m, k), dtype=a.dtype, device=a.device)
        s = torch.zeros((cnt, min(m, n)), dtype=torch.float64, device=a.device)
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


# ---------------------------------------------------------------- 6. conjugation symmetry
@pytest.mark.parametrize("dtype", [C64, C32])
@pytest.mark.parametrize("m,n,k,tol", [(80, 48, 30, 1e-5), (48, 80, 30, 0.0), (128, 128, 64, 1e-8)])
def test_conjugate_input_gives_conjugate_factors(dtype, m, n, k, tol):
    """Every operation of the kernel commutes exactly with negating the imaginary parts: conj(A) gives the same s and ranks and
    the elementwise conjugate of u and vt, bit for bit (the phase entry's imaginary zero is compared as a value)."""
    rng = np.random.default_rng(9)
    mats = np.stack([decaying(rng, m, n, dtype, 1e-6), gaussian(rng, m, n, dtype)])
    u, s, vt, ranks = batched(torch.from_numpy(mats).cuda(), k, tol)
    uc, sc, vtc, ranksc = batched(torch.from_numpy(np.conj(mats)).cuda(), k, tol)
    assert np.array_equal(s, sc) and np.array_equal(ranks, ranksc)
    assert np.array_equal(np.conj(u), uc) and np.array_equal(np.conj(vt), vtc)
    lazy = batched(torch.conj(torch.from_numpy(mats).cuda()), k, tol)  # a lazily conjugated view reads as the conjugate
    for v, w in zip((uc, sc, vtc, ranksc), lazy):
        assert np.array_equal(v, w)


# ---------------------------------------------------------------- 7. agreement with the lone call and with the real batched call
@pytest.mark.parametrize("dtype", [C64, C32])
def test_agrees_with_the_lone_call(dtype):
    rng = np.random.default_rng(10)
    m, n, k = 60, 40, 40
    t = TOL[real_of(dtype)]
    mats = [decaying(rng, m, n, dtype, 1e-4), gaussian(rng, m, n, dtype)]
    u, s, vt, ranks = batched(torch.from_numpy(np.stack(mats)).cuda(), k)
    for i, x in enumerate(mats):
        lone = rc.SVD.compute_from(torch.from_numpy(x).cuda())
        lu, ls, lvt = npy(lone.u), npy(lone.s), npy(lone.vt)
        assert np.abs(s[i].astype(np.float64) - ls).max() <= t["sval"] * ls[0] * 4
        assert check_vectors(u[i], vt[i], lu, lvt, ls, k, dtype) >= 1


@pytest.mark.parametrize("dtype,real", [(C64, np.float64), (C32, np.float32)])
def test_real_valued_input_agrees_with_the_real_batched_call(dtype, real):
    rng = np.random.default_rng(11)
    m, n, k, tol = 90, 60, 40, 10.0 ** -3.75
    t = TOL[np.dtype(real)]
    spec = 10.0 ** (-0.5 * np.arange(n))
    q1, _ = np.linalg.qr(rng.standard_normal((m, n)))
    q2, _ = np.linalg.qr(rng.standard_normal((n, n)))
    x = ((q1 * spec) @ q2.T).astype(real)
    mats = np.stack([x, rng.standard_normal((m, n)).astype(real)])
    ur, sr, vtr, rr = (npy(v) for v in rc.svd_rank_batched(torch.from_numpy(mats).cuda(), k, tol))
    uc, sc, vtc, rcx = batched(torch.from_numpy(mats.astype(dtype)).cuda(), k, tol)
    assert np.abs(sc.astype(np.float64) - sr).max() <= t["sval"] * sr.max() * 4
    assert np.array_equal(rcx, rr)


# ---------------------------------------------------------------- 8. health
@pytest.mark.parametrize("dtype", [C64, C32])
def test_clean_inputs_leave_the_health_word_clear(dtype):
    rng = np.random.default_rng(12)
    ctx = _lib.default_context()
    ctx.synchronize()
    ctx.get_health()
    m, n, k = 128, 128, 64
    clustered = np.concatenate([np.ones(10), 0.5 * np.ones(40), 1e-3 * (1 + 1e-9 * np.arange(78))])
    mats = [with_spectrum(rng, m, n, clustered, dtype), with_spectrum(rng, m, n, np.ones(n), dtype), decaying(rng, m, n, dtype),
            gaussian(rng, m, n, dtype)]
    u, s, vt, ranks = batched(torch.from_numpy(np.stack(mats)).cuda(), k)
    ctx.synchronize()
    assert ctx.get_health() == 0
    for i, x in enumerate(mats):
        check_one(x, u[i], s[i], vt[i], k, dtype)


# ---------------------------------------------------------------- 9. containment of non-finite input
@pytest.mark.parametrize("dtype", [torch.complex128, torch.complex64])
def test_nan_stays_in_its_matrix(dtype):
    rng = np.random.default_rng(13)
    cnt, m, n, k = 12, 90, 70, 30
    clean = torch.from_numpy(np.stack([gaussian(rng, m, n, C64) for _ in range(cnt)])).to(dtype).cuda()
    ref = batched(clean, k, 1e-5)
    bad = clean.clone()
    bad[4, 17, 23] = complex(float("nan"), 0.0)
    bad[8, :, 5] = complex(0.0, float("inf"))
    got = batched(bad, k, 1e-5)
    for i in range(cnt):
        assert 0 <= got[3][i] <= k
        if i in (4, 8):
            continue
        for v, w in zip(ref, got):
            assert np.array_equal(v[i], w[i])
    _lib.default_context().get_health()  # whatever the bad matrices raised


# ---------------------------------------------------------------- 10. arguments
@pytest.mark.parametrize("dtype", [torch.complex128, torch.complex64])
def test_argument_checks(dtype):
    real = torch.float64 if dtype == torch.complex128 else torch.float32
    e = lambda c, r, q: torch.zeros((c, r, q), dtype=dtype, device="cuda")  # noqa: E731
    sbuf = torch.zeros(2 * 600, dtype=real, device="cuda")
    ranks = torch.zeros(2, dtype=torch.int64, device="cuda")

    def call(a, k, tol, u, ubs, vt, vbs, cnt=2):
        return _raw(a, cnt, k, tol, _lib.mat(u[0]), ubs, sbuf, _lib.mat(vt[0]), vbs, ranks, dtype=dtype)

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
    fn = getattr(_lib.lib(), f"rc_svd_rank_batched_{_lib.suffix(dtype)}")
    assert fn(_lib.default_context()._h, _lib.mat(a[0]), ctypes.c_int64(a.stride(0)), ctypes.c_int32(2), ctypes.c_int64(16), ctypes.c_double(0.0),
              _lib.mat(e(2, 200, 16)[0]), ctypes.c_int64(3200), ctypes.c_void_p(None), _lib.mat(e(2, 16, 100)[0]), ctypes.c_int64(1600),
              _lib.i64p(ranks)) == INVALID                                                         # null s
    assert call(a, 16, 0.0, e(2, 200, 16), 3200, e(2, 16, 100), 1600, cnt=0) == 0                 # count = 0: nothing to do
    with pytest.raises(AssertionError, match="rc_compute_svd_"):  # RC_INVALID_ARGUMENT: the reference asserts
        rc.svd_rank_batched_complex(torch.zeros((1, 300, 200), dtype=dtype, device="cuda"), 4)
    u, s, vt, r = rc.svd_rank_batched_complex(torch.zeros((0, 30, 20), dtype=dtype, device="cuda"), 8)
    assert u.shape == (0, 30, 8) and s.shape == (0, 20) and vt.shape == (0, 8, 20) and r.shape == (0,)
    assert u.dtype == dtype and s.dtype == real
    with pytest.raises(TypeError):
        rc.svd_rank_batched_complex(torch.zeros((1, 8, 8), dtype=real, device="cuda"), 4)


# ---------------------------------------------------------------- 11. the C++ mirror
def test_cpp_mirror_batched_svd_complex_example_runs(tmp_path):
    from tests.test_abi_cpu import build_cpp_mirror_examples

    exe = build_cpp_mirror_examples(tmp_path, "batched_svd_complex_example.cpp")
    res = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=dict(os.environ))
    assert res.returncode == 0 and "ALL OK" in res.stdout, res.stdout + res.stderr
