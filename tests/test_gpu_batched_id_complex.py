"""Batched column ID of many small same-shaped COMPLEX matrices (rc_column_id_rank_batched_c64 / _c32, batch.column_id_rank_batched).

Per matrix the reference sequence QR::compute_from(a) -> compress(.) -> column_id() on complex data (?geqp3 is zgeqp3 / cgeqp3,
src/pivoted_qr.rs:187-190), checked against the SciPy-LAPACK oracle and the lone call rc_column_id_rank_c*; plus the contract of
the batch itself (independence of the neighbours, layouts, graph capture, conjugation symmetry, argument checks, containment of
non-finite input)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import rusty_compression_amd as rc
from oracle import ref_lapack as o
from rusty_compression_amd import _lib
from rusty_compression_amd.batch import column_id_rank
from tests.helpers import TOL, agreed_pivot_prefix, batched_launch, is_permutation, npy, rel, stable_prefix

pytestmark = pytest.mark.gpu

C64, C32 = np.complex128, np.complex64
TIE = {np.dtype(np.float64): 1e-6, np.dtype(np.float32): 5e-3}
SLACK_FLOOR = {np.dtype(np.float64): 1e-4, np.dtype(np.float32): 1e-2}


def real_of(dtype):
    """The real dtype of a complex one: the tolerances of tests/helpers.py are keyed by it."""
    return np.dtype(np.float64) if np.dtype(dtype) == np.dtype(C64) else np.dtype(np.float32)


def batched(a, k, tol=0.0):
    c, z, ind, ranks = rc.column_id_rank_batched(a, k, tol)
    torch.cuda.synchronize()
    return npy(c), npy(z), npy(ind), npy(ranks)


def gaussian(rng, m, n, dtype):
    return o.random_gaussian((m, n), rng, dtype)


def decaying(rng, m, n, dtype, lo=1e-10):
    """U diag(geomspace) V^H with complex orthonormal U, V."""
    return o.random_approximate_low_rank_matrix((m, n), 1.0, lo, rng, dtype)


def phased(rng, m, n, dtype, lo=1e-10):
    """A real decaying spectrum times random unit-modulus column phases."""
    a = o.random_approximate_low_rank_matrix((m, n), 1.0, lo, rng, np.float64)
    return (a * np.exp(2j * np.pi * rng.random(n))[None, :]).astype(dtype)


def r_of(a, ind, k):
    """R (k x n, pivoted order) of A[:, ind] in c128: what the batched call factored, up to unit-modulus row factors."""
    return np.linalg.qr(np.asarray(a, dtype=np.complex128)[:, ind], mode="r")[:k]


def greedy_pivot_slack(a, r, ind, k):
    """tests/helpers.greedy_pivot_slack for complex data: partial norms from |A|^2 and |R_ij|^2 in f64."""
    a = np.asarray(a, dtype=np.complex128)
    r = np.asarray(r, dtype=np.complex128)
    vn2 = (np.abs(a[:, np.asarray(ind)]) ** 2).sum(axis=0)
    slack = []
    for j in range(k):
        rest = np.sqrt(np.maximum(vn2[j:], 0.0))
        mx = float(rest.max())
        slack.append((mx - abs(r[j, j])) / mx if mx > 0 else 0.0)
        vn2 = vn2 - np.abs(r[j]) ** 2
    return slack


def check_one(a, c, z, ind, r, k, dtype, oracle_tol=None):
    """One matrix of a batch against zgeqp3 / cgeqp3: pivots, C bit for bit, Z's identity block, the reconstruction C Z."""
    m, n = a.shape
    rd = real_of(dtype)
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
    agreed = agreed_pivot_prefix(ind, mine, ref.ind, ref.r, rd)
    d = np.abs(np.diag(ref.r)[:r]).astype(np.float64)
    ns = min(stable_prefix(ref.r, rd), int(np.sum(d >= SLACK_FLOOR[rd] * d[0])))
    assert max(greedy_pivot_slack(a, mine, ind, ns) or [0.0]) <= TIE[rd]
    if agreed == r:
        oc = ref.column_id()
        assert rel(c[:, :r] @ z[:r], oc.c @ oc.z) <= TOL[rd]["factor"]
    err = np.linalg.norm(a - c[:, :r] @ z[:r]) / np.linalg.norm(a)
    oerr = np.linalg.norm(a - ref.column_id().to_mat()) / np.linalg.norm(a)
    assert err <= 1.5 * oerr + 100 * np.finfo(rd).eps


# ---------------------------------------------------------------- 1. oracle parity across shapes, both kernel variants
# In LDS: c64 64 x 48, 96 x 96 and the degenerate shapes; c32 64 x 48, 128 x 128.  Workspace: c64 128 x 128, and 512 x 256, 200 x 512
# for both.
SHAPES = {
    C64: [(64, 48, 16), (96, 96, 96), (128, 128, 64), (512, 256, 32), (200, 512, 100), (1, 40, 1), (40, 1, 1), (30, 30, 30)],
    C32: [(64, 48, 48), (128, 128, 128), (512, 256, 32), (200, 512, 100), (1, 40, 1), (40, 1, 1)],
}


@pytest.mark.parametrize("dtype,m,n,k", [(d, *s) for d in (C64, C32) for s in SHAPES[d]])
def test_oracle_parity_across_shapes(dtype, m, n, k):
    rng = np.random.default_rng(m * 1000 + n + k + (0 if dtype == C64 else 7))
    mats = [gaussian(rng, m, n, dtype), phased(rng, m, n, dtype)]
    if min(m, n) > 1:
        mats.append(decaying(rng, m, n, dtype, 1e-3))
    c, z, ind, ranks = batched(torch.from_numpy(np.stack(mats)).cuda(), k)
    kk = min(k, m, n)
    assert c.shape == (len(mats), m, kk) and z.shape == (len(mats), kk, n) and c.dtype == dtype
    for i, a in enumerate(mats):
        assert ranks[i] == kk
        check_one(a, c[i], z[i], ind[i], int(ranks[i]), kk, dtype)


# ---------------------------------------------------------------- 2. agreement with the lone call rc_column_id_rank_c*
@pytest.mark.parametrize("dtype", [C64, C32])
@pytest.mark.parametrize("m,n,k", [(64, 48, 16), (300, 180, 40)])
def test_agrees_with_the_lone_call(dtype, m, n, k):
    rng = np.random.default_rng(7 + m)
    mats = [phased(rng, m, n, dtype) for _ in range(2)] + [decaying(rng, m, n, dtype)] + [gaussian(rng, m, n, dtype) for _ in range(2)]
    c, z, ind, ranks = batched(torch.from_numpy(np.stack(mats)).cuda(), k)
    tol = TOL[real_of(dtype)]["factor"]
    checked = 0
    for i, a in enumerate(mats):
        lc, lz, lind = (npy(t) for t in column_id_rank(torch.from_numpy(a).cuda(), k))
        agreed = agreed_pivot_prefix(ind[i], r_of(a, ind[i], k), lind, r_of(a, lind, k), real_of(dtype))
        if agreed == k:
            checked += 1
            assert np.array_equal(ind[i][:k], lind[:k])
            assert rel(z[i], lz) <= tol
            assert rel(c[i] @ z[i], lc @ lz) <= tol
    assert checked >= 3


# ---------------------------------------------------------------- 3. tolerance mode
@pytest.mark.parametrize("dtype,tol", [(C64, 1e-8), (C32, 1e-4)])
def test_tolerance_mode_exact_ranks_zero_and_full(dtype, tol):
    rng = np.random.default_rng(3)
    m, n, k = 150, 120, 64
    mats = [(gaussian(rng, m, rank, np.complex128) @ gaussian(rng, rank, n, np.complex128).conj()).astype(dtype) for rank in (5, 17, 40)]
    mats.append(np.zeros((m, n), dtype=dtype))
    mats += [gaussian(rng, m, n, dtype) for _ in range(2)]
    c, z, ind, ranks = batched(torch.from_numpy(np.stack(mats)).cuda(), k, tol)
    assert np.isfinite(c).all() and np.isfinite(z).all()
    assert list(ranks) == [5, 17, 40, 0, k, k]
    for i, a in enumerate(mats):
        r = int(ranks[i])
        assert is_permutation(ind[i], n)
        assert not np.any(c[i][:, r:]) and not np.any(z[i][r:])
        if r == 0:
            continue
        check_one(a, c[i], z[i], ind[i], r, k, dtype, oracle_tol=tol if r < k else None)


@pytest.mark.parametrize("dtype", [C64, C32])
def test_tolerance_between_two_singular_values(dtype):
    """A spectrum falling by 10x per singular value, with complex singular vectors: tol = 10^-4.5 cuts it between s_4 and s_5."""
    rng = np.random.default_rng(31)
    m, n, k = 90, 70, 40
    u = o.random_orthogonal_matrix((m, 10), rng, np.complex128)
    vh = o.random_orthogonal_matrix((10, n), rng, np.complex128)
    a = ((u * 10.0 ** -np.arange(10)) @ vh).astype(dtype)
    tol = 10 ** -4.5
    c, z, ind, ranks = batched(torch.from_numpy(np.stack([a, gaussian(rng, m, n, dtype)])).cuda(), k, tol)
    r = int(ranks[0])
    assert r == o.QR.compute_from(a).compress_qr_tolerance(tol).rank()
    assert 4 <= r <= 6 and ranks[1] == k
    check_one(a, c[0], z[0], ind[0], r, k, dtype, oracle_tol=tol)


# ---------------------------------------------------------------- 4. independence of position and neighbours
def test_bits_independent_of_position_and_neighbours():
    rng = np.random.default_rng(4)
    m, n, k = 64, 48, 16
    x = phased(rng, m, n, C64)
    alone, probe = batched_launch(lambda: batched(torch.from_numpy(x[None]).cuda(), k, 1e-6))
    big = torch.from_numpy(gaussian(rng, (2 * probe["slots"] + 37) * m, n, C64).reshape(-1, m, n)).cuda()  # slots: this shape's persistent grid
    big[5] *= 1e-3  # different neighbours, among them a tiny one
    for s in (len(big) // 2, len(big) - 1):
        b = big.clone()
        b[s] = torch.from_numpy(x)
        got, lab = batched_launch(lambda: batched(b, k, 1e-6))
        assert lab["count"] > 2 * lab["grid"]  # both positions are some workgroup's second or third matrix
        for u, v in zip(alone, got):
            assert np.array_equal(u[0], v[s])


# ---------------------------------------------------------------- 5. layouts
@pytest.mark.parametrize("dtype,m,n", [(C64, 70, 50), (C64, 140, 100), (C32, 70, 50)])
def test_layouts_give_the_same_bits(dtype, m, n):
    rng = np.random.default_rng(5)
    cnt, k = 9, 20
    base = torch.from_numpy(gaussian(rng, cnt * m, n, dtype).reshape(cnt, m, n)).cuda()
    ref = batched(base.contiguous(), k)
    transposed = base.transpose(1, 2).contiguous().transpose(1, 2)      # every matrix column-major
    padded = torch.zeros((cnt, m + 3, n + 5), dtype=base.dtype, device=base.device)
    padded[:, :m, :n] = base
    last = base.permute(1, 2, 0).contiguous().permute(2, 0, 1)          # a [m, n, count] array
    for view in (transposed, padded[:, :m, :n], last):
        got = batched(view, k)
        for u, v in zip(ref, got):
            assert np.array_equal(u, v)
    same = base[2:3].expand(6, m, n)  # a_batch_stride = 0: count identical results
    assert same.stride(0) == 0
    got = batched(same, k)
    for u, v in zip(ref, got):
        for i in range(6):
            assert np.array_equal(v[i], u[2])


# ---------------------------------------------------------------- 6. graph capture
def test_graph_capture_replays_the_eager_bits():
    rng = np.random.default_rng(6)
    cnt, m, n, k = 33, 128, 96, 24  # the workspace variant for c64
    lib = _lib.lib()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        a = torch.from_numpy(gaussian(rng, cnt * m, n, C64).reshape(cnt, m, n)).cuda()
        eager = batched(a, k, 1e-9)
        ctx = _lib.Context(torch.cuda.current_device(), st.cuda_stream)
        c = torch.zeros((cnt, m, k), dtype=a.dtype, device=a.device)
        z = torch.zeros((cnt, k, n), dtype=a.dtype, device=a.device)
        ind = torch.zeros((cnt, n), dtype=torch.int64, device=a.device)
        ranks = torch.zeros(cnt, dtype=torch.int64, device=a.device)
        st.synchronize()
        args = (_lib.rc_matrix(a.data_ptr(), m, n, a.stride(1), a.stride(2)), ctypes.c_int64(a.stride(0)), ctypes.c_int32(cnt), ctypes.c_int64(k),
                ctypes.c_double(1e-9), _lib.mat(c[0]), ctypes.c_int64(m * k), _lib.mat(z[0]), ctypes.c_int64(k * n), _lib.i64p(ind), _lib.i64p(ranks))
        ctx.check(lib.rc_column_id_rank_batched_c64(ctx._h, *args))  # eager once: sizes the workspace
        ctx.synchronize()
        ctx.get_health()
        for t in (c, z, ind, ranks):
            t.zero_()
        st.synchronize()
        graph = ctypes.c_void_p(None)
        ctx.check(lib.rc_graph_begin_capture(ctx._h))
        ctx.check(lib.rc_column_id_rank_batched_c64(ctx._h, *args))
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


# ---------------------------------------------------------------- 7. conjugation symmetry
@pytest.mark.parametrize("dtype,m,n,k,tol", [(C64, 64, 48, 16, 0.0), (C64, 200, 160, 60, 1e-7), (C32, 128, 128, 64, 1e-4), (C32, 300, 90, 40, 0.0)])
def test_conjugate_input_gives_conjugate_factors(dtype, m, n, k, tol):
    """Every operation of the kernel commutes exactly with negating the imaginary parts: conj(A) gives the same pivots and ranks
    and the elementwise conjugate of C and Z, bit for bit."""
    rng = np.random.default_rng(m + n + k)
    mats = np.stack([phased(rng, m, n, dtype), gaussian(rng, m, n, dtype), decaying(rng, m, n, dtype, 1e-6)])
    c, z, ind, ranks = batched(torch.from_numpy(mats).cuda(), k, tol)
    cc, zc, indc, ranksc = batched(torch.from_numpy(np.conj(mats)).cuda(), k, tol)
    assert np.array_equal(ind, indc) and np.array_equal(ranks, ranksc)
    assert np.array_equal(np.conj(c), cc) and np.array_equal(np.conj(z), zc)
    # a lazily conjugated tensor (torch.conj: a view with the conjugate bit) is read as the conjugate it stands for
    lazy = batched(torch.conj(torch.from_numpy(mats).cuda()), k, tol)
    for u, v in zip((cc, zc, indc, ranksc), lazy):
        assert np.array_equal(u, v)


# ---------------------------------------------------------------- 8. arguments
def _call(a, cnt, k, tol, c, cbs, z, zbs, dtype=torch.complex128):
    """One raw call; a, c and z are [2, rows, cols] buffers so that even a call the checks let through stays inside them."""
    ctx = _lib.default_context()
    fn = getattr(_lib.lib(), f"rc_column_id_rank_batched_{_lib.suffix(dtype)}")
    ind = torch.empty((2, a.shape[2]), dtype=torch.int64, device="cuda")
    ranks = torch.empty(2, dtype=torch.int64, device="cuda")
    return fn(ctx._h, _lib.mat(a[0]), ctypes.c_int64(a.stride(0)), ctypes.c_int32(cnt), ctypes.c_int64(k), ctypes.c_double(tol), _lib.mat(c[0]),
              ctypes.c_int64(cbs), _lib.mat(z[0]), ctypes.c_int64(zbs), _lib.i64p(ind), _lib.i64p(ranks))


@pytest.mark.parametrize("dtype", [torch.complex128, torch.complex64])
def test_argument_checks(dtype):
    dev = "cuda"
    e = lambda r, c: torch.zeros((2, r, c), dtype=dtype, device=dev)  # noqa: E731
    call = lambda *args: _call(*args, dtype=dtype)  # noqa: E731
    INVALID = 5
    assert call(e(520, 130), 2, 8, 0.0, e(520, 8), 520 * 8, e(8, 130), 8 * 130) == INVALID        # m > 512
    assert call(e(130, 520), 2, 8, 0.0, e(130, 8), 130 * 8, e(8, 520), 8 * 520) == INVALID        # n > 512
    a = e(200, 200)
    assert call(a, 2, 16, 0.0, e(200, 16), 200 * 16, e(16, 200), 16 * 200) == 0             # the baseline passes
    assert call(a, 2, 129, 0.0, e(200, 129), 200 * 129, e(129, 200), 129 * 200) == INVALID  # k > 128
    assert call(a, 2, 0, 0.0, e(200, 1), 200, e(1, 200), 200) == INVALID                    # k < 1
    assert call(a, 2, 16, 1.0, e(200, 16), 200 * 16, e(16, 200), 16 * 200) == INVALID       # tol >= 1
    assert call(a, 2, 16, -1e-3, e(200, 16), 200 * 16, e(16, 200), 16 * 200) == INVALID     # tol < 0
    assert call(a, -1, 16, 0.0, e(200, 16), 200 * 16, e(16, 200), 16 * 200) == INVALID      # count < 0
    assert call(a, 2, 16, 0.0, e(200, 16), 200 * 16 - 1, e(16, 200), 16 * 200) == INVALID   # C of two matrices overlap
    assert call(a, 2, 16, 0.0, e(200, 16), 200 * 16, e(16, 200), 15 * 200) == INVALID       # Z of two matrices overlap
    assert call(a, 2, 16, 0.0, e(200, 15), 200 * 15, e(16, 200), 16 * 200) == INVALID       # wrong C shape
    assert call(a, 2, 16, 0.0, e(200, 16), 200 * 16, e(16, 199), 16 * 199) == INVALID       # wrong Z shape
    msg = _lib.lib().rc_last_error_message(_lib.default_context()._h).decode()
    assert "column_id_rank_batched: c must be 200 x 16 and z 16 x 200" in msg
    assert call(a, 0, 16, 0.0, e(200, 16), 200 * 16, e(16, 200), 16 * 200) == 0            # count = 0: nothing to do
    with pytest.raises(AssertionError, match="rc_column_id_rank_"):  # RC_INVALID_ARGUMENT: the reference asserts
        rc.column_id_rank_batched(torch.zeros((1, 600, 10), dtype=dtype, device=dev), 4)
    c, z, ind, ranks = rc.column_id_rank_batched(torch.zeros((0, 30, 20), dtype=dtype, device=dev), 8)
    assert c.shape == (0, 30, 8) and z.shape == (0, 8, 20) and ind.shape == (0, 20) and ranks.shape == (0,) and c.dtype == dtype


# ---------------------------------------------------------------- 9. containment of non-finite input
@pytest.mark.parametrize("dtype", [C64, C32])
def test_nan_stays_in_its_matrix(dtype):
    rng = np.random.default_rng(9)
    cnt, m, n, k = 12, 90, 70, 30
    clean = torch.from_numpy(gaussian(rng, cnt * m, n, dtype).reshape(cnt, m, n)).cuda()
    ref = batched(clean, k, 1e-5)
    bad = clean.clone()
    bad[4, 17, 23] = complex(float("nan"), 0.0)
    bad[8, :, 5] = complex(0.0, float("inf"))
    got = batched(bad, k, 1e-5)
    for i in range(cnt):
        assert is_permutation(got[2][i], n) and 0 <= got[3][i] <= k
        if i in (4, 8):
            continue
        for u, v in zip(ref, got):
            assert np.array_equal(u[i], v[i])


# ---------------------------------------------------------------- 10. the C++ mirror
def test_cpp_mirror_batched_complex_example_runs(tmp_path):
    from tests.test_abi_cpu import build_cpp_mirror_examples

    exe = build_cpp_mirror_examples(tmp_path, "batched_complex_example.cpp")
    res = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=dict(os.environ))
    assert res.returncode == 0 and "ALL OK" in res.stdout, res.stdout + res.stderr
