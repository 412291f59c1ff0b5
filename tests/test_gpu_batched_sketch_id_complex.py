"""Batched sketched column ID of complex tall blocks (rc_sketch_column_id_rank_complex_batched_c64 / _c32,
batch.sketch_column_id_rank_batched_complex): the complex twin of tests/test_gpu_batched_sketch_id.py, group by group.

Per block the sketch Y = omega a (nothing conjugated) formed in one pass over a, then the complex column ID of Y.  Checked: the
sketch against omega a formed in complex128 on the host, component by component, under the dot-product bound of the stated arithmetic;
Z, col_ind and ranks against rc_column_id_rank_batched_c64 / _c32 on the sketch, bit for bit, with C gathered from a; the factorization
end to end against the same algorithm on the host (SciPy's complex pivoted QR of omega a); and the contract of the batch (plans, views,
count and position, graph capture, the conjugation and zero-imaginary-part properties, containment of non-finite input, the default
omega, argument checks, the C++ example).

The bound of group 1.  Each of Re y and Im y is one chain of v_mfma_*_16x16x4 steps from zero over the ascending rows of a, two
instructions of four products per four-row step: 2 m products (with the zero fill, 2 * 4 ceil(m / 4) <= 2 m + 6) added into one
accumulator.  Whatever the order inside an instruction, a sum of N products evaluated with one rounding or more per operation is within
gamma_N sum |x_i y_i| of the exact one (Higham, Accuracy and Stability, (3.5)), gamma_N = N u / (1 - N u) <= (N + 2) u here, so
    |Re y - Re y_ref| <= c (2 m + 8) u (|Om_re| |A_re| + |Om_im| |A_im|),   |Im y - Im y_ref| <= c (2 m + 8) u (|Om_re| |A_im| + |Om_im| |A_re|)
with u the unit roundoff of the real type: the real suite's (m + 4) u with the chain twice as long.  c = 1 for complex64 (the complex128
reference is exact at that scale) and 2 for complex128, whose NumPy reference rounds as much again.

The shapes are the real suite's plus the one boundary this kernel adds: a wave holds at most four 16-row tiles of Y, so l > 64 takes a
second pass over the panels (l = 64, 65, 96, 112 beside the l = 128 of the table).  The row chunk stays 32 and the column panel 64."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import scipy.linalg
import torch

import rusty_compression_amd as rc
from oracle import ref_lapack as o
from rusty_compression_amd import _lib
from rusty_compression_amd.random_matrix import Rng
from tests.helpers import batched_launch, is_permutation, npy

pytestmark = pytest.mark.gpu

# the kernel's two tiling constants (rc_gemm.hpp): rows of a per LDS chunk, columns of Y per panel
ROW_CHUNK = 32   # BSI_ROWS
COL_PANEL = 64   # BSI_COLS
MAX_LDS = 159 * 1024  # BID_MAX_LDS
PASS_TILES = 4   # BSC_TILES (kernels_batched_id_c.hip): 16-row tiles of Y per pass over the panels, l > 64 takes a second pass

DTYPES = [np.complex128, np.complex64]
TOLS = {np.dtype(np.complex128): 1e-8, np.dtype(np.complex64): 1e-4}
REAL = {np.dtype(np.complex128): np.float64, np.dtype(np.complex64): np.float32}
# (m, n, l): edges of the 16-row tiles, the 4-row MFMA step and the plans, every row tile, m past the old domain, then m one less than, at
# and one more than the row chunk, and n likewise around the column panel
SHAPES = [(1, 1, 1), (3, 5, 2), (5, 17, 15), (63, 15, 16), (64, 63, 17), (65, 65, 33), (257, 130, 40), (1030, 33, 128), (700, 512, 128),
          (ROW_CHUNK - 1, 20, 9), (ROW_CHUNK, 20, 9), (ROW_CHUNK + 1, 20, 9), (50, COL_PANEL - 1, 12), (50, COL_PANEL, 12), (50, COL_PANEL + 1, 12),
          (2048, 96, 24),
          # the second pass over the panels: l at and past 16 * PASS_TILES, then two and three row tiles in the second pass (l = 128: four)
          (70, 40, 16 * PASS_TILES), (70, 40, 16 * PASS_TILES + 1), (90, 50, 96), (90, 70, 112)]


def tt(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def sketch_id(a, omega, k, tol=0.0, want_y=True):
    """The call on device tensors; numpy results (c, z, ind, ranks[, y])."""
    out = rc.sketch_column_id_rank_batched_complex(a, k, tol, omega=omega, return_sketch=want_y)
    torch.cuda.synchronize()
    return tuple(npy(t) for t in out)


def cgauss(rng, shape, dtype=np.complex128):
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(dtype)


def decaying(rng, m, n, dtype):
    """random_approximate_low_rank_matrix (singular values from 1 to 1e-10) as the real and as the imaginary part."""
    if min(m, n) < 2:
        return cgauss(rng, (m, n), dtype)
    return (o.random_approximate_low_rank_matrix((m, n), 1.0, 1e-10, rng) + 1j * o.random_approximate_low_rank_matrix((m, n), 1.0, 1e-10, rng)).astype(dtype)


def same_bytes(p, q):
    return p.shape == q.shape and p.dtype == q.dtype and np.array_equal(np.ascontiguousarray(p).view(np.uint8), np.ascontiguousarray(q).view(np.uint8))


_DATA = {}


def data(m, n, l, dtype):
    """Two blocks per shape, one Gaussian and one with a decaying spectrum, a shared Gaussian omega, omega a in complex128 and the two
    matrices of absolute products the component bounds are made of (made once, never changed)."""
    key = (m, n, l, np.dtype(dtype))
    if key not in _DATA:
        rng = np.random.default_rng(1000 * m + 10 * n + l)
        a = np.stack([cgauss(rng, (m, n), dtype), decaying(rng, m, n, dtype)])
        om = cgauss(rng, (l, m), dtype)
        om128, a128 = om.astype(np.complex128), a.astype(np.complex128)
        ore, oim, are, aim = np.abs(om128.real), np.abs(om128.imag), np.abs(a128.real), np.abs(a128.imag)
        _DATA[key] = (a, om, om128 @ a128, ore @ are + oim @ aim, ore @ aim + oim @ are)
    return _DATA[key]


def check_bit_contract(a, y, got, k, tol):
    """got = (c, z, ind, ranks) of the sketched call on the blocks a; y its sketch.  z, ind, ranks = the complex batched column ID of y,
    bit for bit; c gathered from a; zero tails."""
    c, z, ind, ranks = got
    cnt, l, n = y.shape
    kk = min(k, l, n)
    _, rz, rind, rranks = rc.column_id_rank_batched(tt(y), k, tol)
    torch.cuda.synchronize()
    assert c.shape == (cnt, a.shape[1], kk) and z.shape == (cnt, kk, n)
    assert np.array_equal(ranks, npy(rranks))
    assert np.array_equal(ind, npy(rind))
    assert same_bytes(z, npy(rz))  # bytes: a NaN would compare equal to itself, -0.0 not to 0.0
    for i in range(cnt):
        r = int(ranks[i])
        assert 0 <= r <= kk and is_permutation(ind[i], n)
        assert same_bytes(c[i][:, :r], a[i][:, ind[i][:r]])
        assert not np.any(c[i][:, r:]) and not np.any(z[i][r:])


# ---------------------------------------------------------------- 1. the sketch against the host
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m,n,l", SHAPES)
def test_sketch_against_the_host(m, n, l, dtype):
    a, om, y_ref, re_abs, im_abs = data(m, n, l, dtype)
    y = sketch_id(tt(a), tt(om), min(l, 128))[4]
    assert y.shape == (2, l, n) and y.dtype == np.dtype(dtype)
    u = np.finfo(REAL[np.dtype(dtype)]).eps / 2  # unit roundoff of the real type
    cst = 1.0 if dtype == np.complex64 else 2.0  # complex128: the NumPy reference rounds too
    tiny = np.finfo(np.float64).tiny
    y128 = y.astype(np.complex128)
    worst = 0.0
    for name, got, ref, absm in (("Re", y128.real, y_ref.real, re_abs), ("Im", y128.imag, y_ref.imag, im_abs)):
        bound = cst * (2 * m + 8) * u * absm
        err = np.abs(got - ref)
        ratio = float(np.max(err / np.maximum(bound, tiny)))
        worst = max(worst, ratio)
        print(f"sketch {m}x{n} l={l} {np.dtype(dtype).name} {name}: max |y - y_ref| / bound = {ratio:.3e}")
        assert np.all(err <= bound), name
    print(f"sketch {m}x{n} l={l} {np.dtype(dtype).name}: worst ratio {worst:.3e}")


# ---------------------------------------------------------------- 2. the bit contract
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m,n,l", SHAPES)
def test_bit_contract_with_the_batched_column_id_of_the_sketch(m, n, l, dtype):
    a, om, _, _, _ = data(m, n, l, dtype)
    ad, omd = tt(a), tt(om)
    # k past min(l, n) is clamped; k = 200 is past the domain (k <= 128) of this call and of rc_column_id_rank_batched_c*: both reject it
    for k in sorted({1, max(l // 2, 1), l, 128, 200}):
        for tol in (0.0, TOLS[np.dtype(dtype)]):
            if k > 128:
                with pytest.raises(AssertionError):
                    sketch_id(ad, omd, k, tol)
                with pytest.raises(AssertionError):
                    rc.column_id_rank_batched(torch.zeros((2, l, n), dtype=ad.dtype, device="cuda"), k, tol)
                continue
            got = sketch_id(ad, omd, k, tol)
            check_bit_contract(a, got[4], got[:4], k, tol)
            without = sketch_id(ad, omd, k, tol, want_y=False)
            for p, q in zip(got[:4], without):
                assert same_bytes(p, q)


# ---------------------------------------------------------------- 3. end to end beyond the old domain
def host_route(a, om, r):
    """The same algorithm on the host in complex128: SciPy's pivoted QR of omega a, Z by a triangular solve, C gathered.  Returns
    ||a - C Z|| / ||a||."""
    a128 = a.astype(np.complex128)
    _, rr, piv = scipy.linalg.qr(om.astype(np.complex128) @ a128, mode="economic", pivoting=True)
    n = a.shape[1]
    z = np.zeros((r, n), dtype=np.complex128)
    z[:, piv[:r]] = np.eye(r)
    z[:, piv[r:]] = scipy.linalg.solve_triangular(rr[:r, :r], rr[:r, r:])
    return np.linalg.norm(a128 - a128[:, piv[:r]] @ z) / np.linalg.norm(a128)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m,n,l,k", [(2048, 96, 24, 16), (1030, 300, 40, 32)])
def test_end_to_end_beyond_the_old_domain(m, n, l, k, dtype):
    rng = np.random.default_rng(m + n + l)
    om = cgauss(rng, (l, m), dtype)
    exact = [(cgauss(rng, (m, r0)) @ cgauss(rng, (r0, n))).astype(dtype) for r0 in (6, 12)]
    c, z, ind, ranks = sketch_id(tt(np.stack(exact)), tt(om), k, TOLS[np.dtype(dtype)], want_y=False)
    assert list(ranks) == [6, 12]
    for i, a in enumerate(exact):
        r = int(ranks[i])
        assert is_permutation(ind[i], n)
        assert same_bytes(c[i][:, :r], a[:, ind[i][:r]]) and not np.any(c[i][:, r:]) and not np.any(z[i][r:])
    dec = [decaying(rng, m, n, dtype) for _ in range(2)]
    c, z, ind, ranks = sketch_id(tt(np.stack(dec)), tt(om), k, 0.0, want_y=False)
    for i, a in enumerate(dec):
        r = int(ranks[i])
        assert r == k and is_permutation(ind[i], n)
        assert same_bytes(c[i], a[:, ind[i][:r]])
        assert np.array_equal(z[i][:, ind[i][:r]], np.eye(r, dtype=dtype))
        a128 = a.astype(np.complex128)
        err = np.linalg.norm(a128 - c[i].astype(np.complex128) @ z[i].astype(np.complex128)) / np.linalg.norm(a128)
        oerr = host_route(a, om, r)
        print(f"decaying {m}x{n} l={l} k={k} {np.dtype(dtype).name}: err {err:.3e} host {oerr:.3e}")
        assert err <= 1.5 * oerr + 100 * np.finfo(dtype).eps


# ---------------------------------------------------------------- 4. plans
def lds_bytes(l, n, real, w_in_lds):
    """bsc_lds_bytes of kernels_batched_id_c.hip: [W: n x (l|1) complex] tile[8 x 9] complex | A chunk re, im, Omega chunk re, im, vn1[n]
    vn2[n] red[8] real | jp[n]; `real` the bytes of the real type."""
    lp = (min(l, 16 * PASS_TILES) + 15) // 16 * 16  # Omega's image holds the row tiles of one pass
    po = lp if lp & 16 else lp + 16
    cplx = 8 * 9 + (n * (l | 1) if w_in_lds else 0)
    reals = 2 * ROW_CHUNK * 80 + 2 * max(ROW_CHUNK * po, lp * (ROW_CHUNK + 2)) + 2 * n + 8
    return cplx * 2 * real + reals * real + 4 * n


@pytest.mark.parametrize("dtype", DTYPES)
def test_plans_on_both_sides_of_the_lds_boundary(dtype):
    l = 40 if dtype == np.complex128 else 80
    real = np.dtype(dtype).itemsize // 2
    n_fit = max(n for n in range(1, 513) if lds_bytes(l, n, real, True) <= MAX_LDS)  # the widest sketch that stays in LDS
    assert 64 < n_fit < 512
    assert n_fit == (139 if dtype == np.complex128 else 183)  # the boundaries DESIGN.md 7m lists for these l
    m, k = 70, 24
    rng = np.random.default_rng(44)
    om = tt(cgauss(rng, (l, m), dtype))
    for n, plan in ((n_fit, "lds"), (n_fit + 1, "ws")):
        a = np.stack([cgauss(rng, (m, n), dtype), decaying(rng, m, n, dtype)])
        got, lab = batched_launch(lambda: sketch_id(tt(a), om, k, TOLS[np.dtype(dtype)]))
        assert lab["op"] == "batched_sketch_id_c" and (lab["m"], lab["n"], lab["k"], lab["count"]) == (m, n, k, 2)
        assert lab["plan"].startswith(f"W:{plan},l={l},rows={ROW_CHUNK},cols={COL_PANEL},scratch=")  # then the instance's scratch bytes per thread
        check_bit_contract(a, got[4], got[:4], k, TOLS[np.dtype(dtype)])


# ---------------------------------------------------------------- 5. views
def raw(fn_dtype, a, omega, k, tol, y, c, z, ind, ranks, ctx=None, count=None):
    """One raw call on 3-D device views (omega 2-D: shared, batch stride 0; y None: not requested); returns the status."""
    ctx = ctx or _lib.default_context()
    fn = getattr(_lib.lib(), f"rc_sketch_column_id_rank_complex_batched_{_lib.suffix(fn_dtype)}")

    def view(t):
        if t is None:
            return _lib.mat(None), ctypes.c_int64(0)
        if t.dim() == 2:
            return _lib.rc_matrix(t.data_ptr(), t.shape[0], t.shape[1], t.stride(0), t.stride(1)), ctypes.c_int64(0)
        return _lib.rc_matrix(t.data_ptr(), t.shape[1], t.shape[2], t.stride(1), t.stride(2)), ctypes.c_int64(t.stride(0))

    return fn(ctx._h, *view(a), *view(omega), ctypes.c_int32(a.shape[0] if count is None else count), ctypes.c_int64(k), ctypes.c_double(tol), *view(y),
              *view(c), *view(z), _lib.i64p(ind), _lib.i64p(ranks))


@pytest.mark.parametrize("dtype,tol", [(torch.complex128, 1e-9), (torch.complex64, 1e-5)])
def test_views_give_the_contiguous_bits(dtype, tol):
    """Every layout of a and of omega, hence each of the kernel's four staging instances per dtype, gives the contiguous call's bits."""
    rng = np.random.default_rng(5)
    cnt, m, n, l, k = 6, 150, 70, 20, 12
    base = tt(cgauss(rng, (cnt, m, n))).to(dtype)
    om = tt(cgauss(rng, (l, m))).to(dtype)
    ref = sketch_id(base, om, k, tol)
    colmajor = base.transpose(1, 2).contiguous().transpose(1, 2)
    padded = torch.zeros((cnt, m + 3, n + 5), dtype=base.dtype, device="cuda")
    padded[:, :m, :n] = base
    last = base.permute(1, 2, 0).contiguous().permute(2, 0, 1)  # an [m, n, count] array
    om_cm = om.t().contiguous().t()
    assert colmajor.stride(1) == 1 and last.stride(0) == 1 and om_cm.stride(0) == 1
    stacked = om[None].repeat(cnt, 1, 1)
    # lazily conjugated tensors stand for the conjugate of what they store: here for base and om themselves
    lazy_a, lazy_om = torch.conj(base.conj().resolve_conj()), torch.conj(om.conj().resolve_conj())
    assert lazy_a.is_conj() and lazy_om.is_conj()
    for av, ov in ((colmajor, om), (padded[:, :m, :n], om), (last, om), (base, om_cm), (colmajor, om_cm), (padded[:, :m, :n], om_cm), (base, stacked),
                   (lazy_a, om), (base, lazy_om), (lazy_a, lazy_om)):
        got = sketch_id(av, ov, k, tol)
        for p, q in zip(ref, got):
            assert same_bytes(p, q)
    # a_batch_stride = 0: every block is block 0
    shared = sketch_id(base[0:1].expand(cnt, m, n), om, k, tol)
    for p, q in zip(ref, shared):
        for i in range(cnt):
            assert same_bytes(p[0], q[i])
    # a different omega per block = count calls with count = 1
    oms = tt(cgauss(rng, (cnt, l, m))).to(dtype)
    got = sketch_id(base, oms, k, tol)
    for i in range(cnt):
        one = sketch_id(base[i:i + 1], oms[i], k, tol)
        for p, q in zip(one, got):
            assert same_bytes(p[0], q[i])
    # strided y, c and z: the gaps keep their 7.0
    cb = torch.full((cnt, m + 2, k + 3), 7.0, dtype=base.dtype, device="cuda")
    zb = torch.full((cnt, k + 1, n + 4), 7.0, dtype=base.dtype, device="cuda")
    yb = torch.full((cnt, l + 2, n + 1), 7.0, dtype=base.dtype, device="cuda")
    ind = torch.empty((cnt, n), dtype=torch.int64, device="cuda")
    ranks = torch.empty(cnt, dtype=torch.int64, device="cuda")
    cv, zv, yv = cb[:, :m, :k], zb[:, :k, :n], yb[:, :l, :n]
    assert raw(dtype, base, om, k, tol, yv, cv, zv, ind, ranks) == 0
    torch.cuda.synchronize()
    for p, q in zip(ref, (cv, zv, ind, ranks, yv)):
        assert same_bytes(p, npy(q))
    for buf, view in ((cb, cv), (zb, zv), (yb, yv)):
        gaps = torch.ones(buf.shape, dtype=torch.bool, device="cuda")
        gaps[:, :view.shape[1], :view.shape[2]] = False
        assert bool((buf[gaps] == 7.0).all())


# ---------------------------------------------------------------- 6. bits independent of count and position
@pytest.mark.parametrize("dtype,tol", [(torch.complex128, 1e-6), (torch.complex64, 1e-4)])
def test_bits_independent_of_count_position_and_neighbours(dtype, tol):
    rng = np.random.default_rng(6)
    m, n, l, k = 100, 48, 20, 16
    om = tt(cgauss(rng, (l, m))).to(dtype)
    protos = [cgauss(rng, (m, n)), decaying(rng, m, n, np.complex128), 1e-3 * cgauss(rng, (m, n)),
              cgauss(rng, (m, 5)) @ cgauss(rng, (5, n)), 1e6 * decaying(rng, m, n, np.complex128), np.zeros((m, n), dtype=np.complex128),
              cgauss(rng, (m, 1)) @ cgauss(rng, (1, n))]
    alone = []
    for x in protos:
        got, lab = batched_launch(lambda: sketch_id(tt(x[None]).to(dtype), om, k, tol))
        assert (lab["count"], lab["grid"]) == (1, 1)
        alone.append(got)
    slots = lab["slots"]
    # a batch of 7 in two orders: every block first or last once, and among different neighbours
    seven = tt(np.stack(protos)).to(dtype)
    for order in (list(range(7)), [6, 2, 4, 0, 5, 1, 3]):
        got = sketch_id(seven[order].contiguous(), om, k, tol)
        for pos, i in enumerate(order):
            for p, q in zip(alone[i], got):
                assert same_bytes(p[0], q[pos])
    # more blocks than the persistent grid has workgroups: three of them take a second block
    count = slots + 3
    big = seven[torch.arange(count, device="cuda") % len(protos)].contiguous()
    got, lab = batched_launch(lambda: sketch_id(big, om, k, tol))
    assert lab["op"] == "batched_sketch_id_c" and (lab["m"], lab["n"], lab["k"]) == (m, n, k)
    assert lab["count"] == count and lab["grid"] == lab["slots"] == slots
    assert lab["plan"].startswith("W:lds,l=20")
    for i in range(count):
        for p, q in zip(alone[i % len(protos)], got):
            assert same_bytes(p[0], q[i])


# ---------------------------------------------------------------- 7. graph capture
@pytest.mark.parametrize("dtype,tol", [(torch.complex128, 1e-9), (torch.complex64, 1e-5)])
def test_graph_capture_replays_the_eager_bits(dtype, tol):
    rng = np.random.default_rng(7)
    cnt, m, n, l, k = 33, 300, 64, 20, 16
    lib = _lib.lib()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        a = tt(cgauss(rng, (cnt, m, n))).to(dtype)
        om = tt(cgauss(rng, (l, m))).to(dtype)
        eager = sketch_id(a, om, k, tol)
        ctx = _lib.Context(torch.cuda.current_device(), st.cuda_stream)
        c = torch.zeros((cnt, m, k), dtype=a.dtype, device="cuda")
        z = torch.zeros((cnt, k, n), dtype=a.dtype, device="cuda")
        y = torch.zeros((cnt, l, n), dtype=a.dtype, device="cuda")
        ind = torch.zeros((cnt, n), dtype=torch.int64, device="cuda")
        ranks = torch.zeros(cnt, dtype=torch.int64, device="cuda")
        st.synchronize()
        assert raw(dtype, a, om, k, tol, y, c, z, ind, ranks, ctx=ctx) == 0  # eager once: sizes the workspace
        ctx.synchronize()
        ctx.get_health()
        for t in (c, z, y, ind, ranks):
            t.zero_()
        st.synchronize()
        graph = ctypes.c_void_p(None)
        ctx.check(lib.rc_graph_begin_capture(ctx._h))
        ctx.check(raw(dtype, a, om, k, tol, y, c, z, ind, ranks, ctx=ctx))
        ctx.check(lib.rc_graph_end_capture(ctx._h, ctypes.byref(graph)))
        try:
            for _ in range(2):  # one captured launch, replayed twice
                for t in (c, z, y, ind, ranks):
                    t.zero_()
                st.synchronize()
                ctx.check(lib.rc_graph_launch(ctx._h, graph))
                ctx.synchronize()
                for p, q in zip(eager, (c, z, ind, ranks, y)):
                    assert same_bytes(p, npy(q))
            assert ctx.get_health() == 0
        finally:
            ctx.check(lib.rc_graph_destroy(ctx._h, graph))
            ctx.close()


# ---------------------------------------------------------------- 8. conjugation and zero imaginary parts
def is_conjugate_by_bits(got, ref):
    """got == conj(ref) bit for bit, except that a component that is zero in both may carry either sign (an exact cancellation is +0
    either way, and the zero tails are written as +0)."""
    rdt = REAL[got.dtype]
    udt = np.uint64 if rdt == np.float64 else np.uint32
    gr, gi = np.ascontiguousarray(got.real), np.ascontiguousarray(got.imag)
    rr, ri = np.ascontiguousarray(ref.real), np.ascontiguousarray(ref.imag)
    re_ok = (gr.view(udt) == rr.view(udt)) | ((gr == 0) & (rr == 0))
    im_ok = (gi.view(udt) == np.ascontiguousarray(-ri).view(udt)) | ((gi == 0) & (ri == 0))
    return bool(re_ok.all() and im_ok.all())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m,n,l", [(65, 65, 33), (257, 130, 40)])
def test_conjugation_and_zero_imaginary_parts(m, n, l, dtype):
    a, om, _, _, _ = data(m, n, l, dtype)
    k, tol = max(l // 2, 1), TOLS[np.dtype(dtype)]
    ref = sketch_id(tt(a), tt(om), k, tol)
    got = sketch_id(tt(a.conj()), tt(om.conj()), k, tol)
    assert np.array_equal(ref[2], got[2]) and np.array_equal(ref[3], got[3])
    for name, i in (("c", 0), ("z", 1), ("y", 4)):
        assert is_conjugate_by_bits(got[i], ref[i]), name
    # +0 imaginary parts: Re y carries the real call's bits on the real parts, Im y is zero
    a0, om0 = a.real.astype(dtype), om.real.astype(dtype)
    assert not np.any(np.signbit(a0.imag)) and not np.any(np.signbit(om0.imag))
    y = sketch_id(tt(a0), tt(om0), k, tol)[4]
    yr = rc.sketch_column_id_rank_batched(tt(np.ascontiguousarray(a.real)), k, tol, omega=tt(np.ascontiguousarray(om.real)), return_sketch=True)[4]
    torch.cuda.synchronize()
    assert same_bytes(np.ascontiguousarray(y.real), npy(yr))
    assert not np.any(y.imag)


# ---------------------------------------------------------------- 9. containment of non-finite input
@pytest.mark.parametrize("dtype", [torch.complex128, torch.complex64])
def test_non_finite_input_stays_in_its_block(dtype):
    rng = np.random.default_rng(8)
    cnt, m, n, l, k = 3, 130, 70, 30, 20
    clean = tt(cgauss(rng, (cnt, m, n))).to(dtype)
    om = tt(cgauss(rng, (l, m))).to(dtype)  # shared, and clean
    ref = sketch_id(clean, om, k, 1e-5)
    bad = clean.clone()
    bad[1, 17, 23] = complex(float("nan"), 1.0)
    bad[1, 99, 5] = complex(0.5, float("inf"))
    got = sketch_id(bad, om, k, 1e-5)
    for i in range(cnt):
        assert is_permutation(got[2][i], n) and 0 <= got[3][i] <= k
        if i == 1:
            continue
        for p, q in zip(ref, got):
            assert same_bytes(p[i], q[i])


# ---------------------------------------------------------------- 10. the default wrapper
@pytest.mark.parametrize("dtype", [torch.complex128, torch.complex64])
def test_default_omega_is_the_seeded_gaussian(dtype):
    rng = np.random.default_rng(9)
    cnt, m, n, k = 3, 200, 40, 10
    a = tt(cgauss(rng, (cnt, m, n))).to(dtype)
    got = rc.sketch_column_id_rank_batched_complex(a, k, 1e-6, seed=5, return_sketch=True)
    om = rc.random_gaussian((k + 8, m), Rng(5), dtype)
    assert om.dtype == dtype
    ref = rc.sketch_column_id_rank_batched_complex(a, k, 1e-6, omega=om, return_sketch=True)
    other = rc.sketch_column_id_rank_batched_complex(a, k, 1e-6, seed=6, oversampling=3, return_sketch=True)
    torch.cuda.synchronize()
    assert got[4].shape == (cnt, k + 8, n) and other[4].shape == (cnt, k + 3, n)
    for p, q in zip(got, ref):
        assert same_bytes(npy(p), npy(q))
    assert not np.array_equal(npy(got[4])[:, :k + 3], npy(other[4]))
    # l is capped at 128
    wide = rc.sketch_column_id_rank_batched_complex(a, 125, seed=1, return_sketch=True)
    assert wide[4].shape == (cnt, 128, n) and wide[0].shape == (cnt, m, 40)


# ---------------------------------------------------------------- 11. arguments, count = 0, dtype errors
@pytest.mark.parametrize("dtype", [torch.complex128, torch.complex64])
def test_argument_checks_count_zero_and_dtype_errors(dtype):
    INVALID = 5
    ctx = _lib.default_context()
    ctx.get_health()
    e = lambda r, c: torch.zeros((2, r, c), dtype=dtype, device="cuda")  # noqa: E731
    ind = torch.empty((2, 600), dtype=torch.int64, device="cuda")
    ranks = torch.empty(2, dtype=torch.int64, device="cuda")
    m, n, l, k = 60, 30, 12, 8

    def call(a=None, om=None, k=k, tol=0.0, y=None, c=None, z=None, ind=ind, ranks=ranks, count=2):
        a = e(m, n) if a is None else a
        om = e(l, m)[0] if om is None else om
        c = e(m, k) if c is None else c
        z = e(k, n) if z is None else z
        return raw(dtype, a, om, k, tol, y, c, z, ind, ranks, count=count)

    def shaped(t, rows, cols):  # a small allocation whose shape fields alone say rows x cols
        return t.as_strided((2, rows, cols), (1, 0, 0))

    assert call() == 0
    assert call(y=e(l, n)) == 0
    small = e(4, 4)
    assert call(a=shaped(small, m, 513), c=e(m, k), z=shaped(small, k, 513)) == INVALID           # n = 513
    assert call(om=shaped(small, 129, m)[0]) == INVALID                                            # l = 129
    assert call(a=shaped(small, 65537, n), om=shaped(small, l, 65537)[0], c=shaped(small, 65537, k)) == INVALID  # m = 65537
    assert call(k=0, c=e(m, 1), z=e(1, n)) == INVALID                                              # k < 1
    assert call(k=129, c=e(m, l), z=e(l, n)) == INVALID                                            # k > 128
    assert call(tol=1.0) == INVALID and call(tol=-1e-3) == INVALID                                 # tol outside [0, 1)
    assert call(count=-1) == INVALID
    assert call(om=e(l, m + 1)[0]) == INVALID                                                      # omega.cols != a.rows
    assert call(y=e(l + 1, n)) == INVALID and call(y=e(l, n - 1)) == INVALID                       # wrong y shape
    assert call(c=e(m, k - 1)) == INVALID and call(c=e(m + 1, k)) == INVALID                       # wrong c shape
    assert call(z=e(k, n + 1)) == INVALID and call(z=e(k + 1, n)) == INVALID                       # wrong z shape
    assert call(k=20, c=e(m, 20), z=e(20, n)) == INVALID                                           # kk = min(k, l, n) = 12, not 20
    assert call(k=20, c=e(m, l), z=e(l, n)) == 0
    overl = lambda r, c: torch.zeros((2, r, c), dtype=dtype, device="cuda").as_strided((2, r, c), (r * c - 1, c, 1))  # noqa: E731
    assert call(c=overl(m, k)) == INVALID and call(z=overl(k, n)) == INVALID and call(y=overl(l, n)) == INVALID  # overlapping output strides
    assert call(c=overl(m, k), count=1) == 0                                                       # one block: no stride to check
    # a null required pointer (the shape fields are right)
    fn = getattr(_lib.lib(), f"rc_sketch_column_id_rank_complex_batched_{_lib.suffix(dtype)}")
    v = lambda t: (_lib.mat(t[0]), ctypes.c_int64(t.stride(0)))  # noqa: E731
    nullmat = lambda r, c: (_lib.rc_matrix(None, r, c, c, 1), ctypes.c_int64(r * c))  # noqa: E731
    none = (_lib.mat(None), ctypes.c_int64(0))
    a0, om0, c0, z0 = e(m, n), e(l, m), e(m, k), e(k, n)
    tail = (ctypes.c_int32(2), ctypes.c_int64(k), ctypes.c_double(0.0))
    good = dict(a=v(a0), om=v(om0), c=v(c0), z=v(z0), ind=_lib.i64p(ind), ranks=_lib.i64p(ranks))
    for name, null in (("a", nullmat(m, n)), ("om", nullmat(l, m)), ("c", nullmat(m, k)), ("z", nullmat(k, n)), ("ind", None), ("ranks", None)):
        g = dict(good, **{name: null})
        assert fn(ctx._h, *g["a"], *g["om"], *tail, *none, *g["c"], *g["z"], g["ind"], g["ranks"]) == INVALID, name
    assert fn(ctx._h, *v(a0), *v(om0), *tail, *none, *v(c0), *v(z0), _lib.i64p(ind), _lib.i64p(ranks)) == 0
    assert fn(None, *v(a0), *v(om0), *tail, *none, *v(c0), *v(z0), _lib.i64p(ind), _lib.i64p(ranks)) == INVALID  # null context
    # count = 0: nothing to do, the outputs untouched, correctly shaped empty results
    c7, z7 = torch.full((2, m, k), 7.0, dtype=dtype, device="cuda"), torch.full((2, k, n), 7.0, dtype=dtype, device="cuda")
    y7 = torch.full((2, l, n), 7.0, dtype=dtype, device="cuda")
    i7, r7 = torch.full((2, n), 7, dtype=torch.int64, device="cuda"), torch.full((2,), 7, dtype=torch.int64, device="cuda")
    assert call(y=y7, c=c7, z=z7, ind=i7, ranks=r7, count=0) == 0
    torch.cuda.synchronize()
    for t in (c7, z7, y7, i7, r7):
        assert bool((t == 7).all())
    out = rc.sketch_column_id_rank_batched_complex(torch.zeros((0, 30, 20), dtype=dtype, device="cuda"), 8, return_sketch=True)
    assert [tuple(t.shape) for t in out] == [(0, 30, 8), (0, 8, 20), (0, 20), (0,), (0, 16, 20)]
    # dtype and rank errors of the wrappers: the real name keeps refusing complex data, the complex one refuses real data
    real = torch.float64 if dtype == torch.complex128 else torch.float32
    other = torch.complex64 if dtype == torch.complex128 else torch.complex128
    with pytest.raises(TypeError):
        rc.sketch_column_id_rank_batched(torch.zeros((2, 30, 20), dtype=dtype, device="cuda"), 4)
    with pytest.raises(TypeError):
        rc.sketch_column_id_rank_batched_complex(torch.zeros((2, 30, 20), dtype=real, device="cuda"), 4)
    for odt in (real, other):
        with pytest.raises(TypeError):
            rc.sketch_column_id_rank_batched_complex(torch.zeros((2, 30, 20), dtype=dtype, device="cuda"), 4,
                                                     omega=torch.zeros((6, 30), dtype=odt, device="cuda"))
    with pytest.raises(AssertionError):
        rc.sketch_column_id_rank_batched_complex(torch.zeros((30, 20), dtype=dtype, device="cuda"), 4)
    with pytest.raises(AssertionError, match="sketch_column_id_rank_batched"):  # RC_INVALID_ARGUMENT: the reference asserts
        rc.sketch_column_id_rank_batched_complex(torch.zeros((1, 30, 600), dtype=dtype, device="cuda"), 4)
    torch.cuda.synchronize()
    assert ctx.get_health() == 0


# ---------------------------------------------------------------- 12. the C++ mirror
def test_cpp_mirror_batched_sketch_id_complex_example_runs(tmp_path):
    """The example asserts that residual_batched's err is ||a - c z||_F formed on the host from the returned factors, to the complex
    residual example's bounds (1e-10 relative for c64, 1e-4 for c32), and that the recompressed factors reproduce the blocks."""
    from tests.test_abi_cpu import build_cpp_mirror_examples

    exe = build_cpp_mirror_examples(tmp_path, "batched_sketch_id_complex_example.cpp")
    res = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=dict(os.environ))
    print(res.stdout)
    assert res.returncode == 0 and "ALL OK" in res.stdout, res.stdout + res.stderr
