"""Batched range step of complex tall blocks (rc_sketch_range_step_complex_batched_c64 / _c32, batch.sketch_range_step_batched_complex)
and the power-iterated sketched column ID and SVD built on it (batch.sketch_power_omega_batched_complex,
sketch_column_id_rank_power_batched_complex, sketch_svd_rank_power_batched_complex): the complex twin of
tests/test_gpu_batched_range_step.py, group by group, plus the three properties only complex data has (p_conj, conjugation symmetry, zero
imaginary parts) and the step's input scale.

Per block one round of the reference's sample_range_power_iteration (src/random_sampling.rs:128-168) for c64 / c32: the sketch
Y = omega a (nothing conjugated), a basis Q of Y's rows with Q Q^H = I (pivoted complex Householder QR of the plain transpose Y^T) and
the projection P = a Q^H, or conj(P) when asked.  Checked: y against the complex sketched ID's y bit for bit; Q against LAPACK's Q of the
device's own Y in the same precision (SciPy's pivoted qr of Y^T), by orthonormality ||Q_r Q_r^H - I||_F and span
||Y - (Y Q_r^H) Q_r||_F / ||Y||_F, under the real file's rule: at most QR_MARGIN = 4 times LAPACK's figure plus sqrt(l) u; P against the
complex128 host product with the device's own Q, component by component.

The bound of the projection.  Each of Re p and Im p is one chain of v_mfma_*_16x16x4 steps from zero over the ascending columns of a, two
instructions of four products per four-column step: the sketch's chain (tests/test_gpu_batched_sketch_id_complex.py) with m replaced by
n, 2 n products (with the zero fill at most 2 n + 6) in one accumulator, so with gamma_N <= (N + 2) u
    |Re p - Re p_ref| <= c (2 n + 8) u (|A_re| |Q_re|^T + |A_im| |Q_im|^T),   |Im p - Im p_ref| <= c (2 n + 8) u (|A_re| |Q_im|^T + |A_im| |Q_re|^T)
with u the unit roundoff of the real type, c = 1 for complex64 and 2 for complex128 (whose NumPy reference rounds as much again).

The compositions are checked against the host model of tests/range_step_ref_complex.py with the same omega at its pinned seeds, and the
contract of the batch (layouts, views, count and position, neighbours, graph replay, ranks, non-finite input, argument checks) as in the
real file.  Every test here fails without rc_sketch_range_step_complex_batched_*: the symbol is missing.

Measured on an MI355X, worst over the shapes below: orthonormality 1.11 times LAPACK's figure in complex128 and 1.10 in complex64, span
0.97 and 0.98; the projection uses at most 0.061 (Re) / 0.033 (Im) of its bound in complex128 and 0.053 / 0.093 in complex64.  The
power-iterated ID and SVD agree with the host model's error to five digits on all three accuracy shapes in both precisions (ID
1.5652e-01, 3.5748e-02, 9.0333e-02 against 3.2049e-01, 5.7964e-02, 1.5339e-01 in one pass: ratios 0.49, 0.62, 0.59; SVD 1.2942e-01,
2.1763e-02, 6.6033e-02); U and Vt of the power SVD are orthonormal to 8.3e-15 and 1.1e-6."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import scipy.linalg
import torch

import rusty_compression_amd as rc
from rusty_compression_amd import _lib
from tests import range_step_ref_complex as ref
from tests import scale_cases as sc
from tests.helpers import TOL, npy
from tests.test_abi_cpu import build_cpp_mirror_examples

pytestmark = pytest.mark.gpu

DTYPES = [np.complex128, np.complex64]
TDTYPES = [torch.complex128, torch.complex64]
REAL = {np.dtype(np.complex128): np.float64, np.dtype(np.complex64): np.float32}
TREAL = {torch.complex128: torch.float64, torch.complex64: torch.float32}
QR_MARGIN = 4.0
# (m, n, l), the real file's: nothing a multiple of 16 / 32 / 64; the two accuracy shapes; l = 128 (two passes per product, the working copy out
# of LDS); l = n (two passes); l = 1
SHAPES = [(70, 33, 17), (1030, 300, 40), (600, 130, 24), (520, 130, 128), (96, 96, 96), (40, 64, 1)]


def tt(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def cgauss(rng, shape, dtype=np.complex128):
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(dtype)


def step(a, omega, want_y=True, conj_p=False):
    """The call on device tensors; numpy results (q, p, ranks[, y])."""
    out = rc.sketch_range_step_batched_complex(a, omega, return_sketch=want_y, conj_p=conj_p)
    torch.cuda.synchronize()
    return tuple(npy(t) for t in out)


def same_bits(x, y):
    x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
    return x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes()  # bytes: a NaN equals itself, -0.0 is not 0.0


def launch_label(fn):
    """fn() under the default context's event profile: (fn's result, the fields of the one op:batched_range_step_c label it recorded)."""
    ctx = _lib.default_context()
    lib = _lib.lib()
    labels = []
    ctx.check(lib.rc_profile_enable(ctx._h, 1))
    try:
        ctx.check(lib.rc_profile_reset(ctx._h))
        out = fn()
        cnt = ctypes.c_int32(0)
        ctx.check(lib.rc_profile_count(ctx._h, ctypes.byref(cnt)))
        for i in range(cnt.value):
            name = ctypes.create_string_buffer(192)
            ms, calls = ctypes.c_double(0), ctypes.c_int64(0)
            ctx.check(lib.rc_profile_get(ctx._h, i, name, 192, ctypes.byref(ms), ctypes.byref(calls)))
            if name.value.decode().startswith("op:batched_"):
                labels.append((name.value.decode(), calls.value))
    finally:
        lib.rc_profile_enable(ctx._h, 0)
        lib.rc_profile_reset(ctx._h)
    assert len(labels) == 1 and labels[0][1] == 1, labels
    mt = re.fullmatch(r"op:batched_range_step_c (\d+)x(\d+) l=(\d+) count=(\d+) grid=(\d+) slots=(\d+) plan=(\S+)", labels[0][0])
    assert mt, labels[0][0]
    f = dict(zip(("m", "n", "l", "count", "grid", "slots"), map(int, mt.groups()[:6])))
    f["plan"] = mt.group(7)
    return out, f


def raw(fn_dtype, a, omega, y, q, p, ranks, ctx=None, count=None, conj=0):
    """One raw call on 3-D device views (omega 2-D: shared, batch stride 0; y None: not requested); returns the status."""
    ctx = ctx or _lib.default_context()
    fn = getattr(_lib.lib(), f"rc_sketch_range_step_complex_batched_{_lib.suffix(fn_dtype)}")

    def view(t):
        if t is None:
            return _lib.mat(None), ctypes.c_int64(0)
        if t.dim() == 2:
            return _lib.rc_matrix(t.data_ptr(), t.shape[0], t.shape[1], t.stride(0), t.stride(1)), ctypes.c_int64(0)
        return _lib.rc_matrix(t.data_ptr(), t.shape[1], t.shape[2], t.stride(1), t.stride(2)), ctypes.c_int64(t.stride(0))

    return fn(ctx._h, *view(a), *view(omega), ctypes.c_int32(a.shape[0] if count is None else count), *view(y), *view(q), *view(p), _lib.i64p(ranks),
              ctypes.c_int32(conj))


_DATA = {}


def data(m, n, l, dtype):
    """Two blocks per shape, one complex Gaussian and one with the decaying spectrum of the model, and a shared complex Gaussian omega (made
    once, never changed)."""
    key = (m, n, l, np.dtype(dtype))
    if key not in _DATA:
        rng = np.random.default_rng(1000 * m + 10 * n + l)
        dec = ref.decaying(m + n, m, n) if min(m, n) >= 2 else cgauss(rng, (m, n))
        a, om = np.stack([cgauss(rng, (m, n)), dec]).astype(dtype), cgauss(rng, (l, m), dtype)
        a.setflags(write=False)
        om.setflags(write=False)
        _DATA[key] = (a, om)
    return _DATA[key]


def basis_figures(y, q, r):
    """(||Q_r Q_r^H - I||_F, ||Y - (Y Q_r^H) Q_r||_F / ||Y||_F) in complex128 for the rows 0 .. r-1 of q (l x n)."""
    y128, q128 = y.astype(np.complex128), q[:r].astype(np.complex128)
    return np.linalg.norm(q128 @ q128.conj().T - np.eye(r)), np.linalg.norm(y128 - (y128 @ q128.conj().T) @ q128) / np.linalg.norm(y128)


# ---------------------------------------------------------------- 1. one step against the host, on every shape edge
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m,n,l", SHAPES)
def test_one_step_against_the_host(m, n, l, dtype):
    a, om = data(m, n, l, dtype)
    ad, omd = tt(a), tt(om)
    (q, p, ranks, y), lab = launch_label(lambda: step(ad, omd))
    assert (lab["m"], lab["n"], lab["l"], lab["count"]) == (m, n, l, 2)
    assert re.fullmatch(r"W:(lds|ws),Q:ws,rows=\d+,cols=\d+,conj=0,scratch=\d+", lab["plan"]), lab["plan"]
    if (m, n, l) == (520, 130, 128) and dtype == np.complex128:
        assert lab["plan"].startswith("W:ws,")  # 128 x 131 complex128 do not fit in LDS
    assert q.shape == (2, l, n) and p.shape == (2, m, l) and y.shape == (2, l, n) and q.dtype == p.dtype == y.dtype == np.dtype(dtype)
    # the sketch is the complex sketched ID's, bit for bit, and the other outputs do not depend on whether it is written
    y_id = npy(rc.sketch_column_id_rank_batched_complex(ad, min(l, 128), 0.0, omega=omd, return_sketch=True)[4])
    assert same_bits(y, y_id)
    for g, w in zip((q, p, ranks), step(ad, omd, want_y=False)):
        assert same_bits(g, w)
    u = np.finfo(REAL[np.dtype(dtype)]).eps / 2
    cst = 1.0 if dtype == np.complex64 else 2.0
    tiny = np.finfo(np.float64).tiny
    for i in range(2):
        r = int(ranks[i])
        assert r == l  # full-rank data: no exactly zero pivot
        # the basis against LAPACK's on the device's own Y in the same precision
        lq = scipy.linalg.qr(y[i].T, mode="economic", pivoting=True)[0].T
        assert lq.dtype == np.dtype(dtype)
        orth, span = basis_figures(y[i], q[i], r)
        lorth, lspan = basis_figures(y[i], lq, r)
        floor = np.sqrt(l) * u
        print(f"step {m}x{n} l={l} {np.dtype(dtype).name} block {i} plan {lab['plan']}: orth {orth:.3e} lapack {lorth:.3e} ratio "
              f"{orth / max(lorth, floor):.2f}; span {span:.3e} lapack {lspan:.3e} ratio {span / max(lspan, floor):.2f}")
        # the projection against the complex128 host product with the device's own Q, per component
        a128, q128, p128 = a[i].astype(np.complex128), q[i].astype(np.complex128), p[i].astype(np.complex128)
        are, aim, qre, qim = np.abs(a128.real), np.abs(a128.imag), np.abs(q128.real).T, np.abs(q128.imag).T
        pref = a128 @ q128.conj().T
        fac = cst * (2 * n + 8) * u
        ere, eim = np.abs(p128.real - pref.real), np.abs(p128.imag - pref.imag)
        bre, bim = fac * (are @ qre + aim @ qim), fac * (are @ qim + aim @ qre)
        print(f"    projection: max |Re p - ref| / bound = {float(np.max(ere / np.maximum(bre, tiny))):.3e}, Im {float(np.max(eim / np.maximum(bim, tiny))):.3e}")
        assert orth <= QR_MARGIN * lorth + floor
        assert span <= QR_MARGIN * lspan + floor
        assert np.all(ere <= bre) and np.all(eim <= bim)


# ---------------------------------------------------------------- 2. p_conj, conjugation symmetry, zero imaginary parts
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m,n,l", SHAPES)
def test_conj_p_flips_the_imaginary_sign_at_the_store(m, n, l, dtype):
    a, om = data(m, n, l, dtype)
    ad, omd = tt(a), tt(om)
    q0, p0, r0, y0 = rc.sketch_range_step_batched_complex(ad, omd, return_sketch=True)
    q1, p1, r1, y1 = rc.sketch_range_step_batched_complex(ad, omd, return_sketch=True, conj_p=True)
    torch.cuda.synchronize()
    assert torch.equal(torch.view_as_real(p1), torch.view_as_real(p0.conj().resolve_conj()))
    # bit for bit: the real parts as they are, the imaginary parts with the sign bit flipped (a zero included)
    assert same_bits(npy(p1).real, npy(p0).real) and same_bits(npy(p1).imag, -npy(p0).imag)
    for w, g in ((q0, q1), (y0, y1), (r0, r1)):
        assert same_bits(npy(w), npy(g))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m,n,l", SHAPES)
def test_conjugated_inputs_give_the_conjugated_outputs(m, n, l, dtype):
    a, om = data(m, n, l, dtype)
    for conj_p in (False, True):
        q, p, ranks, y = (torch.from_numpy(x) for x in step(tt(a), tt(om), conj_p=conj_p))
        qc, pc, ranksc, yc = (torch.from_numpy(x) for x in step(tt(np.conj(a)), tt(np.conj(om)), conj_p=conj_p))
        assert torch.equal(ranks, ranksc)
        for name, w, g in (("y", y, yc), ("q", q, qc), ("p", p, pc)):
            assert torch.equal(torch.view_as_real(g), torch.view_as_real(w.conj().resolve_conj())), name


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m,n,l", SHAPES)
def test_zero_imaginary_parts_give_the_real_sketch_and_zero_imaginary_outputs(m, n, l, dtype):
    a, om = data(m, n, l, dtype)
    are, omre = np.ascontiguousarray(a.real), np.ascontiguousarray(om.real)
    q, p, ranks, y = step(tt(are.astype(dtype)), tt(omre.astype(dtype)))  # every imaginary part +0
    yr = npy(rc.sketch_range_step_batched(tt(are), tt(omre), return_sketch=True)[3])
    assert same_bits(y.real, yr)
    assert not np.any(y.imag) and not np.any(q.imag) and not np.any(p.imag)
    assert np.all(ranks == l)


# ---------------------------------------------------------------- 3. layouts and views
@pytest.mark.parametrize("dtype", TDTYPES)
def test_layouts_and_views_give_the_contiguous_bits(dtype):
    """Every layout of a and of omega, hence each of the kernel's four instances per dtype, gives the contiguous call's bits; so do a
    per-block omega and strided outputs, with and without y."""
    rng = np.random.default_rng(5)
    cnt, m, n, l = 6, 150, 70, 20
    base = tt(cgauss(rng, (cnt, m, n))).to(dtype)
    om = tt(cgauss(rng, (l, m))).to(dtype)
    want = step(base, om)
    colmajor = base.transpose(1, 2).contiguous().transpose(1, 2)
    padded = torch.zeros((cnt, m + 3, n + 5), dtype=base.dtype, device="cuda")
    padded[:, :m, :n] = base
    last = base.permute(1, 2, 0).contiguous().permute(2, 0, 1)  # an [m, n, count] array
    om_cm = om.t().contiguous().t()
    assert colmajor.stride(1) == 1 and last.stride(0) == 1 and om_cm.stride(0) == 1
    stacked = om[None].repeat(cnt, 1, 1)
    for av, ov in ((colmajor, om), (base, om_cm), (colmajor, om_cm), (padded[:, :m, :n], om), (padded[:, :m, :n], om_cm), (last, om), (base, stacked)):
        for w, g in zip(want, step(av, ov)):
            assert same_bits(w, g)
        for w, g in zip(want[:3], step(av, ov, want_y=False)):
            assert same_bits(w, g)
    # a different omega per block = count calls with count = 1
    oms = tt(cgauss(rng, (cnt, l, m))).to(dtype)
    got = step(base, oms)
    for i in range(cnt):
        for o, g in zip(step(base[i:i + 1], oms[i]), got):
            assert same_bits(o[0], g[i])
    # strided q, p and y: the gaps keep their 7 + 7i; p column-major inside its block; then the same without y
    for with_y in (True, False):
        qb = torch.full((cnt, l + 2, n + 3), 7.0 + 7.0j, dtype=base.dtype, device="cuda")
        pb = torch.full((cnt, l + 1, m + 4), 7.0 + 7.0j, dtype=base.dtype, device="cuda")
        yb = torch.full((cnt, l + 2, n + 1), 7.0 + 7.0j, dtype=base.dtype, device="cuda")
        ranks = torch.empty(cnt, dtype=torch.int64, device="cuda")
        qv, pv, yv = qb[:, :l, :n], pb[:, :l, :m].transpose(1, 2), yb[:, :l, :n]
        assert raw(dtype, base, om, yv if with_y else None, qv, pv, ranks) == 0
        torch.cuda.synchronize()
        for w, g in zip(want if with_y else want[:3], (qv, pv, ranks, yv)):
            assert same_bits(w, npy(g.contiguous()))
        for buf, rows, cols in ((qb, l, n), (pb, l, m), (yb, l if with_y else 0, n)):
            gaps = torch.ones(buf.shape, dtype=torch.bool, device="cuda")
            gaps[:, :rows, :cols] = False
            assert bool((buf[gaps] == 7.0 + 7.0j).all())


# ---------------------------------------------------------------- 4. bits independent of count, position, strides and neighbours
@pytest.mark.parametrize("dtype", TDTYPES)
def test_bits_independent_of_count_position_and_neighbours(dtype):
    rng = np.random.default_rng(6)
    m, n, l = 100, 48, 20
    om = tt(cgauss(rng, (l, m))).to(dtype)
    protos = [cgauss(rng, (m, n)), ref.decaying(3, m, n), 1e-3 * cgauss(rng, (m, n)), cgauss(rng, (m, 5)) @ cgauss(rng, (5, n)),
              np.full((m, n), np.nan + 1j * np.nan), np.zeros((m, n), dtype=np.complex128), cgauss(rng, (m, 1)) @ cgauss(rng, (1, n))]
    alone = []
    for x in protos:
        got, lab = launch_label(lambda: step(tt(x[None]).to(dtype), om))
        assert (lab["count"], lab["grid"]) == (1, 1)
        alone.append(got)
    slots = lab["slots"]
    count = slots + 3  # three workgroups take a second block, next to a block full of NaN
    big = torch.zeros((count, m + 1, n + 2), dtype=dtype, device="cuda")  # a batch stride and a row stride of its own
    big[:, :m, :n] = tt(np.stack(protos)).to(dtype)[torch.arange(count, device="cuda") % len(protos)]
    got, lab = launch_label(lambda: step(big[:, :m, :n], om))
    assert lab["count"] == count and lab["grid"] == lab["slots"] == slots
    for i in range(count):
        for o, g in zip(alone[i % len(protos)], got):
            assert same_bits(o[0], g[i])
        assert 0 <= got[2][i] <= l  # the NaN block included
    assert alone[5][2][0] == 0 and alone[0][2][0] == l


# ---------------------------------------------------------------- 5. graph replay
@pytest.mark.parametrize("dtype", TDTYPES)
def test_graph_replay_gives_the_eager_bits(dtype):
    rng = np.random.default_rng(7)
    cnt, m, n, l = 33, 300, 64, 20
    lib = _lib.lib()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        a = tt(cgauss(rng, (cnt, m, n))).to(dtype)
        om = tt(cgauss(rng, (l, m))).to(dtype)
        eager = step(a, om, conj_p=True)
        ctx = _lib.Context(torch.cuda.current_device(), st.cuda_stream)
        q = torch.zeros((cnt, l, n), dtype=a.dtype, device="cuda")
        p = torch.zeros((cnt, m, l), dtype=a.dtype, device="cuda")
        y = torch.zeros((cnt, l, n), dtype=a.dtype, device="cuda")
        ranks = torch.zeros(cnt, dtype=torch.int64, device="cuda")
        st.synchronize()
        assert raw(dtype, a, om, y, q, p, ranks, ctx=ctx, conj=1) == 0  # eager once: sizes the workspace
        ctx.synchronize()
        ctx.get_health()
        for t in (q, p, y, ranks):
            t.zero_()
        st.synchronize()
        graph = ctypes.c_void_p(None)
        ctx.check(lib.rc_graph_begin_capture(ctx._h))
        ctx.check(raw(dtype, a, om, y, q, p, ranks, ctx=ctx, conj=1))  # one launch: the capture has no parallel branches
        ctx.check(lib.rc_graph_end_capture(ctx._h, ctypes.byref(graph)))
        try:
            ctx.check(lib.rc_graph_launch(ctx._h, graph))
            ctx.synchronize()
            for e, g in zip(eager, (q, p, ranks, y)):
                assert same_bits(e, npy(g))
            assert ctx.get_health() == 0
        finally:
            ctx.check(lib.rc_graph_destroy(ctx._h, graph))
            ctx.close()


# ---------------------------------------------------------------- 6. ranks
@pytest.mark.parametrize("dtype", DTYPES)
def test_zero_and_exactly_rank_deficient_blocks(dtype):
    rng = np.random.default_rng(8)
    m, n, l = 90, 40, 12

    def cint(lo, hi, shape):
        return rng.integers(lo, hi, shape) + 1j * rng.integers(lo, hi, shape)

    # small Gaussian integers: a of exact rank 5 and an integer omega, so that Y = omega a is formed without rounding and has exact rank 5
    low = (cint(-3, 4, (m, 5)) @ cint(-3, 4, (5, n))).astype(dtype)
    om = cint(-2, 3, (l, m)).astype(dtype)
    a = np.stack([np.zeros((m, n), dtype=dtype), low, cgauss(rng, (m, n), dtype)])
    q, p, ranks, y = step(tt(a), tt(om))
    assert np.array_equal(y[1].astype(np.complex128), om.astype(np.complex128) @ low.astype(np.complex128))
    assert np.linalg.matrix_rank(y[1].astype(np.complex128)) == 5
    assert ranks[0] == 0 and not np.any(q[0]) and not np.any(p[0]) and not np.any(y[0])
    assert 5 <= ranks[1] <= l and ranks[2] == l
    print(f"exact rank 5 block {np.dtype(dtype).name}: r = {int(ranks[1])}")
    eps = np.finfo(REAL[np.dtype(dtype)]).eps
    for i in range(3):
        r = int(ranks[i])
        assert not np.any(q[i][r:]) and not np.any(p[i][:, r:])
        if r:
            orth, span = basis_figures(y[i], q[i], r)
            assert orth <= 100 * l * eps and span <= 100 * l * eps


@pytest.mark.parametrize("dtype", TDTYPES)
def test_non_finite_input_stays_in_its_block(dtype):
    rng = np.random.default_rng(9)
    cnt, m, n, l = 12, 130, 70, 30
    clean = tt(cgauss(rng, (cnt, m, n))).to(dtype)
    om = tt(cgauss(rng, (l, m))).to(dtype)
    want = step(clean, om)
    bad = clean.clone()
    bad[4, 17, 23] = complex(float("nan"), 1.0)
    bad[8, 99, 5] = complex(1.0, float("inf"))
    got = step(bad, om)
    for i in range(cnt):
        assert 0 <= got[2][i] <= l
        if i in (4, 8):
            continue
        for w, g in zip(want, got):
            assert same_bits(w[i], g[i])


# ---------------------------------------------------------------- 7. the step's input scale
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m,n,l", sc.STEP_SHAPES)
def test_range_step_at_every_scale(m, n, l, dtype):
    """2^e a gives y and p times 2^e and q and ranks unchanged, bit for bit, at the exponents of the complex sketched ID's far-scale tests
    (tests/scale_cases.py: three kinds of block at seven exponents in one batch).  The step only: the chains built on it are held to the
    same exponents in tests/test_gpu_batched_scales.py."""
    units, cells, stacked = sc.batch((m, n), dtype)
    om = sc.omega((m, n), l, dtype)
    for conj_p in (False, True):
        q, p, ranks, y = step(tt(stacked), tt(om), conj_p=conj_p)
        for idx, (i, e) in enumerate(cells):
            u = sc.unit_cell(cells, i)
            sc.assert_same_as_unit(("q", "p", "ranks", "y"), (q[u], p[u], ranks[u], y[u]), (q[idx], sc.descale(p[idx], e), ranks[idx], sc.descale(y[idx], e)))
        for i in range(2):  # the Gaussian and the 1e-3 kinds are of full rank at every exponent
            assert all(ranks[idx] == l for idx, (j, _) in enumerate(cells) if j == i)


# ---------------------------------------------------------------- 8. the compositions against the host model
_MODEL = {}


def model_case(case, dtype, sigma_min=1e-10):
    """The block and the omega of one accuracy case in `dtype` (made once); the host model runs on exactly these values."""
    key = (case, np.dtype(dtype), sigma_min)
    if key not in _MODEL:
        a, om = ref.case_data(case, sigma_min)
        _MODEL[key] = (a.astype(dtype), om.astype(dtype))
    return _MODEL[key]


_HOST = {}


def host(which, case, dtype):
    key = (which, case, np.dtype(dtype))
    if key not in _HOST:
        a, om = model_case(case, dtype)
        _HOST[key] = (ref.column_id_power if which == "id" else ref.svd_power)(a, om, case[3], 0.0, 1)
    return _HOST[key]


def rel_err(a, approx):
    a128 = a.astype(np.complex128)
    return np.linalg.norm(a128 - approx) / np.linalg.norm(a128)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", ref.DECAY_CASES)
def test_power_iterated_id_against_the_host_model(case, dtype):
    m, n, l, k = case
    a, om = model_case(case, dtype)
    ad, omd = tt(a[None]), tt(om)
    errs = []
    for its in (0, 1):
        c, z, ind, ranks = (npy(t) for t in rc.sketch_column_id_rank_power_batched_complex(ad, k, 0.0, power_iterations=its, omega=omd))
        assert ranks[0] == k and np.array_equal(c[0], a[:, ind[0][:k]])
        errs.append(rel_err(a, c[0].astype(np.complex128) @ z[0].astype(np.complex128)))
    oerr = host("id", case, dtype)[0]
    eps = np.finfo(REAL[np.dtype(dtype)]).eps
    print(f"power ID {m}x{n} l={l} k={k} {np.dtype(dtype).name}: q=0 {errs[0]:.4e} q=1 {errs[1]:.4e} ratio {errs[1] / errs[0]:.3f}; host q=1 {oerr:.4e}")
    assert errs[1] <= 1.5 * oerr + 100 * eps
    assert errs[1] <= 0.75 * errs[0]


@pytest.mark.parametrize("dtype", DTYPES)
def test_tolerance_example_reaches_the_models_rank(dtype):
    m, n, l, k = ref.TOL_CASE
    a, om = model_case(ref.TOL_CASE, dtype, ref.TOL_SIGMA_MIN)
    _, orank, ratios = ref.column_id_power(a, om, k, ref.TOL, 1)
    assert np.min(np.abs(ratios / ref.TOL - 1.0)) > 1e-6  # no ratio of the model within 1e-6 (relative) of the tolerance
    ranks = npy(rc.sketch_column_id_rank_power_batched_complex(tt(a[None]), k, ref.TOL, power_iterations=1, omega=tt(om))[3])
    print(f"tolerance example {np.dtype(dtype).name}: rank {int(ranks[0])}, host model {orank}")
    assert ranks[0] == orank == min(k, l, n) == 40


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", ref.DECAY_CASES)
def test_power_iterated_svd_against_the_host_model(case, dtype):
    m, n, l, k = case
    a, om = model_case(case, dtype)
    u, s, vt, ranks = (npy(t) for t in rc.sketch_svd_rank_power_batched_complex(tt(a[None]), k, 0.0, power_iterations=1, omega=tt(om)))
    assert u.shape == (1, m, k) and vt.shape == (1, k, n) and ranks[0] == k and s.dtype == np.dtype(REAL[np.dtype(dtype)])
    u0, s0, vt0 = u[0].astype(np.complex128), s[0][:k].astype(np.float64), vt[0].astype(np.complex128)
    orth = max(np.abs(u0.conj().T @ u0 - np.eye(k)).max(), np.abs(vt0 @ vt0.conj().T - np.eye(k)).max())
    err = rel_err(a, (u0 * s0) @ vt0)
    oerr, orank = host("svd", case, dtype)
    t = TOL[np.dtype(REAL[np.dtype(dtype)])]
    print(f"power SVD {m}x{n} l={l} k={k} {np.dtype(dtype).name}: err {err:.4e} host {oerr:.4e}; orth {orth:.3e} bound {4 * t['orth']:.3e}")
    assert orank == k
    assert orth <= 4 * t["orth"]
    assert np.all(np.diff(s0) <= 0) and s0[-1] > 0
    assert err <= 1.5 * oerr + 100 * np.finfo(REAL[np.dtype(dtype)]).eps


@pytest.mark.parametrize("dtype", TDTYPES)
def test_no_iterations_is_the_one_pass_call_and_the_chain_is_the_calls_by_hand(dtype):
    rng = np.random.default_rng(11)
    cnt, m, n, k = 3, 200, 40, 10
    a = tt(cgauss(rng, (cnt, m, n))).to(dtype)
    om = tt(cgauss(rng, (k + 6, m))).to(dtype)
    for kw in (dict(omega=om), dict(seed=5, oversampling=4)):
        for w, g in zip(rc.sketch_column_id_rank_batched_complex(a, k, 1e-6, return_sketch=True, **kw),
                        rc.sketch_column_id_rank_power_batched_complex(a, k, 1e-6, power_iterations=0, return_sketch=True, **kw)):
            assert same_bits(npy(w), npy(g))
        for w, g in zip(rc.sketch_svd_rank_batched_complex(a, k, 1e-6, **kw), rc.sketch_svd_rank_power_batched_complex(a, k, 1e-6, power_iterations=0, **kw)):
            assert same_bits(npy(w), npy(g))
    # the default omega is the sketched ID's; one iteration is the range step with conj_p, the tall recompression with right = I and the sketched ID
    q, p, ranks = rc.sketch_range_step_batched_complex(a, k=k, oversampling=4, seed=5, conj_p=True)
    l = k + 4
    q2, p2, ranks2 = rc.sketch_range_step_batched_complex(a, rc.random_gaussian((l, m), rc.Rng(5), dtype), conj_p=True)
    for w, g in ((q, q2), (p, p2), (ranks, ranks2)):
        assert same_bits(npy(w), npy(g))
    eye = torch.eye(l, dtype=dtype, device="cuda").expand(cnt, l, l)
    uu = rc.lowrank_recompress_tall_batched_complex(p, eye, l, 0.0, ranks=ranks)[0]
    omq = rc.sketch_power_omega_batched_complex(a, k, 1, oversampling=4, seed=5)
    assert omq.shape == (cnt, l, m) and not omq.is_conj() and same_bits(npy(omq.contiguous()), npy(uu.mT.contiguous()))
    # its rows are orthonormal and it is U^H of a basis of a Q^H's columns: omq^H omq reproduces the unconjugated projection
    gram = npy(omq).astype(np.complex128)
    assert np.abs(gram @ gram.conj().transpose(0, 2, 1) - np.eye(l)).max() <= 4 * TOL[np.dtype(REAL[npy(omq).dtype])]["orth"]
    pn = npy(rc.sketch_range_step_batched_complex(a, k=k, oversampling=4, seed=5)[1]).astype(np.complex128)
    back = gram.conj().transpose(0, 2, 1) @ (gram @ pn)
    assert np.linalg.norm(back - pn) <= 1e3 * l * np.finfo(REAL[npy(omq).dtype]).eps * np.linalg.norm(pn)
    for w, g in zip(rc.sketch_column_id_rank_batched_complex(a, k, 1e-6, omega=uu.mT),
                    rc.sketch_column_id_rank_power_batched_complex(a, k, 1e-6, oversampling=4, seed=5)):
        assert same_bits(npy(w), npy(g))
    two = rc.sketch_svd_rank_power_batched_complex(a, k, 1e-6, power_iterations=2, oversampling=4, seed=5)
    q3, p3, ranks3 = rc.sketch_range_step_batched_complex(a, uu.mT)
    for w, g in zip(rc.lowrank_recompress_tall_batched_complex(p3, q3, k, 1e-6, ranks=ranks3), two):
        assert same_bits(npy(w), npy(g))
    torch.cuda.synchronize()


# ---------------------------------------------------------------- 9. arguments, count = 0, dtype errors, the C++ example
def test_argument_checks_count_zero_and_dtype_errors():
    INVALID = 5
    ctx = _lib.default_context()
    ctx.get_health()
    e = lambda r, c: torch.zeros((2, r, c), dtype=torch.complex128, device="cuda")  # noqa: E731
    ranks = torch.empty(2, dtype=torch.int64, device="cuda")
    m, n, l = 60, 30, 12

    def call(a=None, om=None, y=None, q=None, p=None, ranks=ranks, count=2, conj=0):
        a = e(m, n) if a is None else a
        om = e(l, m)[0] if om is None else om
        q = e(l, n) if q is None else q
        p = e(m, l) if p is None else p
        return raw(torch.complex128, a, om, y, q, p, ranks, count=count, conj=conj)

    def shaped(t, rows, cols):  # a small allocation whose shape fields alone say rows x cols
        return t.as_strided((2, rows, cols), (1, 0, 0))

    assert call() == 0 and call(conj=1) == 0 and call(conj=-7) == 0  # any non-zero p_conj conjugates
    assert call(y=e(l, n)) == 0
    small = e(4, 4)
    assert call(om=e(31, m)[0], q=e(31, n), p=e(m, 31)) == INVALID                                 # l = 31 > n = 30
    assert call(a=e(10, n), om=e(l, 10)[0], p=e(10, l)) == INVALID                                 # l = 12 > m = 10
    assert call(a=shaped(small, 200, 200), om=shaped(small, 129, 200)[0], q=shaped(small, 129, 200), p=shaped(small, 200, 129)) == INVALID  # l = 129
    assert call(a=shaped(small, m, 513), q=shaped(small, l, 513)) == INVALID                       # n = 513
    assert call(a=shaped(small, 65537, n), om=shaped(small, l, 65537)[0], p=shaped(small, 65537, l)) == INVALID  # m = 65537
    assert call(a=shaped(small, 0, n), om=shaped(small, l, 0)[0], p=shaped(small, 0, l)) == INVALID  # m = 0
    assert call(a=shaped(small, m, 0), q=shaped(small, l, 0)) == INVALID                           # n = 0
    assert call(om=shaped(small, 0, m)[0], q=shaped(small, 0, n), p=shaped(small, m, 0)) == INVALID  # l = 0
    assert call(count=-1) == INVALID
    assert call(om=e(l, m + 1)[0]) == INVALID                                                      # omega.cols != a.rows
    assert call(y=e(l + 1, n)) == INVALID and call(y=e(l, n - 1)) == INVALID                       # wrong y shape
    assert call(q=e(l, n + 1)) == INVALID and call(q=e(l + 1, n)) == INVALID                       # wrong q shape
    assert call(p=e(m, l - 1)) == INVALID and call(p=e(m + 1, l)) == INVALID                       # wrong p shape
    overl = lambda r, c: torch.zeros((2, r, c), dtype=torch.complex128, device="cuda").as_strided((2, r, c), (r * c - 1, c, 1))  # noqa: E731
    assert call(q=overl(l, n)) == INVALID and call(p=overl(m, l)) == INVALID and call(y=overl(l, n)) == INVALID  # overlapping / short output strides
    assert call(q=overl(l, n), count=1) == 0                                                       # one block: no stride to check
    with pytest.raises(AssertionError, match="sketch_range_step_complex_batched"):                 # the messages carry the call's own name
        ctx.check(call(count=-1))
    # a null required pointer (the shape fields are right)
    fn = _lib.lib().rc_sketch_range_step_complex_batched_c64
    v = lambda t: (_lib.mat(t[0]), ctypes.c_int64(t.stride(0)))  # noqa: E731
    nullmat = lambda r, c: (_lib.rc_matrix(None, r, c, c, 1), ctypes.c_int64(r * c))  # noqa: E731
    none = (_lib.mat(None), ctypes.c_int64(0))
    a0, om0, q0, p0 = e(m, n), e(l, m), e(l, n), e(m, l)
    good = dict(a=v(a0), om=v(om0), q=v(q0), p=v(p0), ranks=_lib.i64p(ranks))
    zero = ctypes.c_int32(0)
    for name, null in (("a", nullmat(m, n)), ("om", nullmat(l, m)), ("q", nullmat(l, n)), ("p", nullmat(m, l)), ("ranks", None)):
        g = dict(good, **{name: null})
        assert fn(ctx._h, *g["a"], *g["om"], ctypes.c_int32(2), *none, *g["q"], *g["p"], g["ranks"], zero) == INVALID, name
    assert fn(ctx._h, *v(a0), *v(om0), ctypes.c_int32(2), *none, *v(q0), *v(p0), _lib.i64p(ranks), zero) == 0
    assert fn(None, *v(a0), *v(om0), ctypes.c_int32(2), *none, *v(q0), *v(p0), _lib.i64p(ranks), zero) == INVALID  # null context
    # count = 0: nothing to do, correctly shaped empty results
    assert call(count=0) == 0
    out = rc.sketch_range_step_batched_complex(torch.zeros((0, 30, 20), dtype=torch.complex64, device="cuda"), k=8, return_sketch=True)
    assert [tuple(t.shape) for t in out] == [(0, 16, 20), (0, 30, 16), (0,), (0, 16, 20)]
    # dtype and rank errors of the wrappers: real data, mismatched dtypes; the real functions keep rejecting complex data
    real = torch.zeros((2, 30, 20), dtype=torch.float64, device="cuda")
    cplx = torch.zeros((2, 30, 20), dtype=torch.complex128, device="cuda")
    with pytest.raises(TypeError):
        rc.sketch_range_step_batched_complex(real, k=4)
    with pytest.raises(TypeError):
        rc.sketch_power_omega_batched_complex(real, 4, 1)
    for its in (0, 1):
        with pytest.raises(TypeError):
            rc.sketch_column_id_rank_power_batched_complex(real, 4, power_iterations=its)
        with pytest.raises(TypeError):
            rc.sketch_svd_rank_power_batched_complex(real, 4, power_iterations=its)
        with pytest.raises(TypeError):
            rc.sketch_column_id_rank_power_batched(cplx, 4, power_iterations=its)
    with pytest.raises(TypeError):
        rc.sketch_range_step_batched(cplx, k=4)
    with pytest.raises(TypeError):
        rc.sketch_range_step_batched_complex(cplx, torch.zeros((6, 30), dtype=torch.complex64, device="cuda"))
    with pytest.raises(TypeError):
        rc.sketch_range_step_batched_complex(cplx, torch.zeros((6, 30), dtype=torch.float64, device="cuda"))
    with pytest.raises(AssertionError):
        rc.sketch_range_step_batched_complex(torch.zeros((30, 20), dtype=torch.complex128, device="cuda"), k=4)
    with pytest.raises(AssertionError, match="sketch_range_step_complex_batched"):  # RC_INVALID_ARGUMENT: l = 12 > n = 10
        rc.sketch_range_step_batched_complex(torch.zeros((1, 30, 10), dtype=torch.complex128, device="cuda"), k=4)
    # a lazily conjugated view is materialised: the result is that of the conjugated values
    rng = np.random.default_rng(12)
    x, om = tt(cgauss(rng, (2, 50, 20))), tt(cgauss(rng, (8, 50)))
    for w, g in zip(rc.sketch_range_step_batched_complex(x.conj(), om.conj()), rc.sketch_range_step_batched_complex(x.conj().resolve_conj(), om.conj().resolve_conj())):
        assert same_bits(npy(w), npy(g))
    torch.cuda.synchronize()
    assert ctx.get_health() == 0


def test_cpp_example_runs(tmp_path):
    """tests/cpp/batched_range_step_complex_example.cpp through include/rusty_compression.hpp: every check of the example passes."""
    exe = build_cpp_mirror_examples(tmp_path, "batched_range_step_complex_example.cpp")
    res = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=dict(os.environ))
    print(res.stdout)
    assert res.returncode == 0 and "ALL OK" in res.stdout, res.stdout + res.stderr
