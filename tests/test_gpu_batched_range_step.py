"""Batched range step (rc_sketch_range_step_batched_*, batch.sketch_range_step_batched) and the power-iterated sketched column ID and
SVD built on it (batch.sketch_power_omega_batched, sketch_column_id_rank_power_batched, sketch_svd_rank_power_batched).

Per block one round of the reference's sample_range_power_iteration (src/random_sampling.rs:131-158): the sketch Y = omega a, an
orthonormal basis Q of Y's rows (pivoted Householder QR of Y^T) and the projection P = a Q^T.  Checked: y against the sketched ID's y
bit for bit; Q against LAPACK's Q of the device's own Y in the same precision (SciPy's pivoted qr of Y^T), by orthonormality
||Q_r Q_r^T - I||_F and span ||Y - (Y Q_r^T) Q_r||_F / ||Y||_F; P against the f64 host product with the device's own Q under the
dot-product bound of the sketch test, |p - a Q^T| <= c (n + 4) u (|a| |Q^T|), c = 1 (f32) or 2 (f64); the compositions against the host
model of tests/range_step_ref.py with the same omega; and the contract of the batch (layouts, views, count and position, neighbours, graph
replay, ranks, non-finite input, argument checks).

Yardstick of the basis: both Q's are products of l Householder reflectors applied with an error of a few u each; ours applies them to
one unit vector per wave with a 64-lane tree sum, LAPACK's ?orgqr in blocks, so the constants differ but not the order.  The device's
figure must stay within QR_MARGIN = 4 times LAPACK's plus a floor of sqrt(l) u (LAPACK's own figure is 0 on a 1-row Y and a few u on the
smallest shapes, where a ratio alone means nothing).  Measured on an MI355X, worst over the shapes below: orthonormality 1.55 times
LAPACK's figure in f64 and 1.13 in f32, span 1.32 in f64 and 1.26 in f32 (on most blocks the device's figure is the smaller one); the
projection uses at most 0.096 of its bound in f32 and 0.067 in f64 (the larger f64 shapes agree with the host product exactly).  The
power-iterated ID and SVD agree with the host model's error to five digits on all three accuracy shapes in both precisions (ID
1.4457e-01, 3.1931e-02, 8.9773e-02 against 2.8050e-01, 8.7328e-02, 2.2748e-01 in one pass: ratios 0.52, 0.37, 0.39)."""
import ctypes
import re

import numpy as np
import pytest
import scipy.linalg
import torch

import rusty_compression_amd as rc
from rusty_compression_amd import _lib
from tests import range_step_ref as ref
from tests.helpers import TOL, npy

pytestmark = pytest.mark.gpu

DTYPES = [np.float64, np.float32]
QR_MARGIN = 4.0
# (m, n, l): nothing a multiple of 16 / 32 / 64; the two accuracy shapes; l = 128 with the working copy out of LDS; l = n; l = 1
SHAPES = [(70, 33, 17), (1030, 300, 40), (600, 130, 24), (520, 130, 128), (96, 96, 96), (40, 64, 1)]


def tt(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def step(a, omega, want_y=True):
    """The call on device tensors; numpy results (q, p, ranks[, y])."""
    out = rc.sketch_range_step_batched(a, omega, return_sketch=want_y)
    torch.cuda.synchronize()
    return tuple(npy(t) for t in out)


def same_bits(x, y):
    x, y = np.asarray(x), np.asarray(y)
    return x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes()  # bytes: a NaN equals itself, -0.0 is not 0.0


def launch_label(fn):
    """fn() under the default context's event profile: (fn's result, the fields of the one op:batched_range_step label it recorded)."""
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
    mt = re.fullmatch(r"op:batched_range_step (\d+)x(\d+) l=(\d+) count=(\d+) grid=(\d+) slots=(\d+) plan=(\S+)", labels[0][0])
    assert mt, labels[0][0]
    f = dict(zip(("m", "n", "l", "count", "grid", "slots"), map(int, mt.groups()[:6])))
    f["plan"] = mt.group(7)
    return out, f


def raw(fn_dtype, a, omega, y, q, p, ranks, ctx=None, count=None):
    """One raw call on 3-D device views (omega 2-D: shared, batch stride 0; y None: not requested); returns the status."""
    ctx = ctx or _lib.default_context()
    fn = getattr(_lib.lib(), f"rc_sketch_range_step_batched_{_lib.suffix(fn_dtype)}")

    def view(t):
        if t is None:
            return _lib.mat(None), ctypes.c_int64(0)
        if t.dim() == 2:
            return _lib.rc_matrix(t.data_ptr(), t.shape[0], t.shape[1], t.stride(0), t.stride(1)), ctypes.c_int64(0)
        return _lib.rc_matrix(t.data_ptr(), t.shape[1], t.shape[2], t.stride(1), t.stride(2)), ctypes.c_int64(t.stride(0))

    return fn(ctx._h, *view(a), *view(omega), ctypes.c_int32(a.shape[0] if count is None else count), *view(y), *view(q), *view(p), _lib.i64p(ranks))


_DATA = {}


def data(m, n, l, dtype):
    """Two blocks per shape, one Gaussian and one with the decaying spectrum of the sketch tests, and a shared Gaussian omega (made once)."""
    key = (m, n, l, np.dtype(dtype))
    if key not in _DATA:
        rng = np.random.default_rng(1000 * m + 10 * n + l)
        dec = ref.decaying(m + n, m, n) if min(m, n) >= 2 else rng.standard_normal((m, n))
        _DATA[key] = (np.stack([rng.standard_normal((m, n)), dec]).astype(dtype), rng.standard_normal((l, m)).astype(dtype))
    return _DATA[key]


def basis_figures(y, q, r):
    """(||Q_r Q_r^T - I||_F, ||Y - (Y Q_r^T) Q_r||_F / ||Y||_F) in f64 for the rows 0 .. r-1 of q (l x n)."""
    y64, q64 = y.astype(np.float64), q[:r].astype(np.float64)
    return np.linalg.norm(q64 @ q64.T - np.eye(r)), np.linalg.norm(y64 - (y64 @ q64.T) @ q64) / np.linalg.norm(y64)


# ---------------------------------------------------------------- 1. one step against the host, on every shape edge
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m,n,l", SHAPES)
def test_one_step_against_the_host(m, n, l, dtype):
    a, om = data(m, n, l, dtype)
    ad, omd = tt(a), tt(om)
    (q, p, ranks, y), lab = launch_label(lambda: step(ad, omd))
    assert (lab["m"], lab["n"], lab["l"], lab["count"]) == (m, n, l, 2)
    out_of_lds = (m, n, l) == (520, 130, 128) and dtype == np.float64
    assert lab["plan"].startswith("W:ws,Q:ws," if out_of_lds else "W:")
    assert q.shape == (2, l, n) and p.shape == (2, m, l) and y.shape == (2, l, n) and q.dtype == p.dtype == np.dtype(dtype)
    # the sketch is the sketched ID's, bit for bit, and the other outputs do not depend on whether it is written
    y_id = npy(rc.sketch_column_id_rank_batched(ad, min(l, 128), 0.0, omega=omd, return_sketch=True)[4])
    assert same_bits(y, y_id)
    for g, w in zip((q, p, ranks), step(ad, omd, want_y=False)):
        assert same_bits(g, w)
    u = np.finfo(dtype).eps / 2
    cst = 1.0 if dtype == np.float32 else 2.0
    for i in range(2):
        r = int(ranks[i])
        assert r == l  # full-rank data: no exactly zero pivot
        # the basis against LAPACK's on the device's own Y in the same precision
        lq = scipy.linalg.qr(y[i].T, mode="economic", pivoting=True)[0].T
        assert lq.dtype == np.dtype(dtype)
        orth, span = basis_figures(y[i], q[i], r)
        lorth, lspan = basis_figures(y[i], lq, r)
        floor = np.sqrt(l) * u
        print(f"step {m}x{n} l={l} {np.dtype(dtype).name} block {i}: orth {orth:.3e} lapack {lorth:.3e} ratio {orth / max(lorth, floor):.2f}; "
              f"span {span:.3e} lapack {lspan:.3e} ratio {span / max(lspan, floor):.2f}")
        assert orth <= QR_MARGIN * lorth + floor
        assert span <= QR_MARGIN * lspan + floor
        # the projection against the f64 host product with the device's own Q
        a64, q64 = a[i].astype(np.float64), q[i].astype(np.float64)
        bound = cst * (n + 4) * u * (np.abs(a64) @ np.abs(q64.T))
        err = np.abs(p[i].astype(np.float64) - a64 @ q64.T)
        print(f"    projection: max |p - a q^T| / bound = {float(np.max(err / np.maximum(bound, np.finfo(np.float64).tiny))):.3e}")
        assert np.all(err <= bound)


# ---------------------------------------------------------------- 2. layouts and views
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_layouts_and_views_give_the_contiguous_bits(dtype):
    """Every layout of a and of omega, hence each of the kernel's four instances per dtype, gives the contiguous call's bits; so do a
    per-block omega and strided outputs."""
    rng = np.random.default_rng(5)
    cnt, m, n, l = 6, 150, 70, 20
    base = tt(rng.standard_normal((cnt, m, n))).to(dtype)
    om = tt(rng.standard_normal((l, m))).to(dtype)
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
    # a different omega per block = count calls with count = 1
    oms = tt(rng.standard_normal((cnt, l, m))).to(dtype)
    got = step(base, oms)
    for i in range(cnt):
        for o, g in zip(step(base[i:i + 1], oms[i]), got):
            assert same_bits(o[0], g[i])
    # strided q, p and y: the gaps keep their 7.0; p column-major inside its block
    qb = torch.full((cnt, l + 2, n + 3), 7.0, dtype=base.dtype, device="cuda")
    pb = torch.full((cnt, l + 1, m + 4), 7.0, dtype=base.dtype, device="cuda")
    yb = torch.full((cnt, l + 2, n + 1), 7.0, dtype=base.dtype, device="cuda")
    ranks = torch.empty(cnt, dtype=torch.int64, device="cuda")
    qv, pv, yv = qb[:, :l, :n], pb[:, :l, :m].transpose(1, 2), yb[:, :l, :n]
    assert raw(dtype, base, om, yv, qv, pv, ranks) == 0
    torch.cuda.synchronize()
    for w, g in zip(want, (qv, pv, ranks, yv)):
        assert same_bits(w, npy(g.contiguous()))
    for buf, rows, cols in ((qb, l, n), (pb, l, m), (yb, l, n)):
        gaps = torch.ones_like(buf, dtype=torch.bool)
        gaps[:, :rows, :cols] = False
        assert bool((buf[gaps] == 7.0).all())


# ---------------------------------------------------------------- 3. bits independent of count, position, strides and neighbours
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_bits_independent_of_count_position_and_neighbours(dtype):
    rng = np.random.default_rng(6)
    m, n, l = 100, 48, 20
    om = tt(rng.standard_normal((l, m))).to(dtype)
    protos = [rng.standard_normal((m, n)), ref.decaying(3, m, n), 1e-3 * rng.standard_normal((m, n)),
              rng.standard_normal((m, 5)) @ rng.standard_normal((5, n)), np.full((m, n), np.nan), np.zeros((m, n)),
              rng.standard_normal((m, 1)) @ rng.standard_normal((1, n))]
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


# ---------------------------------------------------------------- 4. graph replay
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_graph_replay_gives_the_eager_bits(dtype):
    rng = np.random.default_rng(7)
    cnt, m, n, l = 33, 300, 64, 20
    lib = _lib.lib()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        a = tt(rng.standard_normal((cnt, m, n))).to(dtype)
        om = tt(rng.standard_normal((l, m))).to(dtype)
        eager = step(a, om)
        ctx = _lib.Context(torch.cuda.current_device(), st.cuda_stream)
        q = torch.zeros((cnt, l, n), dtype=a.dtype, device="cuda")
        p = torch.zeros((cnt, m, l), dtype=a.dtype, device="cuda")
        y = torch.zeros((cnt, l, n), dtype=a.dtype, device="cuda")
        ranks = torch.zeros(cnt, dtype=torch.int64, device="cuda")
        st.synchronize()
        assert raw(dtype, a, om, y, q, p, ranks, ctx=ctx) == 0  # eager once: sizes the workspace
        ctx.synchronize()
        ctx.get_health()
        for t in (q, p, y, ranks):
            t.zero_()
        st.synchronize()
        graph = ctypes.c_void_p(None)
        ctx.check(lib.rc_graph_begin_capture(ctx._h))
        ctx.check(raw(dtype, a, om, y, q, p, ranks, ctx=ctx))  # one launch: the capture has no parallel branches
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


# ---------------------------------------------------------------- 5. ranks
@pytest.mark.parametrize("dtype", DTYPES)
def test_zero_and_exactly_rank_deficient_blocks(dtype):
    rng = np.random.default_rng(8)
    m, n, l = 90, 40, 12
    # small integers: a of exact rank 5 and an integer omega, so that Y = omega a is formed without rounding and has exact rank 5
    low = (rng.integers(-3, 4, (m, 5)) @ rng.integers(-3, 4, (5, n))).astype(dtype)
    om = rng.integers(-2, 3, (l, m)).astype(dtype)
    a = np.stack([np.zeros((m, n), dtype=dtype), low, rng.standard_normal((m, n)).astype(dtype)])
    q, p, ranks, y = step(tt(a), tt(om))
    assert np.array_equal(y[1].astype(np.float64), om.astype(np.float64) @ low.astype(np.float64)) and np.linalg.matrix_rank(y[1].astype(np.float64)) == 5
    assert ranks[0] == 0 and not np.any(q[0]) and not np.any(p[0]) and not np.any(y[0])
    assert 5 <= ranks[1] <= l and ranks[2] == l
    print(f"exact rank 5 block {np.dtype(dtype).name}: r = {int(ranks[1])}")
    for i in range(3):
        r = int(ranks[i])
        assert not np.any(q[i][r:]) and not np.any(p[i][:, r:])
        if r:
            orth, span = basis_figures(y[i], q[i], r)
            assert orth <= 100 * l * np.finfo(dtype).eps and span <= 100 * l * np.finfo(dtype).eps


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_non_finite_input_stays_in_its_block(dtype):
    rng = np.random.default_rng(9)
    cnt, m, n, l = 12, 130, 70, 30
    clean = tt(rng.standard_normal((cnt, m, n))).to(dtype)
    om = tt(rng.standard_normal((l, m))).to(dtype)
    want = step(clean, om)
    bad = clean.clone()
    bad[4, 17, 23] = float("nan")
    bad[8, 99, 5] = float("inf")
    got = step(bad, om)
    for i in range(cnt):
        assert 0 <= got[2][i] <= l
        if i in (4, 8):
            continue
        for w, g in zip(want, got):
            assert same_bits(w[i], g[i])


# ---------------------------------------------------------------- 6. the compositions against the host model
_MODEL = {}


def model_case(case, dtype, sigma_min=1e-10):
    """The block and the omega of one accuracy case in `dtype` (made once); the host model runs on exactly these values."""
    key = (case, np.dtype(dtype), sigma_min)
    if key not in _MODEL:
        m, n, l, k = case
        a = ref.decaying(m + n, m, n, sigma_min).astype(dtype)
        om = ref.gaussian(m + n + l, l, m).astype(dtype)
        _MODEL[key] = (a, om)
    return _MODEL[key]


def rel_err(a, approx):
    a64 = a.astype(np.float64)
    return np.linalg.norm(a64 - approx) / np.linalg.norm(a64)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", ref.DECAY_CASES)
def test_power_iterated_id_against_the_host_model(case, dtype):
    m, n, l, k = case
    a, om = model_case(case, dtype)
    ad, omd = tt(a[None]), tt(om)
    errs = []
    for its in (0, 1):
        c, z, ind, ranks = (npy(t) for t in rc.sketch_column_id_rank_power_batched(ad, k, 0.0, power_iterations=its, omega=omd))
        assert ranks[0] == k and np.array_equal(c[0], a[:, ind[0][:k]])
        errs.append(rel_err(a, c[0].astype(np.float64) @ z[0].astype(np.float64)))
    oerr = ref.column_id_power(a, om, k, 0.0, 1)[0]
    print(f"power ID {m}x{n} l={l} k={k} {np.dtype(dtype).name}: q=0 {errs[0]:.4e} q=1 {errs[1]:.4e} ratio {errs[1] / errs[0]:.3f}; host q=1 {oerr:.4e}")
    assert errs[1] <= 1.5 * oerr + 100 * np.finfo(dtype).eps
    assert errs[1] <= 0.75 * errs[0]


@pytest.mark.parametrize("dtype", DTYPES)
def test_tolerance_example_reaches_the_models_rank(dtype):
    m, n, l, k = ref.TOL_CASE
    a, om = model_case(ref.TOL_CASE, dtype, ref.TOL_SIGMA_MIN)
    _, orank, ratios = ref.column_id_power(a, om, k, ref.TOL, 1)
    assert np.min(np.abs(ratios / ref.TOL - 1.0)) > 1e-6  # no ratio of the model within 1e-6 (relative) of the tolerance
    ranks = npy(rc.sketch_column_id_rank_power_batched(tt(a[None]), k, ref.TOL, power_iterations=1, omega=tt(om))[3])
    print(f"tolerance example {np.dtype(dtype).name}: rank {int(ranks[0])}, host model {orank}")
    assert ranks[0] == orank == min(k, l, n)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", ref.DECAY_CASES)
def test_power_iterated_svd_against_the_host_model(case, dtype):
    m, n, l, k = case
    a, om = model_case(case, dtype)
    u, s, vt, ranks = (npy(t) for t in rc.sketch_svd_rank_power_batched(tt(a[None]), k, 0.0, power_iterations=1, omega=tt(om)))
    assert u.shape == (1, m, k) and vt.shape == (1, k, n) and ranks[0] == k
    u0, s0, vt0 = u[0].astype(np.float64), s[0][:k].astype(np.float64), vt[0].astype(np.float64)
    orth = max(np.abs(u0.T @ u0 - np.eye(k)).max(), np.abs(vt0 @ vt0.T - np.eye(k)).max())
    err = rel_err(a, (u0 * s0) @ vt0)
    oerr, orank = ref.svd_power(a, om, k, 0.0, 1)
    print(f"power SVD {m}x{n} l={l} k={k} {np.dtype(dtype).name}: err {err:.4e} host {oerr:.4e}; orth {orth:.3e} bound {4 * TOL[np.dtype(dtype)]['orth']:.3e}")
    assert orank == k
    assert orth <= 4 * TOL[np.dtype(dtype)]["orth"]
    assert np.all(np.diff(s0) <= 0) and s0[-1] > 0
    assert err <= 1.5 * oerr + 100 * np.finfo(dtype).eps


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_no_iterations_is_the_one_pass_call_and_the_chain_is_the_calls_by_hand(dtype):
    rng = np.random.default_rng(11)
    cnt, m, n, k = 3, 200, 40, 10
    a = tt(rng.standard_normal((cnt, m, n))).to(dtype)
    om = tt(rng.standard_normal((k + 6, m))).to(dtype)
    for kw in (dict(omega=om), dict(seed=5, oversampling=4)):
        for w, g in zip(rc.sketch_column_id_rank_batched(a, k, 1e-6, return_sketch=True, **kw),
                        rc.sketch_column_id_rank_power_batched(a, k, 1e-6, power_iterations=0, return_sketch=True, **kw)):
            assert same_bits(npy(w), npy(g))
        for w, g in zip(rc.sketch_svd_rank_batched(a, k, 1e-6, **kw), rc.sketch_svd_rank_power_batched(a, k, 1e-6, power_iterations=0, **kw)):
            assert same_bits(npy(w), npy(g))
    # the default omega is the sketched ID's; one iteration is the range step, the tall recompression with right = I and the sketched ID
    q, p, ranks = rc.sketch_range_step_batched(a, k=k, oversampling=4, seed=5)
    l = k + 4
    q2, p2, ranks2 = rc.sketch_range_step_batched(a, rc.random_gaussian((l, m), rc.Rng(5), dtype))
    for w, g in ((q, q2), (p, p2), (ranks, ranks2)):
        assert same_bits(npy(w), npy(g))
    eye = torch.eye(l, dtype=dtype, device="cuda").expand(cnt, l, l)
    uu = rc.lowrank_recompress_tall_batched(p, eye, l, 0.0, ranks=ranks)[0]
    omq = rc.sketch_power_omega_batched(a, k, 1, oversampling=4, seed=5)
    assert omq.shape == (cnt, l, m) and same_bits(npy(omq.contiguous()), npy(uu.mT.contiguous()))
    gram = npy(omq).astype(np.float64)
    assert np.abs(gram @ gram.transpose(0, 2, 1) - np.eye(l)).max() <= 4 * TOL[np.dtype(npy(omq).dtype)]["orth"]
    for w, g in zip(rc.sketch_column_id_rank_batched(a, k, 1e-6, omega=uu.mT), rc.sketch_column_id_rank_power_batched(a, k, 1e-6, oversampling=4, seed=5)):
        assert same_bits(npy(w), npy(g))
    two = rc.sketch_svd_rank_power_batched(a, k, 1e-6, power_iterations=2, oversampling=4, seed=5)
    q3, p3, ranks3 = rc.sketch_range_step_batched(a, uu.mT)
    for w, g in zip(rc.lowrank_recompress_tall_batched(p3, q3, k, 1e-6, ranks=ranks3), two):
        assert same_bits(npy(w), npy(g))
    torch.cuda.synchronize()


# ---------------------------------------------------------------- 7. arguments, count = 0, dtype errors
def test_argument_checks_count_zero_and_dtype_errors():
    INVALID = 5
    ctx = _lib.default_context()
    ctx.get_health()
    e = lambda r, c: torch.zeros((2, r, c), dtype=torch.float64, device="cuda")  # noqa: E731
    ranks = torch.empty(2, dtype=torch.int64, device="cuda")
    m, n, l = 60, 30, 12

    def call(a=None, om=None, y=None, q=None, p=None, ranks=ranks, count=2):
        a = e(m, n) if a is None else a
        om = e(l, m)[0] if om is None else om
        q = e(l, n) if q is None else q
        p = e(m, l) if p is None else p
        return raw(torch.float64, a, om, y, q, p, ranks, count=count)

    def shaped(t, rows, cols):  # a small allocation whose shape fields alone say rows x cols
        return t.as_strided((2, rows, cols), (1, 0, 0))

    assert call() == 0
    assert call(y=e(l, n)) == 0
    small = e(4, 4)
    assert call(om=e(31, m)[0], q=e(31, n), p=e(m, 31)) == INVALID                                 # l = 31 > n = 30
    assert call(a=e(10, n), om=e(l, 10)[0], p=e(10, l)) == INVALID                                 # l = 12 > m = 10
    assert call(a=shaped(small, 200, 200), om=shaped(small, 129, 200)[0], q=shaped(small, 129, 200), p=shaped(small, 200, 129)) == INVALID  # l = 129
    assert call(a=shaped(small, m, 513), q=shaped(small, l, 513)) == INVALID                       # n = 513
    assert call(a=shaped(small, 65537, n), om=shaped(small, l, 65537)[0], p=shaped(small, 65537, l)) == INVALID  # m = 65537
    assert call(count=-1) == INVALID
    assert call(om=e(l, m + 1)[0]) == INVALID                                                      # omega.cols != a.rows
    assert call(y=e(l + 1, n)) == INVALID and call(y=e(l, n - 1)) == INVALID                       # wrong y shape
    assert call(q=e(l, n + 1)) == INVALID and call(q=e(l + 1, n)) == INVALID                       # wrong q shape
    assert call(p=e(m, l - 1)) == INVALID and call(p=e(m + 1, l)) == INVALID                       # wrong p shape
    overl = lambda r, c: torch.zeros((2, r, c), dtype=torch.float64, device="cuda").as_strided((2, r, c), (r * c - 1, c, 1))  # noqa: E731
    assert call(q=overl(l, n)) == INVALID and call(p=overl(m, l)) == INVALID and call(y=overl(l, n)) == INVALID  # overlapping / short output strides
    assert call(q=overl(l, n), count=1) == 0                                                       # one block: no stride to check
    # a null required pointer (the shape fields are right)
    fn = _lib.lib().rc_sketch_range_step_batched_f64
    v = lambda t: (_lib.mat(t[0]), ctypes.c_int64(t.stride(0)))  # noqa: E731
    nullmat = lambda r, c: (_lib.rc_matrix(None, r, c, c, 1), ctypes.c_int64(r * c))  # noqa: E731
    none = (_lib.mat(None), ctypes.c_int64(0))
    a0, om0, q0, p0 = e(m, n), e(l, m), e(l, n), e(m, l)
    good = dict(a=v(a0), om=v(om0), q=v(q0), p=v(p0), ranks=_lib.i64p(ranks))
    for name, null in (("a", nullmat(m, n)), ("om", nullmat(l, m)), ("q", nullmat(l, n)), ("p", nullmat(m, l)), ("ranks", None)):
        g = dict(good, **{name: null})
        assert fn(ctx._h, *g["a"], *g["om"], ctypes.c_int32(2), *none, *g["q"], *g["p"], g["ranks"]) == INVALID, name
    assert fn(ctx._h, *v(a0), *v(om0), ctypes.c_int32(2), *none, *v(q0), *v(p0), _lib.i64p(ranks)) == 0
    assert fn(None, *v(a0), *v(om0), ctypes.c_int32(2), *none, *v(q0), *v(p0), _lib.i64p(ranks)) == INVALID  # null context
    # count = 0: nothing to do, correctly shaped empty results
    assert call(count=0) == 0
    out = rc.sketch_range_step_batched(torch.zeros((0, 30, 20), dtype=torch.float32, device="cuda"), k=8, return_sketch=True)
    assert [tuple(t.shape) for t in out] == [(0, 16, 20), (0, 30, 16), (0,), (0, 16, 20)]
    # dtype and rank errors of the wrappers
    cplx = torch.zeros((2, 30, 20), dtype=torch.complex128, device="cuda")
    with pytest.raises(TypeError):
        rc.sketch_range_step_batched(cplx, k=4)
    with pytest.raises(TypeError):
        rc.sketch_power_omega_batched(cplx, 4, 1)
    for its in (0, 1):
        with pytest.raises(TypeError):
            rc.sketch_column_id_rank_power_batched(cplx, 4, power_iterations=its)
        with pytest.raises(TypeError):
            rc.sketch_svd_rank_power_batched(cplx, 4, power_iterations=its)
    with pytest.raises(TypeError):
        rc.sketch_range_step_batched(torch.zeros((2, 30, 20), dtype=torch.float64, device="cuda"), torch.zeros((6, 30), dtype=torch.float32, device="cuda"))
    with pytest.raises(AssertionError):
        rc.sketch_range_step_batched(torch.zeros((30, 20), dtype=torch.float64, device="cuda"), k=4)
    with pytest.raises(AssertionError, match="sketch_range_step_batched"):  # RC_INVALID_ARGUMENT: l = 12 > n = 10
        rc.sketch_range_step_batched(torch.zeros((1, 30, 10), dtype=torch.float64, device="cuda"), k=4)
    torch.cuda.synchronize()
    assert ctx.get_health() == 0
