"""Apply and rebuild batched IDs and SVDs in one rank-aware launch (rc_lowrank_apply_batched_*, batch.lowrank_apply_batched and its
named wrappers): the reference's Apply::dot and to_mat (src/col_interp_decomp.rs:63-65, :134-154,
src/two_sided_interp_decomp.rs:62-65, :159-170, src/svd.rs:42-55) for the outputs of the batched calls.

Accuracy yardstick (derived, not measured): the reference is NumPy in float64 / complex128 on the first r columns and rows of the
factors, and elementwise |y - y_ref| <= (n + 2k + 4) c u E with E = |left[:, :r]| |mid[:r, :r]| diag(|s[:r]|) |right[:r]| |b| (absent
factors omitted), u the unit roundoff of the dtype and c = 1 for real, 4 for complex data: the standard bound gamma_p |A| |B| of a
product of inner dimension p summed in any order, chained over the at most n + k + k terms of the three products plus the scaling."""
import ctypes

import numpy as np
import pytest
import torch

import rusty_compression_amd as rc
from oracle import ref_lapack as o
from rusty_compression_amd import _lib
from tests.helpers import batched_launch, npy

pytestmark = pytest.mark.gpu

INVALID = 5
DTYPES = [np.float64, np.float32, np.complex128, np.complex64]
SHAPES = [(37, 29, 16, 5), (130, 70, 48, 1), (65, 512, 128, 3), (512, 33, 7, 40)]  # (m, n, k, nrhs)


def unit_roundoff(dtype):
    return np.finfo(np.dtype(dtype)).eps / 2


def rand(rng, shape, dtype):
    x = rng.standard_normal(shape)
    if np.iscomplexobj(np.zeros(0, dtype=dtype)):
        x = x + 1j * rng.standard_normal(shape)
    return x.astype(dtype)


def real_of(dtype):
    return np.zeros(0, dtype=dtype).real.dtype


def factors(rng, count, m, n, k, nrhs, dtype, mid=True, s=True):
    f = dict(left=rand(rng, (count, m, k), dtype), right=rand(rng, (count, k, n), dtype), b=rand(rng, (count, n, nrhs), dtype))
    f["mid"] = rand(rng, (count, k, k), dtype) if mid else None
    f["s"] = np.abs(rng.standard_normal((count, k + 3))).astype(real_of(dtype)) + 0.1 if s else None  # p = k + 3 > k: read with stride p
    return f


def mixed_ranks(count, k):
    base = [0, 1, k, k // 2, max(k - 1, 0), min(2, k), k // 3, k]
    return np.array([base[i % len(base)] for i in range(count)], dtype=np.int64)


def reference(left, right, b=None, mid=None, s=None, ranks=None):
    """(y_ref, E) in float64 / complex128 on the first r columns and rows (the rest masked to exact zeros, which changes no sum)."""
    count, m, k = left.shape
    cplx = np.iscomplexobj(left)
    wide = np.complex128 if cplx else np.float64
    r = np.full(count, k) if ranks is None else np.clip(np.asarray(ranks), 0, k)
    keep = (np.arange(k)[None, :] < r[:, None])
    lw = left.astype(wide) * keep[:, None, :]
    rw = right.astype(wide) * keep[:, :, None]
    y, e = rw, np.abs(rw)
    if b is not None:
        bw = b.astype(wide)
        if bw.ndim == 2:
            bw = bw[:, :, None]
        y, e = y @ bw, e @ np.abs(bw)
    if s is not None:
        sw = np.where(keep, s[:, :k].astype(np.float64), 0.0)
        y, e = sw[:, :, None] * y, np.abs(sw)[:, :, None] * e
    if mid is not None:
        mw = mid.astype(wide) * keep[:, None, :] * keep[:, :, None]
        y, e = mw @ y, np.abs(mw) @ e
    y, e = lw @ y, np.abs(lw) @ e
    if b is not None and b.ndim == 2:
        y, e = y[:, :, 0], e[:, :, 0]
    return y, e


def bound_of(e, n, k, dtype):
    c = 4 if np.iscomplexobj(np.zeros(0, dtype=dtype)) else 1
    return (n + 2 * k + 4) * c * unit_roundoff(dtype) * e


def dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def apply(left, right, b=None, mid=None, s=None, ranks=None):
    y = rc.lowrank_apply_batched(dev(left) if isinstance(left, np.ndarray) else left, dev(right) if isinstance(right, np.ndarray) else right,
                                 b=dev(b) if isinstance(b, np.ndarray) else b, mid=dev(mid) if isinstance(mid, np.ndarray) else mid,
                                 s=dev(s) if isinstance(s, np.ndarray) else s, ranks=dev(ranks) if isinstance(ranks, np.ndarray) else ranks)
    torch.cuda.synchronize()
    return npy(y)


def check(y, left, right, b, mid, s, ranks, dtype, slack=1.0):
    n, k = right.shape[2], left.shape[2]
    ref, e = reference(left, right, b, mid, s, ranks)
    assert y.shape == ref.shape and y.dtype == np.dtype(dtype)
    assert np.all(np.isfinite(y))
    err, bnd = np.abs(y.astype(ref.dtype) - ref), slack * bound_of(e, n, k, dtype)
    worst = float((err / np.maximum(bnd, np.finfo(np.float64).tiny)).max()) if err.size else 0.0
    print(f"max |y - y_ref| / bound = {worst:.3e}")
    assert np.all(err <= bnd), worst


# ---------------------------------------------------------------- 1. parity on hand-made random factors
@pytest.mark.parametrize("with_mid,with_s", [(False, False), (True, False), (False, True), (True, True)])
@pytest.mark.parametrize("m,n,k,nrhs", SHAPES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_parity_on_random_factors(dtype, m, n, k, nrhs, with_mid, with_s):
    rng = np.random.default_rng(m * 7 + n * 3 + k + 2 * with_mid + with_s)
    count = 8
    f = factors(rng, count, m, n, k, nrhs, dtype, with_mid, with_s)
    ranks = mixed_ranks(count, k)
    y = apply(f["left"], f["right"], f["b"], f["mid"], f["s"], ranks)
    check(y, f["left"], f["right"], f["b"], f["mid"], f["s"], ranks, dtype)
    assert not np.any(y[ranks == 0])
    rec = apply(f["left"], f["right"], None, f["mid"], f["s"], ranks)
    assert rec.shape == (count, m, n)
    check(rec, f["left"], f["right"], None, f["mid"], f["s"], ranks, dtype)
    vec = f["b"][:, :, 0]
    yv = apply(f["left"], f["right"], vec, f["mid"], f["s"], ranks)
    assert yv.shape == (count, m)
    check(yv, f["left"], f["right"], vec, f["mid"], f["s"], ranks, dtype)
    # the bits of a column do not depend on how many right-hand sides travel with it
    assert np.array_equal(yv, y[:, :, 0])


def test_mixed_dtypes_raise():
    rng = np.random.default_rng(0)
    f = factors(rng, 2, 9, 8, 4, 2, np.float64)
    with pytest.raises(TypeError):
        rc.lowrank_apply_batched(dev(f["left"]), dev(f["right"].astype(np.float32)))
    with pytest.raises(TypeError):
        rc.lowrank_apply_batched(dev(f["left"]), dev(f["right"]), b=dev(f["b"].astype(np.complex128)))
    with pytest.raises(TypeError):
        rc.lowrank_apply_batched(dev(f["left"]), dev(f["right"]), s=dev(f["s"].astype(np.float32)))


# ---------------------------------------------------------------- 2. several units per workgroup
@pytest.mark.parametrize("dtype", [np.float64, np.complex64])
def test_several_units_per_workgroup(dtype):
    m, n, k, nrhs = SHAPES[0]
    rng = np.random.default_rng(2)
    one = factors(rng, 1, m, n, k, nrhs, dtype)
    _, probe = batched_launch(lambda: apply(one["left"], one["right"], one["b"], one["mid"], one["s"], np.array([k // 2], dtype=np.int64)))
    assert probe["op"].startswith("batched_apply") and (probe["m"], probe["n"], probe["k"], probe["count"]) == (m, n, k, 1)
    count = probe["slots"] + 3
    f = factors(rng, count, m, n, k, nrhs, dtype)
    ranks = mixed_ranks(count, k)
    ranks[0], ranks[-1] = k // 2, k - 1
    y, lab = batched_launch(lambda: apply(f["left"], f["right"], f["b"], f["mid"], f["s"], ranks))
    assert lab["count"] == count and lab["grid"] == lab["slots"] < count  # some workgroups take a second unit
    check(y, f["left"], f["right"], f["b"], f["mid"], f["s"], ranks, dtype)
    for i in (0, count - 1):
        alone = apply(*(None if f[name] is None else f[name][i:i + 1] for name in ("left", "right", "b", "mid", "s")), ranks[i:i + 1])
        assert np.array_equal(alone[0], y[i])


# ---------------------------------------------------------------- 3. tails are never read
@pytest.mark.parametrize("layout", ["c_order", "column_major"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_tails_are_never_read(dtype, layout):
    m, n, k, nrhs = 130, 70, 48, 5
    rng = np.random.default_rng(3)
    count = 8
    f = factors(rng, count, m, n, k, nrhs, dtype)
    ranks = mixed_ranks(count, k)
    dirty = {name: f[name].copy() for name in ("left", "right", "mid", "s")}
    for i, r in enumerate(ranks):
        dirty["left"][i, :, r:] = np.nan
        dirty["right"][i, r:, :] = np.nan
        dirty["mid"][i, r:, :] = np.nan
        dirty["mid"][i, :, r:] = np.nan
        dirty["s"][i, r:] = np.nan

    def lay(x):
        t = dev(x)
        return t.transpose(1, 2).contiguous().transpose(1, 2) if layout == "column_major" and t.dim() == 3 else t

    for b in (f["b"], None):
        clean = apply(lay(f["left"]), lay(f["right"]), b, lay(f["mid"]), f["s"], ranks)
        got = apply(lay(dirty["left"]), lay(dirty["right"]), b, lay(dirty["mid"]), dirty["s"], ranks)
        assert np.all(np.isfinite(got))
        assert np.array_equal(got, clean)
        check(got, f["left"], f["right"], b, f["mid"], f["s"], ranks, dtype)


# ---------------------------------------------------------------- 4. ranks handling
@pytest.mark.parametrize("dtype", [np.float64, np.complex128])
def test_ranks_none_and_clamping(dtype):
    m, n, k, nrhs = SHAPES[0]
    rng = np.random.default_rng(4)
    count = 5
    f = factors(rng, count, m, n, k, nrhs, dtype)
    full = apply(f["left"], f["right"], f["b"], f["mid"], f["s"], np.full(count, k, dtype=np.int64))
    assert np.array_equal(apply(f["left"], f["right"], f["b"], f["mid"], f["s"], None), full)
    odd = np.array([-3, k + 9, 4, -3, k + 9], dtype=np.int64)
    clamped = np.array([0, k, 4, 0, k], dtype=np.int64)
    got = apply(f["left"], f["right"], f["b"], f["mid"], f["s"], odd)
    assert np.array_equal(got, apply(f["left"], f["right"], f["b"], f["mid"], f["s"], clamped))
    assert not np.any(got[0]) and np.array_equal(got[1], full[1])


# ---------------------------------------------------------------- 5. layouts
def _raw(left, right, y_view, ybs, count, b=None, mid=None, s=None, ranks=None, ctx=None, dtype=torch.float64):
    """The C entry point on [count, rows, cols] tensors (views of block 0 + batch strides); y_view is an rc_matrix."""
    ctx = ctx or _lib.default_context()

    def view(t):
        if t is None:
            return _lib.mat(None), ctypes.c_int64(0)
        return _lib.rc_matrix(t.data_ptr(), t.shape[1], t.shape[2], t.stride(1), t.stride(2)), ctypes.c_int64(t.stride(0))

    fn = getattr(_lib.lib(), f"rc_lowrank_apply_batched_{_lib.suffix(dtype)}")
    return fn(ctx._h, *view(left), *view(mid), ctypes.c_void_p(s.data_ptr() if s is not None else None),
              ctypes.c_int64(s.stride(0) if s is not None else 0), *view(right), _lib.i64p(ranks), ctypes.c_int32(count), *view(b), y_view,
              ctypes.c_int64(ybs))


@pytest.mark.parametrize("dtype", [np.float64, np.complex64])
def test_column_major_factors_and_shared_b(dtype):
    m, n, k, nrhs = 130, 70, 48, 5
    rng = np.random.default_rng(5)
    count = 6
    f = factors(rng, count, m, n, k, nrhs, dtype)
    ranks = mixed_ranks(count, k)
    cm = lambda x: dev(x).transpose(1, 2).contiguous().transpose(1, 2)  # noqa: E731
    for b in (f["b"], None):
        y = apply(cm(f["left"]), cm(f["right"]), None if b is None else cm(b), cm(f["mid"]), f["s"], ranks)
        check(y, f["left"], f["right"], b, f["mid"], f["s"], ranks, dtype)
    shared = dev(f["b"][2:3]).expand(count, n, nrhs)
    assert shared.stride(0) == 0
    got = apply(f["left"], f["right"], shared, f["mid"], f["s"], ranks)
    copies = np.repeat(f["b"][2:3], count, axis=0)
    assert np.array_equal(got, apply(f["left"], f["right"], copies, f["mid"], f["s"], ranks))
    check(got, f["left"], f["right"], copies, f["mid"], f["s"], ranks, dtype)


def test_padded_y_keeps_its_sentinels():
    m, n, k, nrhs = SHAPES[0]
    rng = np.random.default_rng(6)
    count = 7
    f = factors(rng, count, m, n, k, nrhs, np.float64)
    ranks = mixed_ranks(count, k)
    t = {name: dev(f[name]) for name in ("left", "right", "b", "mid", "s")}
    tr = dev(ranks)
    ref = apply(t["left"], t["right"], t["b"], t["mid"], t["s"], tr)
    sentinel = -12345.5
    for recon in (False, True):
        cols = n if recon else nrhs
        want = apply(t["left"], t["right"], None, t["mid"], t["s"], tr) if recon else ref
        big = torch.full((count, m + 3, cols + 5), sentinel, dtype=torch.float64, device="cuda")
        inner = big[:, 1:m + 1, 2:cols + 2]
        yv = _lib.rc_matrix(inner.data_ptr(), m, cols, inner.stride(1), inner.stride(2))
        assert _raw(t["left"], t["right"], yv, inner.stride(0), count, None if recon else t["b"], t["mid"], t["s"], tr) == 0
        torch.cuda.synchronize()
        out = npy(big)
        assert np.array_equal(out[:, 1:m + 1, 2:cols + 2], want)
        mask = np.ones(out.shape, dtype=bool)
        mask[:, 1:m + 1, 2:cols + 2] = False
        assert np.all(out[mask] == sentinel)


@pytest.mark.parametrize("form", ["column_id", "two_sided_id", "svd"])
@pytest.mark.parametrize("dtype", [np.float64, np.complex128])
def test_transposed_apply_through_swapped_views(dtype, form):
    """A^T x (not conjugated) is the same call on left = right^T, right = left^T (and mid^T) as strided views: A = C Z, C X R or
    U diag(s) Vt, so A^T = Z^T C^T, R^T X^T C^T or Vt^T diag(s) U^T."""
    m, n, k, nrhs = 130, 70, 48, 3
    rng = np.random.default_rng(7)
    count = 6
    f = factors(rng, count, m, n, k, nrhs, dtype, mid=form == "two_sided_id", s=form == "svd")
    ranks = mixed_ranks(count, k)
    x = rand(rng, (count, m, nrhs), dtype)
    left_t, right_t = dev(f["right"]).transpose(1, 2), dev(f["left"]).transpose(1, 2)  # strided views, nothing copied
    mid_t = None if f["mid"] is None else dev(f["mid"]).transpose(1, 2)
    y = apply(left_t, right_t, x, mid_t, f["s"], ranks)
    assert y.shape == (count, n, nrhs)
    a, ea = reference(f["left"], f["right"], None, f["mid"], f["s"], ranks)  # NumPy's A and |C| |X| |S| |R|
    ref = a.transpose(0, 2, 1) @ x.astype(a.dtype)
    e = ea.transpose(0, 2, 1) @ np.abs(x).astype(np.float64)
    assert np.all(np.abs(y - ref) <= bound_of(e, m, k, dtype))  # the chain's inner sizes are m, k, k here


# ---------------------------------------------------------------- 6. graph capture
def test_graph_capture_replays_the_eager_bits():
    m, n, k, nrhs = 96, 128, 24, 5
    rng = np.random.default_rng(8)
    count = 33
    f = factors(rng, count, m, n, k, nrhs, np.float64)
    lib = _lib.lib()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        t = {name: dev(f[name]) for name in ("left", "right", "b", "mid", "s")}
        tr = dev(mixed_ranks(count, k))
        eager = apply(t["left"], t["right"], t["b"], t["mid"], t["s"], tr)
        ctx = _lib.Context(torch.cuda.current_device(), st.cuda_stream)
        y = torch.zeros((count, m, nrhs), dtype=torch.float64, device="cuda")
        st.synchronize()
        args = (t["left"], t["right"], _lib.mat(y[0]), m * nrhs, count, t["b"], t["mid"], t["s"], tr)
        graph = ctypes.c_void_p(None)
        ctx.check(lib.rc_graph_begin_capture(ctx._h))
        assert _raw(*args, ctx=ctx) == 0
        ctx.check(lib.rc_graph_end_capture(ctx._h, ctypes.byref(graph)))
        try:
            st.synchronize()
            assert not np.any(npy(y))  # captured, not run
            ctx.check(lib.rc_graph_launch(ctx._h, graph))
            ctx.synchronize()
            assert np.array_equal(npy(y), eager)
        finally:
            ctx.check(lib.rc_graph_destroy(ctx._h, graph))
            ctx.close()


# ---------------------------------------------------------------- 7. end to end through the batched factorizations
def _decaying_batch(dtype):
    rng = np.random.default_rng(9)
    count, m, n = 24, 96, 80
    mats = []
    for i in range(count):  # singular values 1 .. 10^-(10 + i): s_j / s_0 crosses tol = 1e-6 at j = 47 (cut to k) down to j = 14
        x = o.random_approximate_low_rank_matrix((m, n), 1.0, 10.0 ** -(10 + i), rng)
        if np.iscomplexobj(np.zeros(0, dtype=dtype)):  # the same singular values behind a random unitary factor
            x = x @ np.linalg.qr(rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n)))[0]
        mats.append(x.astype(dtype))
    return np.stack(mats), rand(rng, (count, n, 6), dtype)


@pytest.mark.parametrize("dtype", [np.float64, np.float32, np.complex128])
@pytest.mark.parametrize("kind", ["column_id", "two_sided_id", "svd"])
def test_end_to_end(kind, dtype):
    a, b = _decaying_batch(dtype)
    k, tol = 32, 1e-6
    ta, tb = dev(a), dev(b)
    if kind == "column_id":
        c, z, _, ranks = rc.column_id_rank_batched(ta, k, tol)
        named = lambda rhs: rc.column_id_apply_batched(c, z, ranks, rhs)  # noqa: E731
        parts = dict(left=c, right=z, mid=None, s=None)
    elif kind == "two_sided_id":
        c, x, r, _, _, ranks = rc.two_sided_id_rank_batched(ta, k, tol)
        named = lambda rhs: rc.two_sided_id_apply_batched(c, x, r, ranks, rhs)  # noqa: E731
        parts = dict(left=c, right=r, mid=x, s=None)
    else:
        svd = rc.svd_rank_batched_complex if np.iscomplexobj(a) else rc.svd_rank_batched
        u, s, vt, ranks = svd(ta, k, tol)
        named = lambda rhs: rc.svd_apply_batched(u, s, vt, ranks, rhs)  # noqa: E731
        parts = dict(left=u, right=vt, mid=None, s=s)
    torch.cuda.synchronize()
    h = {name: None if t is None else npy(t) for name, t in parts.items()}
    hr = npy(ranks)
    assert hr.max() == k and 1 <= hr.min() < k - 8  # the batch mixes blocks cut at k with blocks the tolerance stops well below it
    rec, yb = npy(named(None)), npy(named(tb))
    torch.cuda.synchronize()
    check(rec, h["left"], h["right"], None, h["mid"], h["s"], hr, dtype)
    check(yb, h["left"], h["right"], b, h["mid"], h["s"], hr, dtype)
    # apply(b) against to_mat() @ b, within twice the bound
    wide = np.complex128 if np.iscomplexobj(a) else np.float64
    _, e = reference(h["left"], h["right"], b, h["mid"], h["s"], hr)
    assert np.all(np.abs(yb.astype(wide) - rec.astype(wide) @ b.astype(wide)) <= 2 * bound_of(e, a.shape[2], k, dtype))
    # and the factors do describe the matrices: s_32 / s_0 <= 1e-4 for every block, times the IDs' growth
    assert np.linalg.norm(rec - a) / np.linalg.norm(a) <= 1e-2


# ---------------------------------------------------------------- 8. argument checks
def test_argument_checks():
    e = lambda c, r, q: torch.zeros((c, r, q), dtype=torch.float64, device="cuda")  # noqa: E731
    ranks = torch.zeros(2, dtype=torch.int64, device="cuda")
    s = torch.ones((2, 16), dtype=torch.float64, device="cuda")
    m, n, k, nrhs = 40, 30, 16, 3

    def call(left=None, right=None, b=None, mid=None, y=None, ybs=None, count=2, recon=False):
        left = e(2, m, k) if left is None else left
        right = e(2, k, n) if right is None else right
        b = None if recon else (e(2, n, nrhs) if b is None else b)
        y = e(2, m, n if recon else nrhs) if y is None else y
        return _raw(left, right, _lib.mat(y[0]), y.stride(0) if ybs is None else ybs, count, b, mid, s, ranks)

    sentinel = torch.full((2, m, nrhs), 7.0, dtype=torch.float64, device="cuda")
    assert call(right=e(2, k + 1, n), y=sentinel) == INVALID                      # left.cols != right.rows
    assert "right" in _lib.lib().rc_last_error_message(_lib.default_context()._h).decode()
    assert call(mid=e(2, k, k + 1), y=sentinel) == INVALID                        # mid not k x k
    assert call(mid=e(2, k - 1, k), y=sentinel) == INVALID
    assert call(b=e(2, n + 1, nrhs), y=sentinel) == INVALID                       # b.rows != n
    assert call(y=e(2, m, nrhs + 1)) == INVALID                                   # y not m x nrhs
    assert call(y=e(2, m + 1, nrhs)) == INVALID
    assert call(y=e(2, m, nrhs), recon=True) == INVALID                           # y not m x n when reconstructing
    assert call(left=e(2, m, 129), right=e(2, 129, n), y=sentinel) == INVALID     # k = 129
    assert call(left=e(2, 513, k), y=e(2, 513, nrhs)) == INVALID                  # m = 513
    assert call(right=e(2, k, 513), b=e(2, 513, nrhs), y=sentinel) == INVALID     # n = 513
    assert call(y=sentinel, ybs=m * nrhs - 1) == INVALID                          # the y of two blocks overlap
    assert call(y=sentinel, count=-1) == INVALID
    null = torch.zeros((2, m, k), dtype=torch.float64, device="cuda")
    fn = _lib.lib().rc_lowrank_apply_batched_f64
    none, zero = _lib.mat(None), ctypes.c_int64(0)
    lv = _lib.rc_matrix(None, m, k, k, 1)  # a null left with the right shape
    assert fn(_lib.default_context()._h, lv, ctypes.c_int64(m * k), none, zero, None, zero, _lib.mat(e(2, k, n)[0]), ctypes.c_int64(k * n), None,
              ctypes.c_int32(2), _lib.mat(e(2, n, nrhs)[0]), ctypes.c_int64(n * nrhs), _lib.mat(sentinel[0]), ctypes.c_int64(m * nrhs)) == INVALID
    yv = _lib.rc_matrix(None, m, nrhs, nrhs, 1)  # a null y
    assert _raw(null, e(2, k, n), yv, m * nrhs, 2, e(2, n, nrhs)) == INVALID
    assert call(left=torch.ones((2, m, k), dtype=torch.float64, device="cuda"), right=torch.ones((2, k, n), dtype=torch.float64, device="cuda"),
                b=torch.ones((2, n, nrhs), dtype=torch.float64, device="cuda"), y=sentinel, count=0) == 0  # count = 0: nothing to do
    torch.cuda.synchronize()
    assert torch.all(sentinel == 7.0)  # no rejected call, and not the empty one, wrote anything
    with pytest.raises(AssertionError, match="lowrank_apply_batched"):  # RC_INVALID_ARGUMENT: the reference asserts
        rc.lowrank_apply_batched(e(1, 600, 8), e(1, 8, 20))
    y = rc.lowrank_apply_batched(torch.zeros((0, 30, 8), dtype=torch.float32, device="cuda"), torch.zeros((0, 8, 20), dtype=torch.float32, device="cuda"))
    assert y.shape == (0, 30, 20)
