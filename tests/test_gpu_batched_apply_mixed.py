"""Apply batches from factors stored in f32 / c32 under f64 / c64 arithmetic (rc_lowrank_apply_mixed_batched_f64 / _c64,
batch.lowrank_apply_batched_mixed) and the batched conversions that produce such factors (rc_demote_batched_*, rc_promote_batched_*).

The contract is bit-equality with the full-precision call on promoted factors, so most tests compare with np.array_equal.  Two bounds
are derived, not measured:
  * against NumPy on the promoted factors, the full-precision suite's yardstick (n + 2k + 4) c u_T E (tests/test_gpu_batched_apply.py);
  * against NumPy on the original f64 / c128 factors, that yardstick plus the storage rounding q u32 (1 + 2 u32) E: each of the q
    demoted factors of the chain (2, or 3 with mid) carries a relative error of at most u32 = 2^-24 per element (componentwise for a
    complex element, hence also in modulus), and (1 + u)^q - 1 <= q u (1 + 2u) for q <= 3."""
import ctypes

import numpy as np
import pytest
import torch

import rusty_compression_amd as rc
from rusty_compression_amd import _lib
from tests.helpers import batched_launch, npy
from tests.test_gpu_batched_apply import SHAPES, bound_of, dev, factors, mixed_ranks, rand, reference

pytestmark = pytest.mark.gpu

INVALID = 5
WIDE = [np.float64, np.complex128]
NARROW = {np.float64: np.float32, np.complex128: np.complex64}
U32 = 2.0 ** -24
FACTORS = ("left", "right", "mid")


def stored(f, dtype):
    """The factors of f in storage precision (NumPy's rounding, not the library's) and their exact promotion; b and s stay wide."""
    low = dict(f)
    for name in FACTORS:
        low[name] = None if f[name] is None else f[name].astype(NARROW[dtype])
    up = dict(low)
    for name in FACTORS:
        up[name] = None if low[name] is None else low[name].astype(dtype)
    return low, up


def to_dev(x):
    return dev(x) if isinstance(x, np.ndarray) else x


def mixed(f, b="b", ranks=None):
    y = rc.lowrank_apply_batched_mixed(to_dev(f["left"]), to_dev(f["right"]), b=to_dev(f[b]) if isinstance(b, str) else to_dev(b), mid=to_dev(f["mid"]),
                                       s=to_dev(f["s"]), ranks=to_dev(ranks))
    torch.cuda.synchronize()
    return npy(y)


def full(f, b="b", ranks=None):
    y = rc.lowrank_apply_batched(to_dev(f["left"]), to_dev(f["right"]), b=to_dev(f[b]) if isinstance(b, str) else to_dev(b), mid=to_dev(f["mid"]),
                                 s=to_dev(f["s"]), ranks=to_dev(ranks))
    torch.cuda.synchronize()
    return npy(y)


def within(y, ref, bnd, what):
    err = np.abs(y - ref)
    worst = float((err / np.maximum(bnd, np.finfo(np.float64).tiny)).max()) if err.size else 0.0
    print(f"{what}: max |y - y_ref| / bound = {worst:.3e}")
    assert np.all(np.isfinite(y)) and np.all(err <= bnd), (what, worst)


# ---------------------------------------------------------------- 1. the bits of the full-precision call, and two derived bounds
@pytest.mark.parametrize("with_mid,with_s", [(False, False), (True, False), (False, True), (True, True)])
@pytest.mark.parametrize("m,n,k,nrhs", SHAPES)
@pytest.mark.parametrize("dtype", WIDE)
def test_bits_of_the_full_precision_call(dtype, m, n, k, nrhs, with_mid, with_s):
    rng = np.random.default_rng(m * 7 + n * 3 + k + 2 * with_mid + with_s)
    count = 8
    f = factors(rng, count, m, n, k, nrhs, dtype, with_mid, with_s)
    ranks = mixed_ranks(count, k)
    low, up = stored(f, dtype)
    vec = f["b"][:, :, 0]
    for b in (f["b"], vec, None):  # a matrix, a vector, to_mat
        got = mixed(low, b, ranks)
        assert got.dtype == np.dtype(dtype) and got.shape == (count, m) + (() if b is vec else (n if b is None else nrhs,))
        assert np.array_equal(got, full(up, b, ranks))
        assert not np.any(got[ranks == 0])
        # parity independent of the library's own apply: NumPy on the promoted factors
        ref, e = reference(up["left"], up["right"], b, up["mid"], up["s"], ranks)
        within(got, ref, bound_of(e, n, k, dtype), "promoted factors")


@pytest.mark.parametrize("with_mid,with_s", [(False, False), (True, False), (False, True), (True, True)])
@pytest.mark.parametrize("m,n,k,nrhs", SHAPES)
@pytest.mark.parametrize("dtype", WIDE)
def test_storage_rounding(dtype, m, n, k, nrhs, with_mid, with_s):
    rng = np.random.default_rng(m * 5 + n * 11 + k + 2 * with_mid + with_s)
    count = 8
    f = factors(rng, count, m, n, k, nrhs, dtype, with_mid, with_s)
    ranks = mixed_ranks(count, k)
    low = dict(f)
    for name in FACTORS:
        low[name] = None if f[name] is None else rc.demote_batched(dev(f[name]))
        assert low[name] is None or np.array_equal(npy(low[name]), f[name].astype(NARROW[dtype]))
    q = 3 if with_mid else 2
    for b in (f["b"], None):
        got = mixed(low, b, ranks)
        ref, e = reference(f["left"], f["right"], b, f["mid"], f["s"], ranks)  # the ORIGINAL factors
        within(got, ref, bound_of(e, n, k, dtype) + q * U32 * (1 + 2 * U32) * e, "original factors")


# ---------------------------------------------------------------- 2. layouts: the rows-fast path
@pytest.mark.parametrize("layout", ["column_major", "transposed"])
@pytest.mark.parametrize("dtype", WIDE)
def test_rows_fast_views(dtype, layout):
    m, n, k, nrhs = 130, 70, 48, 5
    rng = np.random.default_rng(21)
    count = 8
    f = factors(rng, count, m, n, k, nrhs, dtype)
    ranks = mixed_ranks(count, k)
    low, up = stored(f, dtype)
    if layout == "column_major":
        lay = lambda x: dev(x).transpose(1, 2).contiguous().transpose(1, 2)  # noqa: E731
        vl = {name: lay(low[name]) for name in FACTORS}
        vu = {name: lay(up[name]) for name in FACTORS}
        rhs = f["b"]
    else:  # A^T x through swapped, transposed views of the C-order factors: nothing is copied
        vl = dict(left=dev(low["right"]).transpose(1, 2), right=dev(low["left"]).transpose(1, 2), mid=dev(low["mid"]).transpose(1, 2))
        vu = dict(left=dev(up["right"]).transpose(1, 2), right=dev(up["left"]).transpose(1, 2), mid=dev(up["mid"]).transpose(1, 2))
        rhs = rand(rng, (count, m, nrhs), dtype)
    assert all(t.stride(1) < t.stride(2) for t in vl.values())
    vl["s"] = vu["s"] = f["s"]
    for b in (rhs, rhs[:, :, 0], None):
        assert np.array_equal(mixed(vl, b, ranks), full(vu, b, ranks))


# ---------------------------------------------------------------- 3. tails are never read
@pytest.mark.parametrize("layout", ["c_order", "column_major"])
@pytest.mark.parametrize("dtype", WIDE)
def test_tails_are_never_read(dtype, layout):
    m, n, k, nrhs = 130, 70, 48, 5
    rng = np.random.default_rng(3)
    count = 8
    f = factors(rng, count, m, n, k, nrhs, dtype)
    ranks = mixed_ranks(count, k)
    low, up = stored(f, dtype)
    dirty = {name: low[name].copy() for name in FACTORS}
    dirty.update(s=f["s"].copy(), b=f["b"])
    for i, r in enumerate(ranks):
        dirty["left"][i, :, r:] = np.nan
        dirty["right"][i, r:, :] = np.nan
        dirty["mid"][i, r:, :] = np.nan
        dirty["mid"][i, :, r:] = np.nan
        dirty["s"][i, r:] = np.nan

    def lay(g):
        cm = lambda x: dev(x).transpose(1, 2).contiguous().transpose(1, 2)  # noqa: E731
        return {name: (cm(v) if layout == "column_major" and name in FACTORS else v) for name, v in g.items()}

    for b in (f["b"], None):
        got = mixed(lay(dirty), b, ranks)
        assert np.all(np.isfinite(got))
        assert np.array_equal(got, mixed(lay(low), b, ranks))
        assert np.array_equal(got, full(lay(up), b, ranks))


# ---------------------------------------------------------------- 4. several units per workgroup; a block's bits do not depend on count
@pytest.mark.parametrize("dtype", WIDE)
def test_several_units_per_workgroup(dtype):
    m, n, k, nrhs = SHAPES[0]
    rng = np.random.default_rng(2)
    one, _ = stored(factors(rng, 1, m, n, k, nrhs, dtype), dtype)
    _, probe = batched_launch(lambda: mixed(one, "b", np.array([k // 2], dtype=np.int64)))
    tag = "<complex,mixed>" if dtype is np.complex128 else "<mixed>"
    assert probe["op"] == "batched_apply" + tag and (probe["m"], probe["n"], probe["k"], probe["count"]) == (m, n, k, 1)
    count = probe["slots"] + 3
    low, up = stored(factors(rng, count, m, n, k, nrhs, dtype), dtype)
    ranks = mixed_ranks(count, k)
    ranks[0], ranks[-1] = k // 2, k - 1
    t = {name: dev(low[name]) for name in ("left", "right", "mid", "s", "b")}
    tr = dev(ranks)
    y, lab = batched_launch(lambda: mixed(t, "b", tr))
    assert lab["count"] == count and lab["grid"] == lab["slots"] < count  # some workgroups take a second unit
    assert np.array_equal(y, full(up, "b", ranks))
    alone = torch.cat([rc.lowrank_apply_batched_mixed(t["left"][i:i + 1], t["right"][i:i + 1], b=t["b"][i:i + 1], mid=t["mid"][i:i + 1],
                                                      s=t["s"][i:i + 1], ranks=tr[i:i + 1]) for i in range(count)])
    torch.cuda.synchronize()
    assert np.array_equal(npy(alone), y)


# ---------------------------------------------------------------- 5. graph capture
def _raw(left, right, y_view, ybs, count, b=None, mid=None, s=None, ranks=None, ctx=None, dtype=torch.float64):
    """The C entry point on [count, rows, cols] tensors (views of block 0 + batch strides); y_view is an rc_matrix; dtype is the wide one."""
    ctx = ctx or _lib.default_context()

    def view(t):
        if t is None:
            return _lib.mat(None), ctypes.c_int64(0)
        return _lib.rc_matrix(t.data_ptr(), t.shape[1], t.shape[2], t.stride(1), t.stride(2)), ctypes.c_int64(t.stride(0))

    fn = getattr(_lib.lib(), f"rc_lowrank_apply_mixed_batched_{_lib.suffix(dtype)}")
    return fn(ctx._h, *view(left), *view(mid), ctypes.c_void_p(s.data_ptr() if s is not None else None),
              ctypes.c_int64(s.stride(0) if s is not None else 0), *view(right), _lib.i64p(ranks), ctypes.c_int32(count), *view(b), y_view,
              ctypes.c_int64(ybs))


@pytest.mark.parametrize("dtype", WIDE)
def test_graph_capture_replays_the_eager_bits(dtype):
    m, n, k, nrhs = 96, 128, 24, 5
    rng = np.random.default_rng(8)
    count = 33
    low, _ = stored(factors(rng, count, m, n, k, nrhs, dtype), dtype)
    lib = _lib.lib()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        t = {name: dev(low[name]) for name in ("left", "right", "b", "mid", "s")}
        tr = dev(mixed_ranks(count, k))
        eager = mixed(t, "b", tr)
        ctx = _lib.Context(torch.cuda.current_device(), st.cuda_stream)
        y = torch.zeros((count, m, nrhs), dtype=t["b"].dtype, device="cuda")
        st.synchronize()
        args = (t["left"], t["right"], _lib.mat(y[0]), m * nrhs, count, t["b"], t["mid"], t["s"], tr)
        graph = ctypes.c_void_p(None)
        ctx.check(lib.rc_graph_begin_capture(ctx._h))
        assert _raw(*args, ctx=ctx, dtype=t["b"].dtype) == 0
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


# ---------------------------------------------------------------- 6. argument checks
def test_dtype_combinations_raise():
    rng = np.random.default_rng(0)
    f = factors(rng, 2, 9, 8, 4, 2, np.float64)
    low, _ = stored(f, np.float64)
    t = {name: dev(low[name]) for name in ("left", "right", "mid", "s", "b")}
    with pytest.raises(TypeError, match="lowrank_apply_batched"):  # all-f64 factors: the message names the same-dtype call
        rc.lowrank_apply_batched_mixed(dev(f["left"]), dev(f["right"]), b=t["b"])
    with pytest.raises(TypeError):
        rc.lowrank_apply_batched_mixed(t["left"], t["right"], b=t["b"].float())
    with pytest.raises(TypeError):
        rc.lowrank_apply_batched_mixed(t["left"], t["right"], b=t["b"], s=t["s"].float())
    with pytest.raises(TypeError):
        rc.lowrank_apply_batched_mixed(t["left"], dev(f["right"]), b=t["b"])           # one factor wide
    with pytest.raises(TypeError):
        rc.lowrank_apply_batched_mixed(t["left"], t["right"], b=t["b"].to(torch.complex128))
    with pytest.raises(TypeError):
        rc.lowrank_apply_batched_mixed(t["left"].to(torch.complex64), t["right"].to(torch.complex64), b=t["b"])  # c32 factors want a c128 b
    with pytest.raises(TypeError):
        rc.demote_batched(t["left"])
    with pytest.raises(TypeError):
        rc.promote_batched(dev(f["left"]))


def test_out_of_domain_is_invalid():
    e = lambda c, r, q, dt=torch.float32: torch.zeros((c, r, q), dtype=dt, device="cuda")  # noqa: E731
    w = lambda c, r, q: e(c, r, q, torch.float64)  # noqa: E731
    ranks = torch.zeros(2, dtype=torch.int64, device="cuda")
    s = torch.ones((2, 16), dtype=torch.float64, device="cuda")
    m, n, k, nrhs = 40, 30, 16, 3

    def call(left=None, right=None, b=None, mid=None, y=None, ybs=None, count=2, recon=False):
        left = e(2, m, k) if left is None else left
        right = e(2, k, n) if right is None else right
        b = None if recon else (w(2, n, nrhs) if b is None else b)
        y = w(2, m, n if recon else nrhs) if y is None else y
        return _raw(left, right, _lib.mat(y[0]), y.stride(0) if ybs is None else ybs, count, b, mid, s, ranks)

    sentinel = torch.full((2, m, nrhs), 7.0, dtype=torch.float64, device="cuda")
    assert call(right=e(2, k + 1, n), y=sentinel) == INVALID                      # left.cols != right.rows
    assert "lowrank_apply_batched" in _lib.lib().rc_last_error_message(_lib.default_context()._h).decode()  # the twin's message
    assert call(mid=e(2, k, k + 1), y=sentinel) == INVALID                        # mid not k x k
    assert call(b=w(2, n + 1, nrhs), y=sentinel) == INVALID                       # b.rows != n
    assert call(y=w(2, m, nrhs + 1)) == INVALID                                   # y not m x nrhs
    assert call(y=w(2, m, nrhs), recon=True) == INVALID                           # y not m x n when reconstructing
    assert call(left=e(2, m, 129), right=e(2, 129, n), y=sentinel) == INVALID     # k = 129
    assert call(left=e(2, 513, k), y=w(2, 513, nrhs)) == INVALID                  # m = 513
    assert call(right=e(2, k, 513), b=w(2, 513, nrhs), y=sentinel) == INVALID     # n = 513
    assert call(y=sentinel, ybs=m * nrhs - 1) == INVALID                          # the y of two blocks overlap
    assert call(y=sentinel, count=-1) == INVALID
    yv = _lib.rc_matrix(None, m, nrhs, nrhs, 1)  # a null y
    assert _raw(e(2, m, k), e(2, k, n), yv, m * nrhs, 2, w(2, n, nrhs)) == INVALID
    assert call(left=torch.ones((2, m, k), dtype=torch.float32, device="cuda"), right=torch.ones((2, k, n), dtype=torch.float32, device="cuda"),
                b=torch.ones((2, n, nrhs), dtype=torch.float64, device="cuda"), y=sentinel, count=0) == 0  # count = 0: nothing to do
    torch.cuda.synchronize()
    assert torch.all(sentinel == 7.0)  # no rejected call, and not the empty one, wrote anything
    with pytest.raises(AssertionError, match="lowrank_apply_batched"):  # RC_INVALID_ARGUMENT: the reference asserts
        rc.lowrank_apply_batched_mixed(e(1, 600, 8), e(1, 8, 20))
    y = rc.lowrank_apply_batched_mixed(e(0, 30, 8), e(0, 8, 20))
    assert y.shape == (0, 30, 20) and y.dtype == torch.float64


# ---------------------------------------------------------------- 7. demote and promote
def _planted(dtype):
    """A strided [3, 70, 33] view (a slice of a larger array in both matrix dimensions, batch stride with a gap) holding the edge values of
    the conversion, and the number of finite elements per block that overflow f32."""
    rng = np.random.default_rng(13)
    cplx = dtype is np.complex128
    big = rand(rng, (3, 75, 2 * 33 + 4), dtype)
    view = big[:, 2:72, 1:67:2]
    assert view.shape == (3, 70, 33) and not view.flags["C_CONTIGUOUS"]
    tie_even = 1.0 + 2.0 ** -24          # halfway between 1 and 1 + 2^-23: rounds to the even neighbour, 1
    tie_odd = 1.0 + 3 * 2.0 ** -24       # halfway between 1 + 2^-23 and 1 + 2^-22: rounds up to the even neighbour
    edge = [1e-40, -1e-42, 2.0 ** -150, 0.0, -0.0, 1e300, -1e300, tie_even, tie_odd, np.nan, 3.4028235677973366e38, np.inf]
    #       subnormal results   below half the smallest subnormal -> 0     overflow       ties                 f32 max + half an ulp -> inf
    overflow = np.zeros(3, dtype=np.int64)
    for blk in range(3):
        for j, v in enumerate(edge):
            view[blk, 5 + blk, j] = v
            if cplx:  # the same values in the imaginary part of other elements
                view[blk, 40 + blk, j] = 1j * v if np.isfinite(v) else complex(0.5, v)
        finite_to_inf = 3  # 1e300, -1e300, f32 max + half an ulp (inf itself is not finite, NaN neither)
        overflow[blk] = finite_to_inf * (2 if cplx else 1)
    view[1, 60, 7] = 1e39  # one more in block 1 only
    overflow[1] += 1
    if cplx:
        view[2, 61, 3] = complex(1e300, -1e300)  # one element, both parts overflow: counted once
        overflow[2] += 1
    return big, view, overflow


@pytest.mark.parametrize("dtype", WIDE)
def test_demote_matches_astype_and_counts_overflow(dtype):
    big, view, overflow = _planted(dtype)
    tbig = dev(big)
    tview = tbig[:, 2:72, 1:67:2]
    assert tuple(tview.stride()) == tuple(s // big.itemsize for s in view.strides)
    low, ovf = rc.demote_batched(tview, return_overflow=True)
    torch.cuda.synchronize()
    with np.errstate(over="ignore"):
        want = view.astype(NARROW[dtype])
    got = npy(low)
    assert got.dtype == want.dtype and got.shape == want.shape
    real = np.float32
    g, w = got.view(real), want.view(real)
    nan = np.isnan(w)
    assert nan.any() and np.array_equal(np.isnan(g), nan)                      # NaN by mask
    assert np.array_equal(g.view(np.uint32)[~nan], w.view(np.uint32)[~nan])    # everything else by bits: -0, subnormals, ties, +-inf
    assert np.array_equal(npy(ovf), overflow)
    assert np.array_equal(npy(rc.demote_batched(tview)), got, equal_nan=True)  # without the count: the same values


@pytest.mark.parametrize("dtype", WIDE)
def test_promote_is_exact_and_inverts_demote(dtype):
    rng = np.random.default_rng(14)
    big = rand(rng, (3, 75, 70), NARROW[dtype])
    big[1, 9, 5] = 1e-40   # an f32 subnormal
    big[2, 9, 7] = -0.0
    tview = dev(big)[:, 2:72, 1:67:2]
    up = rc.promote_batched(tview)
    torch.cuda.synchronize()
    want = big[:, 2:72, 1:67:2].astype(dtype)
    assert up.dtype == dev(want).dtype
    assert np.array_equal(npy(up).view(np.uint64), want.view(np.uint64))
    back, ovf = rc.demote_batched(up, return_overflow=True)  # promote then demote of f32-representable data is the identity
    torch.cuda.synchronize()
    assert np.array_equal(npy(back).view(np.uint32), np.ascontiguousarray(big[:, 2:72, 1:67:2]).view(np.uint32))
    assert not np.any(npy(ovf))


def test_convert_argument_checks():
    lib = _lib.lib()
    h = _lib.default_context()._h
    src = torch.ones((2, 6, 5), dtype=torch.float64, device="cuda")
    dst = torch.full((2, 6, 5), 7.0, dtype=torch.float32, device="cuda")
    i64 = ctypes.c_int64

    def demote(sv, dv, dbs=30, count=2):
        return lib.rc_demote_batched_f64(h, sv, i64(30), ctypes.c_int32(count), dv, i64(dbs), None)

    assert demote(_lib.mat(src[0]), _lib.mat(dst[0, :, :4])) == INVALID            # shapes differ
    assert demote(_lib.mat(src[0]), _lib.mat(dst[0]), dbs=29) == INVALID            # two blocks of dst overlap
    assert demote(_lib.mat(src[0]), _lib.mat(dst[0]), count=-1) == INVALID
    assert demote(_lib.rc_matrix(None, 6, 5, 5, 1), _lib.mat(dst[0])) == INVALID   # null src
    assert demote(_lib.rc_matrix(src.data_ptr(), 65537, 1, 1, 1), _lib.rc_matrix(dst.data_ptr(), 65537, 1, 1, 1)) == INVALID
    assert demote(_lib.mat(src[0]), _lib.mat(dst[0]), count=0) == 0                 # nothing to do
    torch.cuda.synchronize()
    assert torch.all(dst == 7.0)
    assert rc.demote_batched(torch.zeros((0, 4, 3), dtype=torch.float64, device="cuda")).shape == (0, 4, 3)
