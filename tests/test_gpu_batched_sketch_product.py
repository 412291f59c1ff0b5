"""Batched sketch product (rc_sketch_product_batched_*, batch.sketch_product_batched): per block Y = omega a and nothing else, for blocks
of up to 65536 columns, one (block, 64-column panel) per work unit of the persistent grid.

Checked: the bit contract (y equals the sketched ID's y for n <= 512 on all four staging instances of both precisions; through transposed
views the call gives the range step's p from the step's own q; for n > 512 every 512-column slice of y equals the existing call's y on
that slice of a); the accuracy of an element against the f64 host product under the project's sketch bound
|y - omega a| <= c (m + 4) u (|omega| |a|), c = 1 (f32) or 2 (f64); the persistent loop (more units than workgroups); 64-bit offsets (a
view that spans more than 2^31 elements); and the contract of the batch (count = 0, shared operands, strided output, position and
neighbours, graph replay, non-finite input, argument checks).

Measured on an MI355X, worst |y - omega a| / bound over the seven shapes below: 0.027 in f64 (40 x 64, l = 1; the 513- and 1100-column
f64 products agree with the host product exactly) and 0.064 in f32 (70 x 1100, l = 128); 0.114 over the 64 blocks of 40 x 4096 in f32.
The chain is the sketched ID's, so are the figures (tests/test_gpu_batched_sketch_id.py)."""
import ctypes
import re

import numpy as np
import pytest
import torch

import rusty_compression_amd as rc
from rusty_compression_amd import _lib
from tests.helpers import npy

pytestmark = pytest.mark.gpu

DTYPES = [np.float64, np.float32]
# (m, n, l) with n <= 512: nothing a multiple of 16 / 32 / 64; the sketch tests' tall shape; l = 128; l = 1 with one full panel
SMALL = [(70, 33, 17), (1030, 300, 40), (520, 130, 128), (40, 64, 1)]
# n > 512: the last panel holds one column; two 512-column slices with a ragged end; three slices at l = 128
WIDE = [(130, 513, 24), (600, 700, 40), (70, 1100, 128)]
INVALID = 5


def tt(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def same_bits(x, y):
    x, y = np.asarray(x), np.asarray(y)
    return x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes()  # bytes: a NaN equals itself, -0.0 is not 0.0


def colmajor(t):
    """A copy of a [.., r, c] tensor whose last two strides are (1, r) whatever its shape (contiguous() keeps the strides of an r = 1 or
    c = 1 matrix)."""
    r, c = t.shape[-2:]
    out = torch.empty_strided(tuple(t.shape), ((r * c,) if t.dim() == 3 else ()) + (1, r), dtype=t.dtype, device=t.device)
    out.copy_(t)
    return out


def product(a, omega, out=None):
    y = rc.sketch_product_batched(a, omega, out=out)
    torch.cuda.synchronize()
    return npy(y.contiguous())


def sketch_of_the_id(a, omega):
    """The y that rc_sketch_column_id_rank_batched_* writes (n <= 512)."""
    y = rc.sketch_column_id_rank_batched(a, min(omega.shape[-2], 128), 0.0, omega=omega, return_sketch=True)[4]
    torch.cuda.synchronize()
    return npy(y)


def launch_label(fn):
    """fn() under the default context's event profile: (fn's result, the fields of the one op:batched_sketch_product label it recorded)."""
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
    mt = re.fullmatch(r"op:batched_sketch_product (\d+)x(\d+) l=(\d+) count=(\d+) grid=(\d+) slots=(\d+) plan=units=(\d+),rows=32,cols=64,scratch=(\d+)",
                      labels[0][0])
    assert mt, labels[0][0]
    return out, dict(zip(("m", "n", "l", "count", "grid", "slots", "units", "scratch"), map(int, mt.groups())))


def raw(fn_dtype, a, omega, y, ctx=None, count=None):
    """One raw call on 3-D device views (omega 2-D: shared, batch stride 0); returns the status."""
    ctx = ctx or _lib.default_context()
    fn = getattr(_lib.lib(), f"rc_sketch_product_batched_{_lib.suffix(fn_dtype)}")

    def view(t):
        if t.dim() == 2:
            return _lib.rc_matrix(t.data_ptr(), t.shape[0], t.shape[1], t.stride(0), t.stride(1)), ctypes.c_int64(0)
        return _lib.rc_matrix(t.data_ptr(), t.shape[1], t.shape[2], t.stride(1), t.stride(2)), ctypes.c_int64(t.stride(0))

    return fn(ctx._h, *view(a), *view(omega), ctypes.c_int32(a.shape[0] if count is None else count), *view(y))


_DATA = {}


def data(m, n, l, dtype):
    """Two Gaussian blocks and a shared Gaussian omega per shape and precision, on the host and the device, and the contiguous call's y
    (all made once and left unchanged)."""
    key = (m, n, l, np.dtype(dtype))
    if key not in _DATA:
        rng = np.random.default_rng(1000 * m + 10 * n + l)
        a, om = rng.standard_normal((2, m, n)).astype(dtype), rng.standard_normal((l, m)).astype(dtype)
        ad, omd = tt(a), tt(om)
        _DATA[key] = (a, om, ad, omd, product(ad, omd))
    return _DATA[key]


def bound_ratio(y, a, om, dtype):
    """max over the elements of |y - omega a| / (c (m + 4) u (|omega| |a|)) for one block, in f64."""
    m = a.shape[0]
    u = np.finfo(dtype).eps / 2
    cst = 1.0 if dtype == np.float32 else 2.0
    a64, o64 = a.astype(np.float64), om.astype(np.float64)
    bound = cst * (m + 4) * u * (np.abs(o64) @ np.abs(a64))
    return float(np.max(np.abs(y.astype(np.float64) - o64 @ a64) / np.maximum(bound, np.finfo(np.float64).tiny)))


# ---------------------------------------------------------------- 1. bits against the existing sketch, on all four instances
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m,n,l", SMALL)
def test_bits_of_the_sketched_ids_sketch_on_every_instance(m, n, l, dtype):
    a, om, ad, omd, y0 = data(m, n, l, dtype)
    want = sketch_of_the_id(ad, omd)
    a_cm, om_cm = colmajor(ad), colmajor(omd)
    for av in (ad, a_cm):
        for ov in (omd, om_cm):
            y, lab = launch_label(lambda: product(av, ov))
            assert (lab["m"], lab["n"], lab["l"], lab["count"]) == (m, n, l, 2)
            assert lab["units"] == 2 * -(-n // 64) and lab["grid"] == min(lab["slots"], lab["units"])
            assert lab["scratch"] == 0  # accumulators and the staging registers alone: no instance spills
            assert y.shape == (2, l, n) and y.dtype == np.dtype(dtype)
            assert same_bits(y, want)
    assert same_bits(y0, want)


# ---------------------------------------------------------------- 2. bits against the range step's projection
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m,n,l", SMALL)
def test_transposed_views_give_the_range_steps_projection(m, n, l, dtype):
    assert l <= min(m, n)
    a, om, ad, omd, _ = data(m, n, l, dtype)
    q, p, ranks = rc.sketch_range_step_batched(ad, omd)
    for qv in (q, colmajor(q)):  # the step's own q, row-major and column-major
        got = torch.full((2, m, l), 7.0, dtype=ad.dtype, device="cuda")
        rc.sketch_product_batched(ad.mT, qv, out=got.mT)
        torch.cuda.synchronize()
        assert same_bits(npy(got), npy(p))


# ---------------------------------------------------------------- 3. panels: every 512-column slice is the existing call on that slice
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m,n,l", WIDE)
def test_every_512_column_slice_is_the_existing_sketch_of_that_slice(m, n, l, dtype):
    a, om, ad, omd, y = data(m, n, l, dtype)
    assert y.shape == (2, l, n)
    for lo in range(0, n, 512):
        hi = min(lo + 512, n)
        want = sketch_of_the_id(ad[:, :, lo:hi], omd)  # a view: the slice's own row stride n
        assert want.shape == (2, l, hi - lo)
        assert same_bits(np.ascontiguousarray(y[:, :, lo:hi]), want), (lo, hi)
    # the column-major block gives the same bits (the other staging instance, panels a column stride apart)
    assert same_bits(product(colmajor(ad), omd), y)


# ---------------------------------------------------------------- 4. accuracy against the f64 host product
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m,n,l", SMALL + WIDE)
def test_elements_are_inside_the_sketch_bound(m, n, l, dtype):
    a, om, _, _, y = data(m, n, l, dtype)
    worst = max(bound_ratio(y[i], a[i], om, dtype) for i in range(2))
    print(f"sketch product {m}x{n} l={l} {np.dtype(dtype).name}: max |y - omega a| / bound = {worst:.3e}")
    assert worst <= 1.0


# ---------------------------------------------------------------- 5. the persistent loop: more units than workgroups
def test_more_units_than_workgroups():
    cnt, m, n, l = 64, 40, 4096, 17
    rng = np.random.default_rng(50)
    a = rng.standard_normal((cnt, m, n)).astype(np.float32)
    om = rng.standard_normal((l, m)).astype(np.float32)
    ad, omd = tt(a), tt(om)
    y, lab = launch_label(lambda: product(ad, omd))
    assert lab["units"] == cnt * (n // 64) == 4096 and lab["count"] == cnt
    assert lab["grid"] < lab["units"] and lab["grid"] == lab["slots"]
    worst = max(bound_ratio(y[i], a[i], om, np.float32) for i in range(cnt))
    print(f"persistent loop: grid {lab['grid']} for {lab['units']} units; max |y - omega a| / bound = {worst:.3e}")
    assert worst <= 1.0
    for i in (0, 31, 63):
        alone, lab1 = launch_label(lambda: product(ad[i:i + 1], omd))
        assert lab1["count"] == 1 and lab1["grid"] == lab1["units"] == 64
        assert same_bits(alone[0], y[i])


# ---------------------------------------------------------------- 6. 64-bit offsets
def test_a_view_spanning_more_than_2_to_31_elements():
    m, n, l = 40, 520, 8
    cs = (1 << 22) + 3
    rng = np.random.default_rng(60)
    block = tt(rng.standard_normal((1, m, n)).astype(np.float32))
    om = tt(rng.standard_normal((l, m)).astype(np.float32))
    span = (n - 1) * cs + (m - 1) + 1
    assert span > 1 << 31
    store = torch.empty(span, dtype=torch.float32, device="cuda")  # only the viewed elements are written
    wide = store.as_strided((1, m, n), (0, 1, cs))
    wide.copy_(block)
    want = product(block, om)
    assert same_bits(product(wide, om), want)
    # the same span along the rows of a: the transposed block through a row stride of cs
    tall = store.as_strided((1, n, m), (0, cs, 1))
    om2 = tt(rng.standard_normal((l, n)).astype(np.float32))
    assert same_bits(product(tall, om2), product(block.mT.contiguous(), om2))
    del store, wide, tall
    torch.cuda.empty_cache()


# ---------------------------------------------------------------- 7. the contract of the batch
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_shared_operands_strided_output_position_and_neighbours(dtype):
    rng = np.random.default_rng(70)
    m, n, l = 90, 200, 20
    om = tt(rng.standard_normal((l, m))).to(dtype)
    protos = [rng.standard_normal((m, n)), 1e-3 * rng.standard_normal((m, n)), np.full((m, n), np.nan), np.zeros((m, n)),
              rng.standard_normal((m, 1)) @ rng.standard_normal((1, n))]
    alone = [product(tt(x[None]).to(dtype), om) for x in protos]
    assert not np.any(alone[3]) and np.all(np.isnan(alone[2]))
    count = 23
    big = torch.zeros((count, m + 1, n + 2), dtype=dtype, device="cuda")  # a batch stride and a row stride of its own
    big[:, :m, :n] = tt(np.stack(protos)).to(dtype)[torch.arange(count, device="cuda") % len(protos)]
    got = product(big[:, :m, :n], om)
    for i in range(count):  # every block next to a block full of NaN, at every position
        assert same_bits(alone[i % len(protos)][0], got[i])
    # batch stride 0 for a: every block of the output is the one block's sketch; a per-block omega = count calls with count = 1
    one = tt(protos[0][None]).to(dtype)
    shared = product(one.expand(5, m, n), om)
    for i in range(5):
        assert same_bits(shared[i], alone[0][0])
    oms = tt(rng.standard_normal((5, l, m))).to(dtype)
    per = product(one.expand(5, m, n), oms)
    for i in range(5):
        assert same_bits(per[i], product(one, oms[i])[0])
    # y into a strided view: the padding keeps its canary; column-major inside its block
    for buf, view in ((torch.full((5, l + 2, n + 3), 7.0, dtype=dtype, device="cuda"), lambda b: b[:, :l, :n]),
                      (torch.full((5, n + 1, l + 4), 7.0, dtype=dtype, device="cuda"), lambda b: b[:, :n, :l].transpose(1, 2))):
        yv = view(buf)
        assert raw(dtype, one.expand(5, m, n), oms, yv) == 0
        torch.cuda.synchronize()
        assert same_bits(npy(yv.contiguous()), per)
        gaps = torch.ones_like(buf, dtype=torch.bool)
        view(gaps)[:] = False
        assert bool((buf[gaps] == 7.0).all())
    # a NaN or Inf element stays in its block
    clean = tt(rng.standard_normal((6, m, n))).to(dtype)
    want = product(clean, om)
    bad = clean.clone()
    bad[2, 17, 23] = float("nan")
    bad[4, 80, 199] = float("inf")
    got = product(bad, om)
    for i in (0, 1, 3, 5):
        assert same_bits(want[i], got[i])
    assert np.all(np.isnan(got[2][:, 23])) and same_bits(np.delete(got[2], 23, axis=1), np.delete(want[2], 23, axis=1))  # its column alone


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_graph_replay_gives_the_eager_bits(dtype):
    rng = np.random.default_rng(71)
    cnt, m, n, l = 5, 300, 700, 20
    lib = _lib.lib()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        a = tt(rng.standard_normal((cnt, m, n))).to(dtype)
        om = tt(rng.standard_normal((l, m))).to(dtype)
        eager = product(a, om)
        ctx = _lib.Context(torch.cuda.current_device(), st.cuda_stream)
        y = torch.zeros((cnt, l, n), dtype=a.dtype, device="cuda")
        st.synchronize()
        assert raw(dtype, a, om, y, ctx=ctx) == 0  # eager once on this context
        ctx.synchronize()
        ctx.get_health()
        y.zero_()
        st.synchronize()
        graph = ctypes.c_void_p(None)
        ctx.check(lib.rc_graph_begin_capture(ctx._h))
        ctx.check(raw(dtype, a, om, y, ctx=ctx))  # one launch: the capture has no parallel branches
        ctx.check(lib.rc_graph_end_capture(ctx._h, ctypes.byref(graph)))
        try:
            ctx.check(lib.rc_graph_launch(ctx._h, graph))
            ctx.synchronize()
            assert same_bits(eager, npy(y))
            assert ctx.get_health() == 0
        finally:
            ctx.check(lib.rc_graph_destroy(ctx._h, graph))
            ctx.close()


def test_argument_checks_count_zero_and_dtype_errors():
    ctx = _lib.default_context()
    ctx.get_health()
    e = lambda r, c: torch.zeros((2, r, c), dtype=torch.float64, device="cuda")  # noqa: E731
    m, n, l = 60, 700, 12

    def call(a=None, om=None, y=None, count=2):
        a = e(m, n) if a is None else a
        om = e(l, m)[0] if om is None else om
        y = e(l, n) if y is None else y
        return raw(torch.float64, a, om, y, count=count)

    def shaped(t, rows, cols):  # a small allocation whose shape fields alone say rows x cols
        return t.as_strided((2, rows, cols), (1, 0, 0))

    assert call() == 0
    small = e(4, 4)
    assert call(a=shaped(small, 200, 200), om=shaped(small, 129, 200)[0], y=shaped(small, 129, 200)) == INVALID      # l = 129
    assert call(a=shaped(small, m, 65537), y=shaped(small, l, 65537)) == INVALID                                      # n = 65537
    assert call(a=shaped(small, 65537, n), om=shaped(small, l, 65537)[0]) == INVALID                                  # m = 65537
    assert call(a=shaped(small, 0, n), om=shaped(small, l, 0)[0]) == INVALID                                          # m = 0
    assert call(a=shaped(small, m, 0), y=shaped(small, l, 0)) == INVALID                                              # n = 0
    assert call(om=shaped(small, 0, m)[0], y=shaped(small, 0, n)) == INVALID                                          # l = 0
    assert call(count=-1) == INVALID
    assert call(om=e(l, m + 1)[0]) == INVALID                                                                         # omega.cols != a.rows
    assert call(y=e(l + 1, n)) == INVALID and call(y=e(l, n - 1)) == INVALID                                          # wrong y shape
    overl = torch.zeros((2, l, n), dtype=torch.float64, device="cuda").as_strided((2, l, n), (l * n - 1, n, 1))
    assert call(y=overl) == INVALID                                                                                   # overlapping / short y stride
    assert call(y=overl, count=1) == 0                                                                                # one block: no stride to check
    # a null required pointer (the shape fields are right)
    fn = _lib.lib().rc_sketch_product_batched_f64
    v = lambda t: (_lib.mat(t[0]), ctypes.c_int64(t.stride(0)))  # noqa: E731
    nullmat = lambda r, c: (_lib.rc_matrix(None, r, c, c, 1), ctypes.c_int64(r * c))  # noqa: E731
    a0, om0, y0 = e(m, n), e(l, m), e(l, n)
    good = dict(a=v(a0), om=v(om0), y=v(y0))
    for name, null in (("a", nullmat(m, n)), ("om", nullmat(l, m)), ("y", nullmat(l, n))):
        g = dict(good, **{name: null})
        assert fn(ctx._h, *g["a"], *g["om"], ctypes.c_int32(2), *g["y"]) == INVALID, name
    assert fn(ctx._h, *v(a0), *v(om0), ctypes.c_int32(2), *v(y0)) == 0
    assert fn(None, *v(a0), *v(om0), ctypes.c_int32(2), *v(y0)) == INVALID  # null context
    # count = 0: nothing to do (null pointers are then legal), the output untouched, a correctly shaped empty result
    canary = torch.full((2, l, n), 7.0, dtype=torch.float64, device="cuda")
    assert call(y=canary, count=0) == 0
    assert fn(ctx._h, *nullmat(m, n), *nullmat(l, m), ctypes.c_int32(0), *nullmat(l, n)) == 0
    torch.cuda.synchronize()
    assert bool((canary == 7.0).all())
    out = rc.sketch_product_batched(torch.zeros((0, 30, 600), dtype=torch.float32, device="cuda"), torch.zeros((9, 30), dtype=torch.float32, device="cuda"))
    assert tuple(out.shape) == (0, 9, 600)
    # dtype and shape errors of the wrapper
    with pytest.raises(TypeError):
        rc.sketch_product_batched(torch.zeros((2, 30, 20), dtype=torch.complex128, device="cuda"), torch.zeros((4, 30), dtype=torch.complex128, device="cuda"))
    with pytest.raises(TypeError):
        rc.sketch_product_batched(e(30, 20), torch.zeros((6, 30), dtype=torch.float32, device="cuda"))
    with pytest.raises(TypeError):
        rc.sketch_product_batched(e(30, 20), e(6, 30)[0], out=torch.zeros((2, 6, 20), dtype=torch.float32, device="cuda"))
    with pytest.raises(AssertionError):
        rc.sketch_product_batched(e(30, 20)[0], e(6, 30)[0])
    with pytest.raises(AssertionError):
        rc.sketch_product_batched(e(30, 20), e(6, 30)[0], out=e(6, 21))
    with pytest.raises(AssertionError, match="sketch_product_batched"):  # RC_INVALID_ARGUMENT: omega.cols != a.rows
        rc.sketch_product_batched(e(30, 20), e(6, 31)[0])
    torch.cuda.synchronize()
    assert ctx.get_health() == 0
