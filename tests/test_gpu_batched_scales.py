"""The one-workgroup batched IDs and SVDs on blocks far from unit scale (entries around 2^+-90 in f32 / c32, 2^+-900 in f64 / c64, and the
exponents where the squares of the entries start to overflow or go subnormal): LAPACK's ?nrm2 scales, and so must the column norms and
the ?larfg norm of these kernels (the domain paragraph at rc_column_id_rank_batched_* in include/rusty_compression_amd.h).

Per family and dtype one call on one stacked batch of every kind x every exponent of tests/scale_cases.py (21 matrices, one launch; the
neighbours of a matrix then differ from it by up to 2^180 / 2^1800, so an exponent leaking from one matrix to the next shows too).  Per
matrix: the family's checker of tests/scale_cases.py after exact descaling (test_scale_cases_cpu.py shows that LAPACK passes it at every
exponent and that a model with unscaled norms does not), then ranks, pivots and every factor against the e = 0 entry of the same batch,
bit for bit: a power of two commutes with every rounding while nothing leaves the normal range.  The health word stays 0.

Every cell of a batch is checked before the test fails, and the failure lists the (kind, e) cells.  On the kernels without the
normalisation every test of sections 1, 2, 4, 5 and 7 failed, in every family and dtype: always at the outer exponents and at the upper
edge, mostly at the lower edge, and the f64 / c64 SVD at all six non-zero exponents ("Input scales of the batched IDs and
SVDs").  Section 6's compositions failed there too and, with the IDs and the range step normalised, still failed through the
recompression they call (f64 from 2^+-300 on) until its factor loads were normalised as well."""
import ctypes

import numpy as np
import pytest
import torch

import rusty_compression_amd as rc
from rusty_compression_amd import _lib
from tests import range_step_ref as ref
from tests import range_step_ref_complex as refc
from tests import scale_cases as sc
from tests import test_gpu_batched_sketch_id as bsi
from tests import test_gpu_batched_sketch_id_complex as bsic
from tests.helpers import TOL, batched_launch, npy

pytestmark = pytest.mark.gpu

REAL = [np.float64, np.float32]
ALL = [np.float64, np.float32, np.complex128, np.complex64]


def tt(x):
    return torch.from_numpy(np.array(x, order="C")).cuda()  # a copy: the cached cases are read-only


def call(fn, *args, **kw):
    """fn on device tensors: numpy outputs, and the default context's health word is 0 afterwards."""
    out = fn(*args, **kw)
    torch.cuda.synchronize()
    assert _lib.default_context().get_health() == 0
    return tuple(npy(t) for t in out)


def tol_of(dtype):
    return sc.TOLS[sc.real_of(dtype)]


def for_every_cell(cells, check, kinds=sc.KINDS):
    """check(index, kind index, e) on every cell; one failure message that lists every failing (kind, e)."""
    failed = []
    for idx, (i, e) in enumerate(cells):
        try:
            check(idx, i, e)
        except AssertionError as err:
            failed.append((kinds[i], e, str(err).splitlines()[0][:160] if str(err) else "assert"))
    assert not failed, f"{len(failed)} of {len(cells)} cells failed: {failed}"


def expected_rank(shape, i, kk):
    return sc.exact_rank(shape) if sc.KINDS[i] == "exact" else kk


# ------------------------------------------------------------------------------------------------ 1. the IDs
@pytest.mark.parametrize("dtype", ALL)
@pytest.mark.parametrize("m,n,k", sc.ID_SHAPES)
def test_column_id_at_every_scale(m, n, k, dtype):
    units, cells, stacked = sc.batch((m, n), dtype)
    tol = tol_of(dtype)
    c, z, ind, ranks = call(rc.column_id_rank_batched, tt(stacked), k, tol)

    def check(idx, i, e):
        assert ranks[idx] == expected_rank((m, n), i, k)
        sc.check_column_id(units[i], e, c[idx], z[idx], ind[idx], ranks[idx], k, dtype, tol)
        u = sc.unit_cell(cells, i)
        sc.assert_same_as_unit(("c", "z", "ind", "ranks"), (c[u], z[u], ind[u], ranks[u]), (sc.descale(c[idx], e), z[idx], ind[idx], ranks[idx]),
                               sc.id_stable_prefix(units[i], ind[u], int(ranks[u]), dtype))

    for_every_cell(cells, check)


@pytest.mark.parametrize("dtype", ALL)
@pytest.mark.parametrize("m,n,k", sc.ID_SHAPES)
def test_two_sided_id_at_every_scale(m, n, k, dtype):
    units, cells, stacked = sc.batch((m, n), dtype)
    c, x, rr, row_ind, col_ind, ranks = call(rc.two_sided_id_rank_batched, tt(stacked), k, tol_of(dtype))

    def check(idx, i, e):
        assert ranks[idx] == expected_rank((m, n), i, k)
        sc.check_two_sided_id(units[i], e, c[idx], x[idx], rr[idx], row_ind[idx], col_ind[idx], ranks[idx], k, dtype)
        u = sc.unit_cell(cells, i)
        # the row pivots of an r x m factor are all decided once the column pivots are: compared over the rank
        sc.assert_same_as_unit(("c", "x", "r", "ranks"), (c[u], x[u], rr[u], ranks[u]), (c[idx], sc.descale(x[idx], e), rr[idx], ranks[idx]))
        ns = sc.id_stable_prefix(units[i], col_ind[u], int(ranks[u]), dtype)
        assert np.array_equal(col_ind[idx][:ns], col_ind[u][:ns]) and np.array_equal(row_ind[idx][:ns], row_ind[u][:ns])

    for_every_cell(cells, check)


# ------------------------------------------------------------------------------------------------ 2. the SVD
@pytest.mark.parametrize("dtype", ALL)
@pytest.mark.parametrize("m,n", sc.SVD_SHAPES)
def test_svd_at_every_scale(m, n, dtype):
    units, cells, stacked = sc.batch((m, n), dtype)
    k = min(m, n)
    fn = rc.svd_rank_batched_complex if sc.is_complex(dtype) else rc.svd_rank_batched
    u, s, vt, ranks = call(fn, tt(stacked), k, tol_of(dtype))

    def check(idx, i, e):
        assert ranks[idx] == expected_rank((m, n), i, k)
        sc.check_svd(units[i], e, u[idx], s[idx], vt[idx], ranks[idx], k, dtype)
        j = sc.unit_cell(cells, i)
        sc.assert_same_as_unit(("u", "s", "vt", "ranks"), (u[j], s[j], vt[j], ranks[j]), (u[idx], sc.descale(s[idx], e), vt[idx], ranks[idx]))

    for_every_cell(cells, check)


# ------------------------------------------------------------------------------------------------ 3. both plans of the working copy
@pytest.mark.parametrize("dtype", ALL)
@pytest.mark.parametrize("family", ["column_id", "two_sided_id", "svd"])
def test_the_shapes_reach_the_lds_and_the_workspace_plan(family, dtype):
    """The shapes above put the working copy W in LDS and in the workgroup's workspace slot in every family and dtype, so a change that
    normalises one variant only cannot pass."""
    seen = set()
    shapes = [(m, n, min(m, n)) for m, n in sc.SVD_SHAPES] if family == "svd" else sc.ID_SHAPES
    svd = rc.svd_rank_batched_complex if sc.is_complex(dtype) else rc.svd_rank_batched
    fn = {"column_id": rc.column_id_rank_batched, "two_sided_id": rc.two_sided_id_rank_batched, "svd": svd}[family]
    for m, n, k in shapes:
        a = tt(np.stack(sc.batch((m, n), dtype)[0]))
        _, lab = batched_launch(lambda: call(fn, a, k, tol_of(dtype)))
        print(f"{family} {np.dtype(dtype).name} {m}x{n}: {lab['op']} plan={lab['plan']}")
        seen.add(lab["plan"].split(",")[0])
    assert {"W:lds", "W:ws"} <= seen, seen


# ------------------------------------------------------------------------------------------------ 4. the sketched ID
@pytest.mark.parametrize("dtype", ALL)
@pytest.mark.parametrize("m,n,l", sc.SKETCH_SHAPES)
def test_sketched_id_at_every_scale(m, n, l, dtype):
    units, cells, stacked = sc.batch((m, n), dtype)
    om = sc.omega((m, n), l, dtype)
    tol = tol_of(dtype)
    fn = rc.sketch_column_id_rank_batched_complex if sc.is_complex(dtype) else rc.sketch_column_id_rank_batched
    (c, z, ind, ranks, y), lab = batched_launch(lambda: call(fn, tt(stacked), l, tol, omega=tt(om), return_sketch=True))
    assert lab["plan"].startswith("W:lds" if (m, n, l) == sc.SKETCH_SHAPES[0] else "W:ws"), lab["plan"]

    def check(idx, i, e):
        assert ranks[idx] == expected_rank((m, n), i, l)
        sc.check_sketch_id(units[i], om, e, c[idx], z[idx], ind[idx], ranks[idx], y[idx], l, dtype)
        u = sc.unit_cell(cells, i)
        sc.assert_same_as_unit(("c", "z", "ind", "ranks", "y"), (c[u], z[u], ind[u], ranks[u], y[u]),
                               (sc.descale(c[idx], e), z[idx], ind[idx], ranks[idx], sc.descale(y[idx], e)),
                               sc.id_stable_prefix(y[u], ind[u], int(ranks[u]), dtype))

    for_every_cell(cells, check)
    # the bit contract on the outermost blocks: Z, ind and ranks are the batched column ID's of the returned (scaled) sketch
    outer = [idx for idx, (_, e) in enumerate(cells) if e in (min(sc.exponents(dtype)), max(sc.exponents(dtype)))]
    got = (c[outer], z[outer], ind[outer], ranks[outer])
    if sc.is_complex(dtype):
        bsic.check_bit_contract(stacked[outer], y[outer], got, l, tol)
    else:
        bsi.check_bit_contract(stacked[outer], y[outer], got, l, tol, dtype)


# ------------------------------------------------------------------------------------------------ 5. the range step
@pytest.mark.parametrize("dtype", REAL)
@pytest.mark.parametrize("m,n,l", sc.STEP_SHAPES)
def test_range_step_at_every_scale(m, n, l, dtype):
    units, cells, stacked = sc.batch((m, n), dtype)
    om = sc.omega((m, n), l, dtype)
    q, p, ranks, y = call(rc.sketch_range_step_batched, tt(stacked), tt(om), return_sketch=True)

    def check(idx, i, e):
        sc.check_range_step(units[i], om, e, q[idx], p[idx], ranks[idx], y[idx], dtype)
        u = sc.unit_cell(cells, i)
        sc.assert_same_as_unit(("q", "p", "ranks", "y"), (q[u], p[u], ranks[u], y[u]),
                               (q[idx], sc.descale(p[idx], e), ranks[idx], sc.descale(y[idx], e)))

    for_every_cell(cells, check)


# ------------------------------------------------------------------------------------------------ 6. the power-iterated compositions
_HOST = {}


def host_model(which, shape, l, i, dtype):
    """(error, rank) of the f64 host model of tests/range_step_ref.py (complex data: the c128 one of tests/range_step_ref_complex.py) on unit
    matrix i with the same omega (made once)."""
    key = (which, shape, l, i, np.dtype(dtype))
    if key not in _HOST:
        a, om = sc.batch(shape, dtype)[0][i], sc.omega(shape, l, dtype)
        mod = refc if sc.is_complex(dtype) else ref
        fn = mod.column_id_power if which == "id" else mod.svd_power
        _HOST[key] = fn(a, om, l, tol_of(dtype), 1)[:2]
    return _HOST[key]


@pytest.mark.parametrize("dtype", ALL)
@pytest.mark.parametrize("m,n,l", sc.SKETCH_SHAPES)
def test_power_iterated_sketched_id_at_every_scale(m, n, l, dtype):
    """One round of power iteration, then the sketched ID.  The round orthonormalises P = a Q^T (complex: a Q^H), which carries the block's
    scale, by the tall recompression: that kernel loads its operands times exact powers of two (brc_exponent), the complex one as the real
    one, so the basis of the round, and with it every output, is the unit-scale one bit for bit."""
    units, cells, stacked = sc.batch((m, n), dtype)
    om = sc.omega((m, n), l, dtype)
    wide = np.complex128 if sc.is_complex(dtype) else np.float64
    fn = rc.sketch_column_id_rank_power_batched_complex if sc.is_complex(dtype) else rc.sketch_column_id_rank_power_batched
    c, z, ind, ranks = call(fn, tt(stacked), l, tol_of(dtype), power_iterations=1, omega=tt(om))

    def check(idx, i, e):
        r = int(ranks[idx])
        oerr, orank = host_model("id", (m, n), l, i, dtype)
        assert r == orank == expected_rank((m, n), i, l)
        assert sc.same_bits(c[idx][:, :r], stacked[idx][:, ind[idx][:r]]) and not np.any(c[idx][:, r:]) and not np.any(z[idx][r:])
        a64 = units[i].astype(wide)
        err = np.linalg.norm(a64 - sc.descale(c[idx], e)[:, :r].astype(wide) @ z[idx][:r].astype(wide)) / np.linalg.norm(a64)
        assert err <= 1.5 * oerr + 100 * np.finfo(sc.real_of(dtype)).eps, (err, oerr)
        u = sc.unit_cell(cells, i)
        sc.assert_same_as_unit(("c", "z", "ind", "ranks"), (c[u], z[u], ind[u], ranks[u]), (sc.descale(c[idx], e), z[idx], ind[idx], ranks[idx]), r)

    for_every_cell(cells, check)


@pytest.mark.parametrize("dtype", ALL)
@pytest.mark.parametrize("m,n,l", sc.SKETCH_SHAPES)
def test_power_iterated_sketched_svd_at_every_scale(m, n, l, dtype):
    """One range step, then the tall recompression of (P, Q): s carries the scale, U and Vt are the unit-scale ones bit for bit."""
    units, cells, stacked = sc.batch((m, n), dtype)
    om = sc.omega((m, n), l, dtype)
    wide = np.complex128 if sc.is_complex(dtype) else np.float64
    fn = rc.sketch_svd_rank_power_batched_complex if sc.is_complex(dtype) else rc.sketch_svd_rank_power_batched
    u, s, vt, ranks = call(fn, tt(stacked), l, tol_of(dtype), power_iterations=1, omega=tt(om))

    def check(idx, i, e):
        r = int(ranks[idx])
        oerr, orank = host_model("svd", (m, n), l, i, dtype)
        assert r == orank == expected_rank((m, n), i, l)
        u0, s0, vt0 = u[idx][:, :r].astype(wide), sc.descale(s[idx], e)[:r].astype(np.float64), vt[idx][:r].astype(wide)
        assert max(np.abs(u0.conj().T @ u0 - np.eye(r)).max(), np.abs(vt0 @ vt0.conj().T - np.eye(r)).max()) <= 4 * TOL[sc.real_of(dtype)]["orth"]
        assert np.all(np.diff(s0) <= 0) and s0[-1] > 0
        a64 = units[i].astype(wide)
        err = np.linalg.norm(a64 - (u0 * s0) @ vt0) / np.linalg.norm(a64)
        assert err <= 1.5 * oerr + 100 * np.finfo(sc.real_of(dtype)).eps, (err, oerr)
        j = sc.unit_cell(cells, i)
        sc.assert_same_as_unit(("u", "s", "vt", "ranks"), (u[j], s[j], vt[j], ranks[j]), (u[idx], sc.descale(s[idx], e), vt[idx], ranks[idx]))

    for_every_cell(cells, check)


# ------------------------------------------------------------------------------------------------ 7. graph capture at 2^-90
def test_graph_capture_replays_the_eager_bits_at_the_smallest_scale():
    m, n, k = sc.ID_SHAPES[0]
    units, cells, stacked = sc.batch((m, n), np.float32)
    sel = [idx for idx, (_, e) in enumerate(cells) if e == min(sc.E32)]
    cnt = len(sel)
    tol = tol_of(np.float32)
    lib = _lib.lib()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        a = tt(stacked[sel])
        eager = tuple(npy(t) for t in rc.column_id_rank_batched(a, k, tol))
        torch.cuda.synchronize()
        assert list(eager[3]) == [expected_rank((m, n), cells[idx][0], k) for idx in sel]
        ctx = _lib.Context(torch.cuda.current_device(), st.cuda_stream)
        c = torch.zeros((cnt, m, k), dtype=a.dtype, device=a.device)
        z = torch.zeros((cnt, k, n), dtype=a.dtype, device=a.device)
        ind = torch.zeros((cnt, n), dtype=torch.int64, device=a.device)
        ranks = torch.zeros(cnt, dtype=torch.int64, device=a.device)
        st.synchronize()
        args = (_lib.rc_matrix(a.data_ptr(), m, n, a.stride(1), a.stride(2)), ctypes.c_int64(a.stride(0)), ctypes.c_int32(cnt), ctypes.c_int64(k),
                ctypes.c_double(tol), _lib.mat(c[0]), ctypes.c_int64(m * k), _lib.mat(z[0]), ctypes.c_int64(k * n), _lib.i64p(ind), _lib.i64p(ranks))
        ctx.check(lib.rc_column_id_rank_batched_f32(ctx._h, *args))  # eager once: sizes the workspace
        ctx.synchronize()
        ctx.get_health()
        for t in (c, z, ind, ranks):
            t.zero_()
        st.synchronize()
        graph = ctypes.c_void_p(None)
        ctx.check(lib.rc_graph_begin_capture(ctx._h))
        ctx.check(lib.rc_column_id_rank_batched_f32(ctx._h, *args))
        ctx.check(lib.rc_graph_end_capture(ctx._h, ctypes.byref(graph)))
        try:
            ctx.check(lib.rc_graph_launch(ctx._h, graph))
            ctx.synchronize()
            for p, q in zip(eager, (c, z, ind, ranks)):
                assert sc.same_bits(p, npy(q))
            assert ctx.get_health() == 0
        finally:
            ctx.check(lib.rc_graph_destroy(ctx._h, graph))
            ctx.close()
