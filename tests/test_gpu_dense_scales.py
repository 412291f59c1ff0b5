"""The dense single-factorization calls on matrices far from unit scale (entries around 2^+-90 in f32 / c32, 2^+-900 in f64 / c64, and
the exponents where the squares of the entries start to overflow or go subnormal): rc_pivoted_qr_*, rc_pivoted_lq_*, rc_geqp3_* with
rc_orgqr_*, rc_compute_svd_*, rc_max_col_norm_*, rc_rel_diff_fro_* and the composition QR -> column ID -> two-sided ID (the "Input scale"
paragraph at rc_pivoted_qr_* in include/rusty_compression_amd.h).

One test per (entry point, route, dtype) with 21 small calls on the default context: every kind x every exponent of
tests/dense_scale_cases.py, on the smallest shape that reaches the route.  Per cell: the entry point's unit-scale checker after exact
descaling (tests/test_dense_scale_cases_cpu.py shows that LAPACK passes it at every exponent and that a QR with unscaled norms does
not); the health word, read and cleared before the call, 0 after it; the set of op: / info: profile labels equal to the unit cell's,
whose set holds the route the test names (a route that falls back at 2^510 fails here even with the right numbers); and, for the
Gaussian and the 1e-3 kind, pivots and every scale-free factor (Q, U, Vt, tau, reflectors, Z) equal to the unit cell's bytes, every
scaled factor (R, L, s, C) equal to them after descale: the entry points normalise by an exact power of two, so the kernels see the same
bits at every scale.  Every cell is checked before a test fails, and the failure lists the (kind, e) cells."""
import ctypes

import numpy as np
import pytest
import torch

import rusty_compression_amd as rc
from oracle import ref_lapack as o
from rusty_compression_amd import _lib
from tests import dense_scale_cases as dc
from tests import scale_cases as sc
from tests.helpers import npy
from tests.test_gpu_svd_routes import profiled

pytestmark = pytest.mark.gpu

ALL = dc.REAL + dc.COMPLEX
CT = rc.CompressionType


def tt(x):
    return torch.from_numpy(np.array(x, order="C")).cuda()  # a copy: the cached cases are read-only


def with_options(options, fn):
    """fn() with the context options of a route (names of rusty_compression_amd._lib) set, and put back to 1."""
    ctx = _lib.default_context()
    for name, value in options.items():
        ctx.set_option(getattr(_lib, name), value)
    try:
        return fn()
    finally:
        for name in options:
            ctx.set_option(getattr(_lib, name), 1)


def observed(fn, options=None):
    """(numpy outputs of fn, the op: and info: labels it recorded); the health word, cleared before, is asserted 0 after."""
    ctx = _lib.default_context()
    ctx.get_health()

    def run():
        out = fn()
        out = out if isinstance(out, (tuple, list)) else (out,)
        return tuple(npy(t) if hasattr(t, "detach") else t for t in out)

    out, labels = with_options(options or {}, lambda: profiled(run))
    torch.cuda.synchronize()
    health = ctx.get_health()
    assert health == 0, "health %d" % health
    return out, frozenset(k for k in labels if k.startswith(("op:", "info:")))


def every_cell(shape, dtype, run, check, names, descaled, route_labels, options=None):
    """run(scaled input) -> outputs (numpy); check(a, e, *outputs) is the tolerance checker; names: the outputs by name; descaled(outs, e)
    -> the outputs with the scale removed from those that carry it.  The unit cell of a kind runs first."""
    units, cells = dc.cases(shape, dtype)
    unit = {}
    failed = []
    for i, e in cells:
        try:
            outs, labels = observed(lambda: run(tt(sc.scale(units[i], e))), options)
            if e == 0:
                unit[i] = (descaled(outs, 0), labels)
                for prefix in route_labels:
                    assert any(k.startswith(prefix) for k in labels), ("route", prefix, sorted(labels))
            check(units[i], e, *outs)
            assert labels == unit[i][1], ("labels", sorted(labels ^ unit[i][1]))
            if dc.KINDS[i] in dc.BITWISE_KINDS:
                dc.assert_same_as_unit(names, unit[i][0], descaled(outs, e))
        except AssertionError as err:
            failed.append((dc.KINDS[i], e, dc.where(err)))
    assert not failed, f"{len(failed)} of {len(cells)} cells failed: {failed}"


# ------------------------------------------------------------------------------------------------ 1. pivoted QR and LQ
@pytest.mark.parametrize("dtype", dc.REAL)
@pytest.mark.parametrize("route", list(dc.QR_ROUTES))
def test_pivoted_qr_at_every_scale(route, dtype):
    shape, k, options, label = dc.QR_ROUTES[route]
    every_cell(shape, dtype, lambda x: rc.pivoted_qr(x, rank=k), lambda a, e, q, r, ind: dc.check_qr(a, e, q, r, ind, k), ("q", "r", "ind"),
               lambda outs, e: (outs[0], sc.descale(outs[1], e), outs[2]), (label,), options)


@pytest.mark.parametrize("dtype", dc.COMPLEX)
@pytest.mark.parametrize("shape", dc.COMPLEX_QR_SHAPES)
def test_complex_pivoted_qr_at_every_scale(shape, dtype):
    k = min(shape)
    every_cell(shape, dtype, rc.pivoted_qr, lambda a, e, q, r, ind: dc.check_qr(a, e, q, r, ind, k), ("q", "r", "ind"),
               lambda outs, e: (outs[0], sc.descale(outs[1], e), outs[2]), (dc.COMPLEX_LABEL,))


@pytest.mark.parametrize("dtype", dc.REAL)
@pytest.mark.parametrize("route", list(dc.LQ_ROUTES))
def test_pivoted_lq_at_every_scale(route, dtype):
    shape, k, options, label = dc.LQ_ROUTES[route]
    every_cell(shape, dtype, rc.pivoted_lq, dc.check_lq, ("l", "q", "ind"), lambda outs, e: (sc.descale(outs[0], e), outs[1], outs[2]), (label,), options)


@pytest.mark.parametrize("dtype", dc.COMPLEX)
@pytest.mark.parametrize("shape", dc.COMPLEX_QR_SHAPES)
def test_complex_pivoted_lq_at_every_scale(shape, dtype):
    every_cell(shape, dtype, rc.pivoted_lq, dc.check_lq, ("l", "q", "ind"), lambda outs, e: (sc.descale(outs[0], e), outs[1], outs[2]), (dc.COMPLEX_LABEL,))


# ------------------------------------------------------------------------------------------------ 2. ?geqp3 and ?orgqr
def geqp3_orgqr(x):
    f, jp, tau = rc.geqp3(x)
    return f, jp, tau, rc.orgqr(f, tau)


def geqp3_shapes():
    real = [pytest.param(v[0], v[3], dt, id="%s-%s" % (name, np.dtype(dt).name)) for name, v in dc.GEQP3_ROUTES.items() for dt in dc.REAL]
    return real + [pytest.param(s, dc.COMPLEX_LABEL, dt, id="%dx%d-%s" % (s + (np.dtype(dt).name,))) for s in dc.COMPLEX_QR_SHAPES for dt in dc.COMPLEX]


@pytest.mark.parametrize("shape,label,dtype", geqp3_shapes())
def test_geqp3_and_orgqr_at_every_scale(shape, label, dtype):
    """tau and the reflectors below the diagonal are the unit cell's, R carries 2^e, and ?orgqr of the result is the unit cell's Q."""
    k = min(shape)
    every_cell(shape, dtype, geqp3_orgqr, dc.check_geqp3_at, ("f", "jpvt", "tau", "q"),
               lambda outs, e: (dc.descale_geqp3(outs[0], e, k), outs[1], outs[2], outs[3]), (label,))


# ------------------------------------------------------------------------------------------------ 3. the SVD
def svd_params():
    return [pytest.param(dt, name, id="%s-%s" % (np.dtype(dt).name, name)) for dt in ALL for name in dc.svd_routes(dt)]


@pytest.mark.parametrize("dtype,route", svd_params())
def test_compute_svd_at_every_scale(dtype, route):
    shape, labels = dc.svd_routes(dtype)[route]
    every_cell(shape, dtype, rc.compute_svd, dc.check_svd, ("u", "s", "vt"), lambda outs, e: (outs[0], sc.descale(outs[1], e), outs[2]), labels)


# ------------------------------------------------------------------------------------------------ 4. the host scalars
@pytest.mark.parametrize("dtype", ALL)
@pytest.mark.parametrize("shape", [(60, 40), (1024, 33)])
def test_max_col_norm_and_rel_diff_fro_at_every_scale(shape, dtype):
    """max_col_norm(2^e a) is ldexp(max_col_norm(a), e) and rel_diff_fro(2^e b, 2^e a) is rel_diff_fro(b, a), both bit for bit and in
    every kind (they are no noise-level outputs); the unit values against the oracle's to test_max_col_norm_and_rel_diff's bounds."""
    rd = sc.real_of(dtype)
    f64 = rd == np.dtype(np.float64)
    units, cells = dc.cases(shape, dtype)
    unit = {}
    failed = []
    for i, e in cells:
        a, b = units[i], dc.perturbed(units[i])
        try:
            (nrm, diff), _ = observed(lambda: (rd.type(rc.max_col_norm(tt(sc.scale(a, e)))), rd.type(rc.rel_diff_fro(tt(sc.scale(b, e)), tt(sc.scale(a, e))))))
            if e == 0:
                unit[i] = (nrm, diff)
                assert abs(float(nrm) - float(o.max_col_norm(a))) <= (1e-12 if f64 else 1e-4)
                assert abs(float(diff) - o.rel_diff_fro(b, a)) <= (1e-12 if f64 else 1e-6)
            assert sc.same_bits(nrm, np.ldexp(unit[i][0], e)), ("max_col_norm", float(nrm), float(np.ldexp(unit[i][0], e)))
            assert sc.same_bits(diff, unit[i][1]), ("rel_diff_fro", float(diff), float(unit[i][1]))
        except AssertionError as err:
            failed.append((dc.KINDS[i], e, dc.where(err)))
    assert not failed, f"{len(failed)} of {len(cells)} cells failed: {failed}"


# ------------------------------------------------------------------------------------------------ 5. one composition per dtype
@pytest.mark.parametrize("dtype", ALL)
def test_qr_to_two_sided_id_at_every_scale(dtype):
    """QR.compute_from -> column_id -> two_sided_id on 60 x 40: Z and the two-sided ID's C and R (free of X) equal the unit cell's bytes,
    the column ID's C and the skeleton X descale to them; QR.compress by tolerance cuts the `exact` kind at rank 5 at every exponent."""
    shape = (60, 40)
    tol = sc.TOLS[sc.real_of(dtype)]
    units, cells = dc.cases(shape, dtype)
    unit = {}
    failed = []

    def run(x, compress):
        qr = rc.QR.compute_from(x)
        cid = qr.column_id()
        ts = cid.two_sided_id()
        # (the other two kinds never fall below the tolerance, which the reference answers with a CompressionError)
        return cid.c, cid.z, cid.col_ind, ts.c, ts.x, ts.r, ts.row_ind, qr.compress(CT.ADAPTIVE(tol)).rank() if compress else None

    for i, e in cells:
        a = units[i]
        try:
            (c, z, col_ind, tc, tx, tr, row_ind, rank), _ = observed(lambda: run(tt(sc.scale(a, e)), dc.KINDS[i] == "exact"))
            got = (sc.descale(c, e), z, col_ind, tc, sc.descale(tx, e), tr, row_ind)
            if e == 0:
                unit[i] = got
            assert np.all(np.isfinite(c)) and np.all(np.isfinite(z))
            if dc.KINDS[i] == "exact":
                assert rank == sc.exact_rank(shape), ("rank", rank)
            else:
                dc.assert_same_as_unit(("c", "z", "col_ind", "ts.c", "ts.x", "ts.r", "row_ind"), unit[i], got)
        except AssertionError as err:
            failed.append((dc.KINDS[i], e, dc.where(err)))
    assert not failed, f"{len(failed)} of {len(cells)} cells failed: {failed}"


# ------------------------------------------------------------------------------------------------ 6. under capture
@pytest.mark.parametrize("e", [-900, 900])
@pytest.mark.parametrize("call", ["rc_pivoted_qr_f64", "rc_compute_svd_f64"])
def test_captured_calls_at_the_outer_scales_replay_the_eager_bits(call, e):
    """1024 x 33 (CholeskyQR2) at 2^+-900, eagerly and then recorded into a hipGraph and replayed twice into zeroed outputs: the replays
    equal the eager result's bytes and the health word stays 0.  Under capture no fallback and no host read is possible, so the exponent
    is computed and applied on the device."""
    lib = _lib.lib()
    m, n = 1024, 33
    an = sc.scale(dc.cases((m, n), np.float64)[0][0], e)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        ctx = _lib.Context(torch.cuda.current_device(), st.cuda_stream)
        a = tt(an)
        if call == "rc_pivoted_qr_f64":
            outs = [torch.empty((m, n), dtype=torch.float64, device="cuda"), torch.empty((n, n), dtype=torch.float64, device="cuda"),
                    torch.empty(n, dtype=torch.int64, device="cuda")]
            args = (_lib.mat(a), _lib.mat(outs[0]), _lib.mat(outs[1]), _lib.i64p(outs[2]))
        else:
            outs = [torch.empty((m, n), dtype=torch.float64, device="cuda"), torch.empty(n, dtype=torch.float64, device="cuda"),
                    torch.empty((n, n), dtype=torch.float64, device="cuda")]
            args = (_lib.mat(a), _lib.mat(outs[0]), ctypes.c_void_p(outs[1].data_ptr()), _lib.mat(outs[2]))
        ctx.get_health()
        ctx.call(call, *args)
        ctx.synchronize()
        eager = [t.clone() for t in outs]
        graph = ctypes.c_void_p(None)
        ctx.check(lib.rc_graph_begin_capture(ctx._h))
        ctx.call(call, *args)
        ctx.check(lib.rc_graph_end_capture(ctx._h, ctypes.byref(graph)))
        replays = []
        for _ in range(2):
            for t in outs:
                t.zero_()
            ctx.check(lib.rc_graph_launch(ctx._h, graph))
            ctx.synchronize()
            replays.append([t.clone() for t in outs])
        health = ctx.get_health()
        ctx.check(lib.rc_graph_destroy(ctx._h, graph))
        ctx.close()
    a0 = dc.cases((m, n), np.float64)[0][0]
    if call == "rc_pivoted_qr_f64":
        dc.check_qr(a0, e, npy(eager[0]), npy(eager[1]), npy(eager[2]), n)
    else:
        dc.check_svd(a0, e, npy(eager[0]), npy(eager[1]), npy(eager[2]))
    for i, rep in enumerate(replays):
        assert all(sc.same_bits(npy(g), npy(w)) for g, w in zip(rep, eager)), "replay %d differs from the eager call" % i
    assert health == 0, health
