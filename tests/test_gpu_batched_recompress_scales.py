"""The batched recompressions and residual norms on operands far from unit scale: the calls that consume what the batched IDs and SVDs
return for a block at 2^+-90 (f32 / c32) or 2^+-900 (f64 / c64), held to the same domain as those (the "Input scale" paragraph at
rc_column_id_rank_batched_* in include/rusty_compression_amd.h) by the cases and checkers of tests/scale_cases.py.

Per test one call on one stacked batch of every kind x every exponent (a neighbour of a block differs from it by up to 2^180 / 2^1800).
Recompression: a carrier says which operand takes 2^e (left: a column ID's C; mid: a two-sided ID's X; s: an SVD's s; split: every
operand extreme, the product at unit scale).  Per block s_out is descaled exactly and the family's own check_block runs against the
unit-scale dense product, then u, vt, the rank and the descaled s_out are held to the e = 0 entry of the same batch bit for bit.
Residual norms: a and the factor a compressor would return at scale take 2^e; err, nrm and e are descaled and held to
residual_ref.bound, e bit for bit to the unit entry's.  tests/test_scale_cases_cpu.py shows that the host passes these checkers at every
cell and that models with plain sums of squares do not.  Every cell of a batch is checked before a test fails.

Before mid and s (complex: any operand) were normalised and the f64 / c64 sums of squares were binned, these tests failed as that file's
planted models do: inf, NaN or rank 0 from the recompressions at the outer and edge exponents, err = nrm = 0 or inf from the f64 / c64
residual norms at -900, +510 and +900; the f32 / c32 residual tests passed and pin that their single f64 accumulator is enough."""
import ctypes

import numpy as np
import pytest
import torch

import rusty_compression_amd as rc
from rusty_compression_amd import _lib
from tests import range_step_ref as ref
from tests import scale_cases as sc
from tests import test_gpu_batched_recompress as brc
from tests import test_gpu_batched_recompress_complex as brcc
from tests.helpers import TOL, npy
from tests.test_gpu_batched_scales import ALL, REAL, call, expected_rank, for_every_cell, tol_of, tt

pytestmark = pytest.mark.gpu

RECOMPRESS = {
    ("small", False): rc.lowrank_recompress_batched, ("small", True): rc.lowrank_recompress_batched_complex,
    ("tall", False): rc.lowrank_recompress_tall_batched, ("tall", True): rc.lowrank_recompress_tall_batched_complex,
    ("large", False): rc.lowrank_recompress_large_batched, ("large", True): rc.lowrank_recompress_large_batched_complex,
}


def dev(x):
    return None if x is None else tt(x)


# ------------------------------------------------------------------------------------------------ 1. recompression, every carrier
@pytest.mark.parametrize("dtype", ALL)
@pytest.mark.parametrize("carrier", list(sc.CARRIERS))
@pytest.mark.parametrize("family,shape", [(fam, sh) for fam, shapes in sc.RECOMPRESS_SHAPES.items() for sh in shapes])
def test_recompression_at_every_scale(family, shape, carrier, dtype):
    m, n, K = shape
    units, cells, (left, right, mid, s), refs = sc.recompress_batch(shape, dtype, carrier)
    u, s_out, vt, ranks = call(RECOMPRESS[(family, sc.is_complex(dtype))], tt(left), tt(right), K, 0.0, mid=dev(mid), s=dev(s))

    def check(idx, i, e):
        assert ranks[idx] == K
        j = sc.unit_cell(cells, i)
        sc.check_recompress(refs[i], carrier, e, u[idx], s_out[idx], vt[idx], ranks[idx], K, dtype, (u[j], s_out[j], vt[j], ranks[j]))

    for_every_cell(cells, check, sc.recompress_kinds(carrier, dtype))


# ------------------------------------------------------------------------------------------------ 2. residual norms, every mode
def residual_fn(dtype):
    return rc.lowrank_residual_batched_complex if sc.is_complex(dtype) else rc.lowrank_residual_batched


@pytest.mark.parametrize("dtype", ALL)
@pytest.mark.parametrize("mode", list(sc.RESIDUAL_CARRIER))
@pytest.mark.parametrize("m,n,K", sc.RESIDUAL_SHAPES)
def test_residual_norms_at_every_scale(m, n, K, mode, dtype):
    units, cells, st = sc.residual_batch((m, n, K), dtype, mode)
    args = (tt(st["a"]), tt(st["left"]), tt(st["right"]))
    err, nrm, e_out = call(residual_fn(dtype), *args, mid=dev(st["mid"]), s=dev(st["s"]), want_residual=True)
    err2, nrm2 = call(residual_fn(dtype), *args, mid=dev(st["mid"]), s=dev(st["s"]), want_residual=False)
    assert sc.same_bits(err, err2) and sc.same_bits(nrm, nrm2)  # the norms do not depend on whether e is written

    def check(idx, i, e):
        sc.check_residual(units[i], e, err[idx], nrm[idx], e_out[idx], e_out[sc.unit_cell(cells, i)], dtype)

    for_every_cell(cells, check, sc.RESIDUAL_KINDS)


# ------------------------------------------------------------------------------------------------ 3. the chains
CHAIN_ID_SHAPE = sc.ID_SHAPES[0]  # (96, 40, 40)
CHAIN_SVD_SHAPE, CHAIN_SVD_K = (60, 30), 12


def chain_reference(left, right, mid, s, q, dtype):
    """(a, sigma, oracle SVD) of the unit-scale dense product of a chain's first stage at inner rank q (its e = 0 outputs)."""
    mod = brcc if sc.is_complex(dtype) else brc
    a, sigma = mod.dense(left, right, mid, s, q)
    from oracle import ref_lapack as o

    return a, sigma, o.SVD.compute_from(a)


def check_chain(cells, units_a, stacked_a, first, dtype, fn_second, fn_residual, kk):
    """first = dict(left, right, mid, s, ranks) of the first stage's outputs on the stacked batch (mid / s None where absent; the operand
    that carries 2^e is whichever the compressor returns at scale).  Runs the recompression and the residual call on them and checks every
    cell: check_recompress against the dense product of the unit cell's factors, check_residual against the unit block."""
    u, s_out, vt, ranks = fn_second()
    err, nrm, e_out = fn_residual(u, s_out, vt, ranks)
    refs = {}

    def check(idx, i, e):
        j = sc.unit_cell(cells, i)
        q = int(first["ranks"][j]) if first["ranks"] is not None else first["left"].shape[2]
        assert first["ranks"] is None or first["ranks"][idx] == q
        if i not in refs:
            pick = lambda x: None if x is None else x[j]  # noqa: E731
            refs[i] = chain_reference(first["left"][j], first["right"][j], pick(first["mid"]), pick(first["s"]), q, dtype)
        sc.check_recompress(refs[i], "left", e, u[idx], s_out[idx], vt[idx], ranks[idx], kk, dtype, (u[j], s_out[j], vt[j], ranks[j]))
        r = int(ranks[j])
        f = {"a": units_a[i], "left": u[j][:, :r], "right": vt[j][:r], "mid": None, "s": s_out[j][:r]}
        sc.check_residual(f, e, err[idx], nrm[idx], e_out[idx], e_out[j], dtype)

    for_every_cell(cells, check)


@pytest.mark.parametrize("dtype", ALL)
def test_column_id_then_to_svd_then_residual_at_every_scale(dtype):
    m, n, k = CHAIN_ID_SHAPE
    cx = sc.is_complex(dtype)
    units, cells, stacked = sc.batch((m, n), dtype)
    tol = tol_of(dtype)
    a = tt(stacked)
    c, z, ind, ranks = rc.column_id_rank_batched(a, k, tol)
    first = {"left": npy(c), "right": npy(z), "mid": None, "s": None, "ranks": npy(ranks)}
    to_svd = rc.column_id_to_svd_batched_complex if cx else rc.column_id_to_svd_batched
    res = rc.svd_residual_batched_complex if cx else rc.svd_residual_batched
    check_chain(cells, units, stacked, first, dtype, lambda: call(to_svd, c, z, ranks, k, tol),
                lambda u, s, vt, r: call(res, a, tt(u), tt(s), tt(vt), tt(r), want_residual=True), k)


@pytest.mark.parametrize("dtype", ALL)
def test_two_sided_id_then_to_svd_then_residual_at_every_scale(dtype):
    m, n, k = CHAIN_ID_SHAPE
    cx = sc.is_complex(dtype)
    units, cells, stacked = sc.batch((m, n), dtype)
    tol = tol_of(dtype)
    a = tt(stacked)
    c, x, rr, row_ind, col_ind, ranks = rc.two_sided_id_rank_batched(a, k, tol)
    first = {"left": npy(c), "right": npy(rr), "mid": npy(x), "s": None, "ranks": npy(ranks)}
    to_svd = rc.two_sided_id_to_svd_batched_complex if cx else rc.two_sided_id_to_svd_batched
    res = rc.svd_residual_batched_complex if cx else rc.svd_residual_batched
    check_chain(cells, units, stacked, first, dtype, lambda: call(to_svd, c, x, rr, ranks, k, tol),
                lambda u, s, vt, r: call(res, a, tt(u), tt(s), tt(vt), tt(r), want_residual=True), k)


@pytest.mark.parametrize("dtype", ALL)
def test_svd_then_svd_add_then_residual_at_every_scale(dtype):
    """Two batches of SVDs at 2^e (the batch, and the batch with its kinds rotated by one: the same exponent per cell) are added and
    rounded: s = [s1, s2] carries 2^e into the recompression.  The residual is taken against the sum of the two unit blocks."""
    m, n = CHAIN_SVD_SHAPE
    k = CHAIN_SVD_K
    cx = sc.is_complex(dtype)
    units, cells, stacked = sc.batch((m, n), dtype)
    tol = tol_of(dtype)
    other = [cells.index(((i + 1) % len(sc.KINDS), e)) for i, e in cells]
    svd = rc.svd_rank_batched_complex if cx else rc.svd_rank_batched
    u1, s1, vt1, _ = svd(tt(stacked), k, tol)
    u2, s2, vt2 = u1[other], s1[other], vt1[other]
    sums = [(units[i] + units[(i + 1) % len(sc.KINDS)]).astype(dtype) for i in range(len(sc.KINDS))]
    a_sum = tt(np.stack([sc.scale(sums[i], e) for i, e in cells]))
    first = {"left": np.concatenate([npy(u1), npy(u2)], axis=2), "right": np.concatenate([npy(vt1), npy(vt2)], axis=1), "mid": None,
             "s": np.concatenate([npy(s1)[:, :k], npy(s2)[:, :k]], axis=1), "ranks": None}
    add = rc.svd_add_batched_complex if cx else rc.svd_add_batched
    res = rc.svd_residual_batched_complex if cx else rc.svd_residual_batched

    def residual(u, s, vt, r):
        return call(res, a_sum, tt(u), tt(s), tt(vt), tt(r), want_residual=True)

    u, s_out, vt, ranks = call(add, u1, s1, vt1, u2, s2, vt2, 2 * k, tol)
    err, nrm, e_out = residual(u, s_out, vt, ranks)
    refs = {}

    def check(idx, i, e):
        j = sc.unit_cell(cells, i)
        if i not in refs:
            refs[i] = chain_reference(first["left"][j], first["right"][j], None, first["s"][j], 2 * k, dtype)
        sc.check_recompress(refs[i], "s", e, u[idx], s_out[idx], vt[idx], ranks[idx], 2 * k, dtype, (u[j], s_out[j], vt[j], ranks[j]))
        r = int(ranks[j])
        f = {"a": sums[i], "left": u[j][:, :r], "right": vt[j][:r], "mid": None, "s": s_out[j][:r]}
        sc.check_residual(f, e, err[idx], nrm[idx], e_out[idx], e_out[j], dtype)

    for_every_cell(cells, check)


# ------------------------------------------------------------------------------------------------ 4. one wide real block
@pytest.mark.parametrize("dtype", REAL)
def test_wide_sketched_svd_at_every_scale(dtype):
    """sketch_svd_rank_large_batched on 130 x 513 blocks: the sketch product, the tall recompression of the range step and the large
    recompression of (P, Q) in one chain; s carries the scale, U and Vt are the unit-scale ones bit for bit."""
    m, n, l = 130, 513, 24
    units, cells, stacked = sc.batch((m, n), dtype)
    om = sc.omega((m, n), l, dtype)
    tol = tol_of(dtype)
    u, s, vt, ranks = call(rc.sketch_svd_rank_large_batched, tt(stacked), l, tol, 1, omega=tt(om))
    host = {}

    def check(idx, i, e):
        r = int(ranks[idx])
        if i not in host:
            host[i] = ref.svd_power(units[i], om, l, tol, 1)[:2]
        oerr, orank = host[i]
        assert r == orank == expected_rank((m, n), i, l)
        u0, s0, vt0 = u[idx][:, :r].astype(np.float64), sc.descale(s[idx], e)[:r].astype(np.float64), vt[idx][:r].astype(np.float64)
        assert max(np.abs(u0.T @ u0 - np.eye(r)).max(), np.abs(vt0 @ vt0.T - np.eye(r)).max()) <= 4 * TOL[np.dtype(dtype)]["orth"]
        assert np.all(np.diff(s0) <= 0) and s0[-1] > 0
        a64 = units[i].astype(np.float64)
        err = np.linalg.norm(a64 - (u0 * s0) @ vt0) / np.linalg.norm(a64)
        assert err <= 1.5 * oerr + 100 * np.finfo(dtype).eps, (err, oerr)
        j = sc.unit_cell(cells, i)
        sc.assert_same_as_unit(("u", "s", "vt", "ranks"), (u[j], s[j], vt[j], ranks[j]), (u[idx], sc.descale(s[idx], e), vt[idx], ranks[idx]))

    for_every_cell(cells, check)


# ------------------------------------------------------------------------------------------------ 5. graph capture at 2^-90
def test_graph_capture_replays_the_eager_bits_at_the_smallest_scale():
    """The f32 recompression with every operand present, the split carrier at 2^-90, captured and replayed: the eager call's bits."""
    m, n, K = sc.RECOMPRESS_SHAPES["small"][1]
    units, cells, (left, right, mid, s), refs = sc.recompress_batch((m, n, K), np.float32, "split")
    sel = [idx for idx, (_, e) in enumerate(cells) if e == min(sc.E32)]
    cnt = len(sel)
    lib = _lib.lib()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        lf, rt, md, sv = tt(left[sel]), tt(right[sel]), tt(mid[sel]), tt(s[sel])
        eager = tuple(npy(t) for t in rc.lowrank_recompress_batched(lf, rt, K, 0.0, mid=md, s=sv))
        torch.cuda.synchronize()
        assert list(eager[3]) == [K] * cnt
        ctx = _lib.Context(torch.cuda.current_device(), st.cuda_stream)
        u = torch.zeros((cnt, m, K), dtype=lf.dtype, device=lf.device)
        s_out = torch.zeros((cnt, K), dtype=lf.dtype, device=lf.device)
        vt = torch.zeros((cnt, K, n), dtype=lf.dtype, device=lf.device)
        ranks = torch.zeros(cnt, dtype=torch.int64, device=lf.device)
        st.synchronize()

        def view(t):
            return _lib.rc_matrix(t.data_ptr(), t.shape[1], t.shape[2], t.stride(1), t.stride(2)), ctypes.c_int64(t.stride(0))

        args = (  # the binding's own argument list (batch._lowrank_recompress_batched)
*view(lf), *view(md), ctypes.c_void_p(sv.data_ptr()), ctypes.c_int64(sv.stride(0)), *view(rt), _lib.i64p(None), ctypes.c_int32(cnt),
            ctypes.c_int64(K), ctypes.c_double(0.0), *view(u), ctypes.c_void_p(s_out.data_ptr()), *view(vt), _lib.i64p(ranks))
        ctx.check(lib.rc_lowrank_recompress_batched_f32(ctx._h, *args))  # eager once: sizes the workspace
        ctx.synchronize()
        ctx.get_health()
        for t in (u, s_out, vt, ranks):
            t.zero_()
        st.synchronize()
        graph = ctypes.c_void_p(None)
        ctx.check(lib.rc_graph_begin_capture(ctx._h))
        ctx.check(lib.rc_lowrank_recompress_batched_f32(ctx._h, *args))
        ctx.check(lib.rc_graph_end_capture(ctx._h, ctypes.byref(graph)))
        try:
            ctx.check(lib.rc_graph_launch(ctx._h, graph))
            ctx.synchronize()
            for p, q in zip(eager, (u, s_out, vt, ranks)):
                assert sc.same_bits(p, npy(q))
            assert ctx.get_health() == 0
        finally:
            ctx.check(lib.rc_graph_destroy(ctx._h, graph))
            ctx.close()
