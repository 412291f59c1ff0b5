"""The fused launch of RC_OPT_FUSED_CONSUMERS (k_wq_jacobi_fused) on 1024-thread workgroups: the pivoted QR of B = Q^H A holds TWO
columns per 8-lane group on 128 groups (a workgroup still owns 256 columns) and the Jacobi of the 128 x 128 core runs one column
pair per 16-lane group, which is literally the arithmetic of k_jacobi_lds.

The reference is the option-off order: the staged 512-thread k_wq_coop launches (four columns per group on 64 groups) and the
1024-thread k_jacobi_lds.  A column is 8 lanes with rows l8 + 8 e in either layout, its dot products, reductions and ?laqp2
down-dates are per column, and pivot ties are broken by position, not by the lane, wave or workgroup that holds the column -- so
ALL nine outputs of rc_rsvd_id_f64 are compared bit for bit between option off and on, eager and replayed from a captured graph,
at RC_OPT_CONCURRENCY_HINT 1 and 4 (RC_OPT_KERNEL_SLOTS 4), at the smallest shapes where the new column -> group mapping
(c0 + g8 + 128 q, q < 2) can go wrong."""
import ctypes

import numpy as np
import pytest
import torch

import rusty_compression_amd as rc
from tests.helpers import npy

pytestmark = pytest.mark.gpu

FUSED_OP = "+ jacobi_svd"   # the stage timers' name of the fused launch: "op:geqp3_wide_coop MxN + jacobi_svd n=128 wgs=G+2"
OUTPUTS = ("qr_q", "qr_r", "qr_ind", "id_c", "id_z", "range_q", "s", "u", "vt")
SETTINGS = [(1, 4, 0), (1, 4, 1), (4, 4, 0), (4, 4, 1)]   # (hint, kernel slots, fused consumers)


def _buffers(m, n, k):
    from rusty_compression_amd import _lib

    mk = lambda r, c: torch.zeros((r, c), dtype=torch.float64, device="cuda")  # noqa: E731
    b = dict(range_q=mk(m, k), u=mk(m, k), s=torch.zeros(k, dtype=torch.float64, device="cuda"), vt=mk(k, n), qr_q=mk(m, k), qr_r=mk(k, n),
             qr_ind=torch.zeros(n, dtype=torch.int64, device="cuda"), id_c=mk(m, k), id_z=mk(k, n))
    o_ = _lib.rc_rsvd_id_out(_lib.mat(b["range_q"]), _lib.mat(b["u"]), ctypes.c_void_p(b["s"].data_ptr()), _lib.mat(b["vt"]), _lib.mat(b["qr_q"]),
                             _lib.mat(b["qr_r"]), ctypes.c_void_p(b["qr_ind"].data_ptr()), _lib.mat(b["id_c"]), _lib.mat(b["id_z"]))
    return b, o_


def _op_names(ctx, lib):
    cnt = ctypes.c_int32(0)
    ctx.check(lib.rc_profile_count(ctx._h, ctypes.byref(cnt)))
    names = []
    for i in range(cnt.value):
        name = ctypes.create_string_buffer(192)
        ms, calls = ctypes.c_double(0), ctypes.c_int64(0)
        ctx.check(lib.rc_profile_get(ctx._h, i, name, 192, ctypes.byref(ms), ctypes.byref(calls)))
        names.append(name.value.decode())
    return names


def _all_runs(a, k, p, seed):
    """a through rc_rsvd_id_f64 on one context for every setting: eagerly, replayed from a captured graph, and once more eagerly
    under the stage timers (for the names of what ran).  The health word must be zero after every run."""
    from rusty_compression_amd import _lib

    lib = _lib.lib()
    m, n = a.shape
    st = torch.cuda.Stream()
    out = {}
    with torch.cuda.stream(st):
        ctx = _lib.Context(torch.cuda.current_device(), st.cuda_stream)
        a = a.to("cuda")
        st.synchronize()
        b, o_ = _buffers(m, n, k)

        def run():
            ctx.call("rc_rsvd_id_f64", _lib.mat(a), ctypes.c_int64(k), ctypes.c_int64(p), _lib.mat(None), ctypes.c_uint64(seed), ctypes.byref(o_))

        for hint, slots, fused in SETTINGS:
            ctx.set_option(_lib.RC_OPT_CONCURRENCY_HINT, hint)
            ctx.set_option(_lib.RC_OPT_KERNEL_SLOTS, slots)
            ctx.set_option(_lib.RC_OPT_FUSED_CONSUMERS, fused)
            run()
            ctx.synchronize()
            assert ctx.get_health() == 0, (hint, slots, fused, "eager", ctx.get_health())
            eager = {k_: npy(v).copy() for k_, v in b.items()}
            graph = ctypes.c_void_p(None)
            ctx.check(lib.rc_graph_begin_capture(ctx._h))
            run()
            ctx.check(lib.rc_graph_end_capture(ctx._h, ctypes.byref(graph)))
            for t in b.values():
                t.zero_()
            ctx.check(lib.rc_graph_launch(ctx._h, graph))
            ctx.synchronize()
            assert ctx.get_health() == 0, (hint, slots, fused, "replayed", ctx.get_health())
            replayed = {k_: npy(v).copy() for k_, v in b.items()}
            ctx.check(lib.rc_graph_destroy(ctx._h, graph))
            lib.rc_profile_enable(ctx._h, 1)
            lib.rc_profile_reset(ctx._h)
            run()
            names = _op_names(ctx, lib)
            lib.rc_profile_enable(ctx._h, 0)
            ctx.synchronize()
            assert ctx.get_health() == 0, (hint, slots, fused, "timed", ctx.get_health())
            out[(hint, slots, fused)] = (eager, replayed, names)
        ctx.close()
    return out


def _assert_same_bits(x, y, what):
    for key in OUTPUTS:
        assert np.array_equal(x[key], y[key]), (what, key, float(np.abs(x[key].astype(np.float64) - y[key].astype(np.float64)).max()))


def _took_fused_launch(names):
    return any(FUSED_OP in nm for nm in names)


def _check_off_against_on(runs):
    """The eager option-off run is the reference of its hint (bits are promised per setting of min(hint, slots), not across them):
    the option-on run, and both replays, must equal it bit for bit."""
    for hint in (1, 4):
        off_e, off_r, off_names = runs[(hint, 4, 0)]
        on_e, on_r, on_names = runs[(hint, 4, 1)]
        assert not _took_fused_launch(off_names), (hint, off_names)
        assert _took_fused_launch(on_names), (hint, on_names)
        _assert_same_bits(off_e, on_e, ("eager off / on", hint))
        _assert_same_bits(off_e, off_r, ("off: eager / replayed", hint))
        _assert_same_bits(off_e, on_r, ("off eager / on replayed", hint))


def _is_permutation(ind, n):
    return np.array_equal(np.sort(ind), np.arange(n))


def test_smallest_qualifying_shape_every_group_holds_two_columns():
    """1024 x 1024 Gaussian (the tall-skinny QR of the sketch needs n >= 1024): B is 128 x 1024 on g = 4 workgroups of 256 columns
    each, so both column slots of all 128 groups are live in every workgroup."""
    a = rc.random_gaussian((1024, 1024), rc.Rng(21), torch.float64)
    runs = _all_runs(a, 128, 5, 15)
    _check_off_against_on(runs)
    g = runs[(4, 4, 1)][0]
    assert _is_permutation(g["qr_ind"], 1024)
    assert np.all(g["s"][:-1] >= g["s"][1:]) and g["s"][-1] > 0


def test_ragged_workgroups_groups_with_an_empty_second_slot():
    """1024 x 1124 Gaussian: g = 5, cpw = 225.  In every workgroup the groups g8 >= 97 hold a column in slot 0 and none in slot 1
    (cl = g8 + 128 q < nloc, pos[1] = -1, a norm owner l8 = 1 without a column), and the last workgroup holds 224 columns."""
    a = rc.random_gaussian((1024, 1124), rc.Rng(22), torch.float64)
    runs = _all_runs(a, 128, 5, 16)
    _check_off_against_on(runs)
    assert _is_permutation(runs[(4, 4, 1)][0]["qr_ind"], 1124)


def test_repeated_columns_ties_are_broken_by_position():
    """A[:, j] = A0[:, j % 300] with A0 Gaussian 1024 x 300: B has exactly equal columns, hence exactly equal partial norms, and
    the copies lie in different lanes, different waves of the 16-wave workgroup and different workgroups (225 columns each).
    Position breaks the ties, so qr_ind equals the option-off result.  B keeps full row rank (rank 300 >= 133)."""
    a0 = rc.random_gaussian((1024, 300), rc.Rng(23), torch.float64)
    a = a0[:, torch.arange(1124) % 300].contiguous()
    assert torch.equal(a[:, 0], a[:, 300]) and torch.equal(a[:, 0], a[:, 900])
    runs = _all_runs(a, 128, 5, 17)
    _check_off_against_on(runs)
    assert _is_permutation(runs[(4, 4, 1)][0]["qr_ind"], 1124)


def test_clustered_core_on_the_1024_thread_producer_and_consumer():
    """The "all equal" recipe of tests/test_gpu_fused_consumers.py (2048 x 2048, rank 128, p = 0): the rotations of the core stay
    large for many sweeps, which the 1024-thread producer / consumer pair of the fused launch must follow record by record."""
    n, r = 2048, 128
    rng = np.random.default_rng(2048 * 1000 + r)
    qa = np.linalg.qr(rng.standard_normal((n, r)))[0]
    qb = np.linalg.qr(rng.standard_normal((n, r)))[0]
    sig = np.ones(r)
    a = (qa * sig) @ qb.T
    runs = _all_runs(torch.from_numpy(a), r, 0, 9)
    _check_off_against_on(runs)
    g = runs[(4, 4, 1)][0]
    assert np.abs(g["s"] - sig).max() <= 1e-12
    assert np.abs(g["u"].T @ g["u"] - np.eye(r)).max() <= 1e-12
    assert np.abs(g["vt"] @ g["vt"].T - np.eye(r)).max() <= 1e-12
    assert np.linalg.norm((g["u"] * g["s"]) @ g["vt"] - a) / np.linalg.norm(a) <= 1e-12
