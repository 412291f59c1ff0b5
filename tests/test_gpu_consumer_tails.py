"""The tails of the fused QRCP/Jacobi launch in ONE launch (k_rsvd_id_tails, RC_OPT_FUSED_CONSUMERS = 1): Z solved from the
factored matrix (role of k_id_z<T, false>), Q_b formed on four workgroups of 32 columns (role of k_form_q_small<T, 16>) and R
extracted on a grid-stride range of workgroups (role of k_extract_r), and the left vectors of the core written by the Jacobi
straight into the operand of U = range ub (no copy).

The reference is the option-off order (extract_r, form_q, id_z_from_r as three launches behind the staged QRCP, and the copy).
Every output entry is computed by the same instruction sequence on the same operands, so ALL outputs of rc_rsvd_id_f64 are
compared bit for bit between option off and on within a hint, eager and replayed from a captured graph, and the stage timers
must show the tails launch with the option on and not with it off."""
import ctypes

import numpy as np
import pytest
import torch

import rusty_compression_amd as rc
from tests.helpers import npy

pytestmark = pytest.mark.gpu

TAILS_OP = "tails"          # the stage timers' name of the launch: "op:rsvd_id_tails k=K n=N wgs=Z+Q+R"
OUTPUTS = ("qr_q", "qr_r", "qr_ind", "id_c", "id_z", "range_q", "s", "u", "vt")
SETTINGS = [(1, 4, 0), (1, 4, 1), (4, 4, 0), (4, 4, 1)]   # (hint, kernel slots, fused consumers)


def _buffers(m, n, k, want_cz):
    from rusty_compression_amd import _lib

    mk = lambda r, c: torch.zeros((r, c), dtype=torch.float64, device="cuda")  # noqa: E731
    b = dict(range_q=mk(m, k), u=mk(m, k), s=torch.zeros(k, dtype=torch.float64, device="cuda"), vt=mk(k, n), qr_q=mk(m, k), qr_r=mk(k, n),
             qr_ind=torch.zeros(n, dtype=torch.int64, device="cuda"))
    if want_cz:
        b.update(id_c=mk(m, k), id_z=mk(k, n))
    cz = [_lib.mat(b["id_c"]), _lib.mat(b["id_z"])] if want_cz else [_lib.mat(None), _lib.mat(None)]
    o_ = _lib.rc_rsvd_id_out(_lib.mat(b["range_q"]), _lib.mat(b["u"]), ctypes.c_void_p(b["s"].data_ptr()), _lib.mat(b["vt"]), _lib.mat(b["qr_q"]),
                             _lib.mat(b["qr_r"]), ctypes.c_void_p(b["qr_ind"].data_ptr()), *cz)
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


def _all_runs(a, k, p, seed, want_cz=True):
    """a through rc_rsvd_id_f64 on ONE context for every setting: eagerly, replayed from a captured graph, and once more eagerly
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
        b, o_ = _buffers(m, n, k, want_cz)

        def run():
            ctx.call("rc_rsvd_id_f64", _lib.mat(a), ctypes.c_int64(k), ctypes.c_int64(p), _lib.mat(None), ctypes.c_uint64(seed), ctypes.byref(o_))

        for hint, slots, fused in SETTINGS:
            ctx.set_option(_lib.RC_OPT_CONCURRENCY_HINT, hint)
            ctx.set_option(_lib.RC_OPT_KERNEL_SLOTS, slots)
            ctx.set_option(_lib.RC_OPT_FUSED_CONSUMERS, fused)
            for t in b.values():
                t.zero_()
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
    assert set(x) == set(y)
    for key in OUTPUTS:
        if key in x:
            assert np.array_equal(x[key], y[key]), (what, key, float(np.abs(x[key].astype(np.float64) - y[key].astype(np.float64)).max()))


def _took_tails_launch(names):
    return any(TAILS_OP in nm for nm in names)


def _check_off_against_on(runs, tails_expected=True):
    """The eager option-off run is the reference of its hint (bits are promised per setting of min(hint, slots), not across them):
    the option-on run, and both replays, must equal it bit for bit."""
    for hint in (1, 4):
        off_e, off_r, off_names = runs[(hint, 4, 0)]
        on_e, on_r, on_names = runs[(hint, 4, 1)]
        assert not _took_tails_launch(off_names), (hint, off_names)
        if tails_expected:
            assert _took_tails_launch(on_names), (hint, on_names)
        _assert_same_bits(off_e, on_e, ("eager off / on", hint))
        _assert_same_bits(off_e, off_r, ("off: eager / replayed", hint))
        _assert_same_bits(off_e, on_r, ("off eager / on replayed", hint))


def _is_permutation(ind, n):
    return np.array_equal(np.sort(ind), np.arange(n))


def _z_reproduces_r(g, k):
    """Z = [I | R11^-1 R12] P^T: R11 Z[:, ind] = R up to rounding (a check of Z that does not go through the option-off twin)."""
    r, z, ind = g["qr_r"], g["id_z"], g["qr_ind"]
    zp = z[:, ind]
    assert np.array_equal(zp[:, :k], np.eye(k))
    res = np.linalg.norm(r[:, :k] @ zp - r) / np.linalg.norm(r)
    # backward-stable triangular solve: the residual is O(k eps) relative to |R11| |Z|; |Z| entries of a pivoted QR stay modest
    assert res <= 1e-12, res


def test_smallest_qualifying_shape_four_full_z_workgroups():
    """1024 x 1024 Gaussian, p = 5: the smallest shape the fused path takes.  B is 128 x 1024: the Z role is four full workgroups
    of 256 positions (the first half of workgroup 0 writes identity columns), the Q_b role four workgroups of 32 columns."""
    a = rc.random_gaussian((1024, 1024), rc.Rng(31), torch.float64)
    runs = _all_runs(a, 128, 5, 25)
    _check_off_against_on(runs)
    g = runs[(4, 4, 1)][0]
    assert _is_permutation(g["qr_ind"], 1024)
    _z_reproduces_r(g, 128)
    assert np.abs(g["qr_q"].T @ g["qr_q"] - np.eye(128)).max() <= 1e-12
    assert np.array_equal(np.tril(g["qr_r"], -1), np.zeros_like(g["qr_r"]))


def test_ragged_last_z_workgroup_and_r_role_tail():
    """1024 x 1124 Gaussian: the last Z workgroup holds 100 positions (156 threads own nothing but still load tiles and meet the
    barriers), and 128 * 1124 entries of R are no multiple of the R role's threads (grid-stride tail)."""
    a = rc.random_gaussian((1024, 1124), rc.Rng(32), torch.float64)
    runs = _all_runs(a, 128, 5, 26)
    _check_off_against_on(runs)
    g = runs[(4, 4, 1)][0]
    assert _is_permutation(g["qr_ind"], 1124)
    _z_reproduces_r(g, 128)


def test_repeated_columns_scattered_destinations_cross_workgroups():
    """A[:, j] = A0[:, j % 300] with A0 Gaussian 1024 x 300: the pivots lie outside their own 256-column block, so the Z role's
    destinations id_z[:, ind[p]] of one workgroup are scattered over the blocks of all the others."""
    a0 = rc.random_gaussian((1024, 300), rc.Rng(33), torch.float64)
    a = a0[:, torch.arange(1124) % 300].contiguous()
    assert torch.equal(a[:, 0], a[:, 300]) and torch.equal(a[:, 0], a[:, 900])
    runs = _all_runs(a, 128, 5, 27)
    _check_off_against_on(runs)
    g = runs[(4, 4, 1)][0]
    ind = g["qr_ind"]
    assert _is_permutation(ind, 1124)
    assert np.any(ind // 256 != np.arange(1124) // 256)


def test_without_id_c_and_id_z():
    """1024 x 1024 with id_c / id_z not requested: Q, R, ind and the SVD must still match the option-off order (the tails launch
    then has no Z role, or the separate launches run)."""
    a = rc.random_gaussian((1024, 1024), rc.Rng(31), torch.float64)
    runs = _all_runs(a, 128, 5, 25, want_cz=False)
    _check_off_against_on(runs, tails_expected=False)
    g = runs[(4, 4, 1)][0]
    assert "id_z" not in g and _is_permutation(g["qr_ind"], 1024)
    assert np.abs(g["qr_q"].T @ g["qr_q"] - np.eye(128)).max() <= 1e-12
