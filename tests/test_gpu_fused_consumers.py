"""RC_OPT_FUSED_CONSUMERS (include/rusty_compression_amd.h): rc_rsvd_id_f64 with the pivoted QR of B = Q^H A and the Jacobi SVD of
the 128 x 128 core of B in one launch (k_wq_jacobi_fused) against the order it replaces (pivoted-QR / ID branch, then SVD branch).

Neither factorization changes its arithmetic: the pivoted QR is k_wq_coop's body run as one stage (RC_WQ_STAGES documents that the
stages give the bits of the single launch), and the Jacobi runs its 64 column pairs on 32 lane groups, two pairs each, every
pair with the instruction sequence it had on 64 groups.  So EVERY output is compared bit for bit between option off and on,
eager and replayed from a captured graph, at RC_OPT_CONCURRENCY_HINT 1 and 4."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import rusty_compression_amd as rc
from tests.helpers import npy

pytestmark = pytest.mark.gpu

FUSED_OP = "+ jacobi_svd"   # the stage timers' name of the fused launch: "op:geqp3_wide_coop MxN + jacobi_svd n=128 wgs=G+2"
ID_OUTPUTS = ("qr_q", "qr_r", "qr_ind", "id_c", "id_z", "range_q")
SVD_OUTPUTS = ("s", "u", "vt")


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


def _all_runs(a, k, p, seed, settings):
    """a through rc_rsvd_id_f64 on one context for every (hint, slots, fused) of `settings`: eagerly, replayed from a captured
    graph, and once more eagerly under the stage timers (for the names of what ran).  Returns {setting: (eager outputs, replayed
    outputs, op names)} with the outputs on the host; the health word was zero after every run."""
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

        for hint, slots, fused in settings:
            ctx.set_option(_lib.RC_OPT_CONCURRENCY_HINT, hint)
            ctx.set_option(_lib.RC_OPT_KERNEL_SLOTS, slots)
            ctx.set_option(_lib.RC_OPT_FUSED_CONSUMERS, fused)
            run()
            ctx.synchronize()
            assert ctx.get_health() == 0, (hint, slots, fused, "eager")
            eager = {k_: npy(v).copy() for k_, v in b.items()}
            graph = ctypes.c_void_p(None)
            ctx.check(lib.rc_graph_begin_capture(ctx._h))
            run()
            ctx.check(lib.rc_graph_end_capture(ctx._h, ctypes.byref(graph)))
            for t in b.values():
                t.zero_()
            ctx.check(lib.rc_graph_launch(ctx._h, graph))
            ctx.synchronize()
            assert ctx.get_health() == 0, (hint, slots, fused, "replayed")
            replayed = {k_: npy(v).copy() for k_, v in b.items()}
            ctx.check(lib.rc_graph_destroy(ctx._h, graph))
            lib.rc_profile_enable(ctx._h, 1)
            lib.rc_profile_reset(ctx._h)
            run()
            names = _op_names(ctx, lib)
            lib.rc_profile_enable(ctx._h, 0)
            ctx.synchronize()
            assert ctx.get_health() == 0, (hint, slots, fused, "timed")
            out[(hint, slots, fused)] = (eager, replayed, names)
        ctx.close()
    return out


def _assert_same_bits(x, y, what):
    for key in ID_OUTPUTS + SVD_OUTPUTS:
        assert np.array_equal(x[key], y[key]), (what, key, float(np.abs(x[key].astype(np.float64) - y[key].astype(np.float64)).max()))


def _took_fused_launch(names):
    return any(FUSED_OP in nm for nm in names)


def _check_off_against_on(runs, hints=(1, 4), qualifies=True):
    for hint in hints:
        off_e, off_r, off_names = runs[(hint, 4, 0)]
        on_e, on_r, on_names = runs[(hint, 4, 1)]
        assert not _took_fused_launch(off_names), hint
        assert _took_fused_launch(on_names) == qualifies, (hint, on_names)
        _assert_same_bits(off_e, on_e, ("eager off / on", hint))
        _assert_same_bits(off_e, off_r, ("off: eager / replayed", hint))
        _assert_same_bits(on_e, on_r, ("on: eager / replayed", hint))
        d = float(np.abs(off_e["s"] - on_e["s"]).max() / off_e["s"][0])
        print("hint %d: largest off/on difference of s relative to s[0]: %.3e" % (hint, d))


SETTINGS = [(1, 4, 0), (1, 4, 1), (4, 4, 0), (4, 4, 1)]


def test_headline_shape_gives_the_same_bits_off_and_on():
    """8192^2 Gaussian, k = 128, p = 5 (what bench.py times): the fused launch runs with the option on at hints 1 and 4 and
    all nine outputs equal those of the old order bit for bit, eagerly and replayed."""
    a = rc.random_gaussian((8192, 8192), rc.Rng(11), torch.float64)
    runs = _all_runs(a, 128, 5, 5, SETTINGS)
    _check_off_against_on(runs)
    g = runs[(4, 4, 1)][0]
    assert np.all(g["s"][:-1] >= g["s"][1:]) and g["s"][-1] > 0


def test_smaller_qualifying_shape_and_the_regime_of_many_kernels_in_flight():
    """4096 x 2048 (B is 128 x 2048: eight cooperative workgroups + the Jacobi's two).  With min(hint, slots) >= 8 the chip is the
    bound and the staged pivoted QR stays: the option then changes nothing, not even the launches."""
    a = rc.random_gaussian((4096, 2048), rc.Rng(12), torch.float64)
    runs = _all_runs(a, 128, 5, 6, SETTINGS + [(44, 24, 0), (44, 24, 1)])
    _check_off_against_on(runs)
    off, on = runs[(44, 24, 0)], runs[(44, 24, 1)]
    assert not _took_fused_launch(on[2]) and not _took_fused_launch(off[2])
    _assert_same_bits(off[0], on[0], "many in flight: off / on")
    _assert_same_bits(on[0], on[1], "many in flight: eager / replayed")


@pytest.mark.parametrize("case", ["1 + 1e-9 r", "all equal", "two clusters"])
def test_clustered_and_repeated_singular_values_in_the_fused_core(case):
    """The singular values of test_svd_of_clustered_and_repeated_singular_values on a 2048 x 2048 matrix of rank 128, compressed
    with k = 128, p = 0: B and its 128 x 128 core carry exactly these values.  Off and on agree bit for bit; the values
    themselves and the orthogonality of the factors hold the bounds of that test."""
    n, r = 2048, 128
    rng = np.random.default_rng(2048 * 1000 + r)
    qa = np.linalg.qr(rng.standard_normal((n, r)))[0]
    qb = np.linalg.qr(rng.standard_normal((n, r)))[0]
    sig = {"1 + 1e-9 r": 1.0 + 1e-9 * rng.standard_normal(r), "all equal": np.ones(r),
           "two clusters": np.where(np.arange(r) % 2 == 0, 1.0, 0.5 + 1e-12 * np.arange(r))}[case]
    a = (qa * sig) @ qb.T
    runs = _all_runs(torch.from_numpy(a), r, 0, 9, SETTINGS)
    _check_off_against_on(runs)
    g = runs[(4, 4, 1)][0]
    so = np.sort(sig)[::-1]
    assert np.abs(g["s"] - so).max() <= 1e-12 * so[0]
    assert np.abs(g["u"].T @ g["u"] - np.eye(r)).max() <= 1e-12
    assert np.abs(g["vt"] @ g["vt"].T - np.eye(r)).max() <= 1e-12
    assert np.linalg.norm((g["u"] * g["s"]) @ g["vt"] - a) / np.linalg.norm(a) <= 1e-12


def test_rank_64_does_not_qualify_and_takes_the_old_order():
    """k = 64: the core is 64 x 64, the fused launch is built for 128 -- the option is ignored."""
    a = rc.random_gaussian((2048, 2048), rc.Rng(13), torch.float64)
    runs = _all_runs(a, 64, 5, 7, SETTINGS)
    _check_off_against_on(runs, qualifies=False)


def test_fused_launch_on_fresh_workspace_memory():
    """The regression of test_results_do_not_depend_on_what_fresh_workspace_memory_holds for the fused launch: a fresh process
    whose FIRST call is a qualifying rc_rsvd_id_f64 (option on, its default), plain and with RC_DEBUG_POISON_WORKSPACE=1."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

    def digests(extra):
        env = dict(os.environ, **extra)
        res = subprocess.run([sys.executable, os.path.join(root, "tests", "fused_consumers_worker.py")], env=env, capture_output=True, text=True, timeout=600)
        assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
        line = [ln for ln in res.stdout.splitlines() if ln.startswith("DIGESTS ")][-1]
        return json.loads(line[len("DIGESTS "):])

    plain, poisoned = digests({"RC_DEBUG_POISON_WORKSPACE": "0"}), digests({"RC_DEBUG_POISON_WORKSPACE": "1"})
    assert plain["fused_launch_ran"] and poisoned["fused_launch_ran"]
    assert plain["health"] == 0 and poisoned["health"] == 0
    assert plain == poisoned, {k: (plain[k], poisoned[k]) for k in plain if plain[k] != poisoned[k]}
