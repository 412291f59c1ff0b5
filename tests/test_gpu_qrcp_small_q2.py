"""Q2 of the small pivoted QR on several workgroups (k_qrcp_small<T, 18, 1024, true> + k_qrcp_small_q2, kernels_tsqr.hip).

With fewer than 8 compressions side by side (the smaller of RC_OPT_CONCURRENCY_HINT and RC_OPT_KERNEL_SLOTS) the tall-skinny pivoted QR factors its n x n triangle
(64 < n <= 144) in one workgroup, hands the factored LDS image over and forms the columns of Q2 on several workgroups; at 8 or
more Q2 is formed inside the one-workgroup kernel.  Every column is formed by the same calls in the same order from the same
image, so Q, R and ind of rc_pivoted_qr_f64 are compared bit for bit between hint 1 (spread) and hint 8 (in-kernel), both at 8
kernel slots (at the default of 4 slots a hint of 8 still means 4 side by side).  The shapes
have fewer than 32 output tiles in every product, so the hint changes no split count: the stage timers must show the same
"splits=" names in both runs, and then a difference can only come from the Q2 path."""
import ctypes

import numpy as np
import pytest
import torch

import rusty_compression_amd as rc
from oracle import ref_lapack as o
from tests.helpers import npy, rel

pytestmark = pytest.mark.gpu

Q2_OP = "qrcp_small_q2"   # the stage timers' name of the separate Q2 launch: "op:qrcp_small_q2 n=N cols=K wgs=G"


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


def _pivoted_qr_at_hints(a, k, hints=(1, 8)):
    """{hint: (q, r, ind, names)} of rc_pivoted_qr_f64 (m x n -> q m x k, r k x n) on one context; outputs poisoned before each run."""
    from rusty_compression_amd import _lib

    lib = _lib.lib()
    m, n = a.shape
    st = torch.cuda.Stream()
    out = {}
    with torch.cuda.stream(st):
        ctx = _lib.Context(torch.cuda.current_device(), st.cuda_stream)
        ta = torch.from_numpy(a).to("cuda")
        q = torch.empty((m, k), dtype=torch.float64, device="cuda")
        r = torch.empty((k, n), dtype=torch.float64, device="cuda")
        ind = torch.empty(n, dtype=torch.int64, device="cuda")
        st.synchronize()
        ctx.set_option(_lib.RC_OPT_KERNEL_SLOTS, 8)
        for hint in hints:
            ctx.set_option(_lib.RC_OPT_CONCURRENCY_HINT, hint)
            q.fill_(float("nan")), r.fill_(float("nan")), ind.fill_(-1)
            lib.rc_profile_enable(ctx._h, 1)
            lib.rc_profile_reset(ctx._h)
            ctx.call("rc_pivoted_qr_f64", _lib.mat(ta), _lib.mat(q), _lib.mat(r), ctypes.c_void_p(ind.data_ptr()))
            names = _op_names(ctx, lib)
            lib.rc_profile_enable(ctx._h, 0)
            ctx.synchronize()
            assert ctx.get_health() == 0, (hint, ctx.get_health())
            out[hint] = (npy(q).copy(), npy(r).copy(), npy(ind).copy(), names)
        ctx.close()
    return out


def _check_spread_against_in_kernel(a, k, spread_expected=True):
    runs = _pivoted_qr_at_hints(a, k)
    (q1, r1, i1, n1), (q8, r8, i8, n8) = runs[1], runs[8]
    assert any(Q2_OP in nm for nm in n1) == spread_expected, n1
    assert not any(Q2_OP in nm for nm in n8), n8
    splits = lambda names: sorted(nm for nm in names if "splits=" in nm)  # noqa: E731
    assert splits(n1) == splits(n8), (splits(n1), splits(n8))
    assert np.array_equal(i1, i8)
    assert np.array_equal(r1, r8), float(np.abs(r1 - r8).max())
    assert np.array_equal(q1, q8), float(np.abs(q1 - q8).max())
    n = a.shape[1]
    assert np.array_equal(np.sort(i1), np.arange(n))
    assert np.abs(q1.T @ q1 - np.eye(k)).max() <= 1e-13   # (the bound of tests/test_gpu_parity.py for the tall pivoted QR)
    return q1, r1, i1


def test_smallest_n_of_the_instance():
    """1024 x 65: n = 65 is the smallest triangle the <18, 1024> instance takes; 65 columns of Q2 on 8-column waves leave the last
    workgroup with one column."""
    a = np.random.default_rng(65).standard_normal((1024, 65))
    _check_spread_against_in_kernel(a, 65)


def test_fewer_q2_columns_than_n():
    """1024 x 133 with k = 128 (the small factor of the flagship workload: kmax = 128 steps of a 133 x 133 triangle, 128 columns
    of Q2 with 133 rows each)."""
    a = np.random.default_rng(133).standard_normal((1024, 133))
    q, r, ind = _check_spread_against_in_kernel(a, 128)
    assert rel(q @ r[:, :128], a[:, ind[:128]]) <= 1e-13


def _check_against_lapack(a, got):
    """The tolerances of tests/test_gpu_parity.py::test_tall_pivoted_qr_across_the_register_tile_variants."""
    gq, gr, gi = got
    q, r, ind = o.pivoted_qr(a)
    assert np.array_equal(gi, ind)
    assert rel(gr, r) <= 1e-12 and rel(gq, q) <= 1e-12
    assert np.abs(gq.T @ gq - np.eye(a.shape[1])).max() <= 1e-13


def test_largest_n_of_the_tall_skinny_route_against_lapack():
    """1024 x 139 with k = 139: the largest triangle the tall-skinny route hands to k_qrcp_small (tsqr_supported: the n x n image
    with its four vectors must fit 158 KB of LDS, which ends at n = 139).  139 columns in blocks of 24 (whole waves of 8): the
    last workgroup's block holds 19, its third wave three columns and five idle groups -- and the spread path is held to ?geqp3
    itself, not only to its in-kernel twin."""
    a = np.random.default_rng(139).standard_normal((1024, 139))
    _check_against_lapack(a, _check_spread_against_in_kernel(a, 139))


def test_n_144_stays_on_its_own_path():
    """1024 x 144 with k = 144, the largest n of the <18, 1024> instance: the tall-skinny route does not take it (see above), so
    no run may show the separate Q2 launch, the hints must still agree bit for bit, and the result is ?geqp3's."""
    a = np.random.default_rng(144).standard_normal((1024, 144))
    _check_against_lapack(a, _check_spread_against_in_kernel(a, 144, spread_expected=False))
