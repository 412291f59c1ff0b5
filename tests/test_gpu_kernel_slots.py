"""The kernel-slot model (RC_OPT_KERNEL_SLOTS, include/rusty_compression_amd.h): launches are sized for
min(RC_OPT_CONCURRENCY_HINT, RC_OPT_KERNEL_SLOTS) compressions running side by side, not for the hint alone.

On the cfg3 pipeline (8192^2 f64, k = 128, p = 5, through rc_rsvd_id_f64): settings with the same min(hint, slots) class give the
same bits, the class decides how far the two big products split K (checked on the stage timers' kernel names), and the classes
agree with each other to rounding."""
import ctypes
import re

import numpy as np
import pytest
import torch

import rusty_compression_amd as rc
from tests.helpers import agreed_pivot_prefix, npy, rel

pytestmark = pytest.mark.gpu

N, K, P = 8192, 128, 5
_SPLIT = re.compile(r"kernel:k_splitk_reduce M=(\d+) N=(\d+) splits=(\d+)")


def _buffers():
    from rusty_compression_amd import _lib

    mk = lambda r, c: torch.zeros((r, c), dtype=torch.float64, device="cuda")  # noqa: E731
    b = dict(range_q=mk(N, K), u=mk(N, K), s=torch.zeros(K, dtype=torch.float64, device="cuda"), vt=mk(K, N), qr_q=mk(N, K), qr_r=mk(K, N),
             qr_ind=torch.zeros(N, dtype=torch.int64, device="cuda"), id_c=mk(N, K), id_z=mk(K, N))
    o_ = _lib.rc_rsvd_id_out(_lib.mat(b["range_q"]), _lib.mat(b["u"]), ctypes.c_void_p(b["s"].data_ptr()), _lib.mat(b["vt"]), _lib.mat(b["qr_q"]),
                             _lib.mat(b["qr_r"]), ctypes.c_void_p(b["qr_ind"].data_ptr()), _lib.mat(b["id_c"]), _lib.mat(b["id_z"]))
    return b, o_


@pytest.fixture(scope="module")
def runs():
    """One eager compression of the same seeded input per (hint, slots) setting, on one context: outputs on the host, and the
    split counts of the split-K reductions of the wide products (output >= 128 x 8192), from the stage timers."""
    from rusty_compression_amd import _lib

    lib = _lib.lib()
    st = torch.cuda.Stream()
    out = {}
    with torch.cuda.stream(st):
        ctx = _lib.Context(torch.cuda.current_device(), st.cuda_stream)
        a = rc.random_gaussian((N, N), rc.Rng(11), torch.float64)
        st.synchronize()
        b, o_ = _buffers()
        settings = [(44, None), (4, None), (2, None), (44, 24), (8, 8), (1, None), (44, 1)]
        for hint, slots in settings:
            ctx.set_option(_lib.RC_OPT_CONCURRENCY_HINT, hint)
            ctx.set_option(_lib.RC_OPT_KERNEL_SLOTS, 4 if slots is None else slots)
            lib.rc_profile_enable(ctx._h, 1)
            lib.rc_profile_reset(ctx._h)
            ctx.call("rc_rsvd_id_f64", _lib.mat(a), ctypes.c_int64(K), ctypes.c_int64(P), _lib.mat(None), ctypes.c_uint64(5), ctypes.byref(o_))
            cnt = ctypes.c_int32(0)
            ctx.check(lib.rc_profile_count(ctx._h, ctypes.byref(cnt)))
            splits = set()
            for i in range(cnt.value):
                name = ctypes.create_string_buffer(192)
                ms, calls = ctypes.c_double(0), ctypes.c_int64(0)
                ctx.check(lib.rc_profile_get(ctx._h, i, name, 192, ctypes.byref(ms), ctypes.byref(calls)))
                m_ = _SPLIT.match(name.value.decode())
                if m_ and int(m_.group(1)) * int(m_.group(2)) >= K * N:
                    splits.add(int(m_.group(3)))
            lib.rc_profile_enable(ctx._h, 0)
            ctx.synchronize()
            assert ctx.get_health() == 0
            out[(hint, slots)] = ({k_: npy(v).copy() for k_, v in b.items()}, splits)
        ctx.close()
    return out


def _same_bits(x, y):
    for key in x:
        assert np.array_equal(x[key], y[key]), key


def test_default_slots_cap_a_large_hint_at_four(runs):
    """Hint 44 on the default 4 slots is the 2..7 class: the same bits as hints 4 and 2, the wide products split to 128
    workgroups (32 output tiles x 4)."""
    _same_bits(runs[(44, None)][0], runs[(4, None)][0])
    _same_bits(runs[(44, None)][0], runs[(2, None)][0])
    assert runs[(44, None)][1] == {4}


def test_many_slots_keep_the_unsplit_products(runs):
    """Hint 44 on 24 slots is the path a hint >= 8 took before slots existed: wide products not split, no reduction."""
    _same_bits(runs[(44, 24)][0], runs[(8, 8)][0])
    assert runs[(44, 24)][1] == set()


def test_one_slot_or_hint_one_is_the_lone_launch(runs):
    """min(hint, slots) = 1: a wide product splits until it covers the 256 CUs (32 tiles x 8)."""
    _same_bits(runs[(1, None)][0], runs[(44, 1)][0])
    assert runs[(1, None)][1] == {8}


def test_the_classes_differ_by_rounding_only(runs):
    base = runs[(44, None)][0]
    for other in ((44, 24), (1, None)):
        g = runs[other][0]
        assert rel(g["range_q"], base["range_q"]) <= 1e-12
        assert np.abs(g["s"] - base["s"]).max() / base["s"][0] <= 1e-12
        assert rel((g["u"] * g["s"]) @ g["vt"], (base["u"] * base["s"]) @ base["vt"]) <= 1e-10
        # the same pivots on the prefix the data determine (a disagreement only at a near tie, helpers.agreed_pivot_prefix)
        agreed_pivot_prefix(g["qr_ind"], g["qr_r"], base["qr_ind"], base["qr_r"], np.float64)
        if np.array_equal(g["qr_ind"][:K], base["qr_ind"][:K]):
            assert rel(g["qr_r"], base["qr_r"]) <= 1e-10 and rel(g["id_c"], base["id_c"]) <= 1e-10
