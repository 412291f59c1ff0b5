"""The Gram and shallow products of the tall-skinny chain on many small workgroups (gemm_chain, kernels_gemm.hip).

With fewer than 8 compressions side by side (the smaller of RC_OPT_CONCURRENCY_HINT and RC_OPT_KERNEL_SLOTS) gemm_chain cuts the
one 144 x 144 tile of a Gram product into nine of 48 x 48 and the 128-wide tiles of a shallow product (K <= 160 under a tall side
>= 2048) into tiles of 32 or 64 columns, on smaller wave tiles, and keeps the K slabs gemm plans; at 8 and more it is gemm.  Every entry of a product
is the same chain of MFMAs over the same slab either way, so rc_pivoted_qr_f64 and rc_compute_svd_f64 are compared bit for bit
between hint 1 (spread) and hint 8 (gemm's own launch), both at 8 kernel slots, the stage timers must show the same "splits="
names, and rc_last_gemm_kernel_name tells which form the last product of each run took.  The hint-1 result is then held to LAPACK
with the tolerances of tests/test_gpu_parity.py::test_tall_pivoted_qr_across_the_register_tile_variants."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import ref_lapack as o
from tests.helpers import npy, rel
from tests.small_product_cases import op_names

pytestmark = pytest.mark.gpu

# as rc_last_gemm_kernel_name spells them: the instantiations of gemm_chain's spread forms, and gemm's for the same products
SPREAD_SHALLOW_TILES = (",128,32,16,4,2,", ",136,64,16,2,4,")
PARENT_SHALLOW_TILES = (",128,128,16,1,8,", ",136,128,16,2,4,")


def _last_kernel(ctx, lib):
    fn = lib.rc_last_gemm_kernel_name
    fn.restype = ctypes.c_char_p
    fn.argtypes = [ctypes.c_void_p]
    return fn(ctx._h).decode()


def _at_hints(fn, a, outs, hints=(1, 8)):
    """{hint: (outputs..., names, last kernel)} of one entry point on one context at 8 kernel slots; outputs poisoned before each run.
    outs: [(shape, torch dtype)]; a matrix goes in as rc_matrix, a vector as its pointer."""
    from rusty_compression_amd import _lib

    lib = _lib.lib()
    st = torch.cuda.Stream()
    res = {}
    with torch.cuda.stream(st):
        ctx = _lib.Context(torch.cuda.current_device(), st.cuda_stream)
        ta = torch.from_numpy(a).to("cuda")
        bufs = [torch.empty(shape, dtype=dt, device="cuda") for shape, dt in outs]
        args = [_lib.mat(t) if t.dim() == 2 else ctypes.c_void_p(t.data_ptr()) for t in bufs]
        st.synchronize()
        ctx.set_option(_lib.RC_OPT_KERNEL_SLOTS, 8)
        for hint in hints:
            ctx.set_option(_lib.RC_OPT_CONCURRENCY_HINT, hint)
            for t in bufs:
                t.fill_(float("nan") if t.is_floating_point() else -1)
            lib.rc_profile_enable(ctx._h, 1)
            lib.rc_profile_reset(ctx._h)
            ctx.call(fn, _lib.mat(ta), *args)
            names = sorted(op_names(ctx, lib))
            lib.rc_profile_enable(ctx._h, 0)
            ctx.synchronize()
            assert ctx.get_health() == 0, (hint, ctx.get_health())
            res[hint] = tuple(npy(t).copy() for t in bufs) + (names, _last_kernel(ctx, lib))
        ctx.close()
    return res


def _splits(names):
    return [nm for nm in names if "splits=" in nm]


def _pivoted_qr_hint_1_against_8(m, n, k, seed):
    a = np.random.default_rng(seed).standard_normal((m, n))
    runs = _at_hints("rc_pivoted_qr_f64", a, [((m, k), torch.float64), ((k, n), torch.float64), ((n,), torch.int64)])
    (q1, r1, i1, n1, last1), (q8, r8, i8, n8, last8) = runs[1], runs[8]
    print("%d x %d k %d: hint 1 %s | hint 8 %s | %s" % (m, n, k, last1, last8, _splits(n1)))
    assert _splits(n1) == _splits(n8), (_splits(n1), _splits(n8))
    assert np.array_equal(i1, i8)
    assert np.array_equal(r1, r8), float(np.abs(r1 - r8).max())
    assert np.array_equal(q1, q8), float(np.abs(q1 - q8).max())
    # against ?geqp3: pivots, and Q and R of the first k steps (final after k steps; columns >= k of R in LAPACK's order of the same indices)
    oq, orr, oind = (np.asarray(x) for x in o.pivoted_qr(a))
    assert np.array_equal(i1[:k], oind[:k]) and np.array_equal(np.sort(i1), np.arange(n))
    opos = np.empty(n, dtype=np.int64)
    opos[oind] = np.arange(n)
    print("  rel R %.3e  rel Q %.3e  orth %.3e" % (rel(r1, orr[:k][:, opos[i1]]), rel(q1, oq[:, :k]), np.abs(q1.T @ q1 - np.eye(k)).max()))
    assert rel(r1, orr[:k][:, opos[i1]]) <= 1e-12 and rel(q1, oq[:, :k]) <= 1e-12
    assert np.abs(q1.T @ q1 - np.eye(k)).max() <= 1e-13
    return n1, last1, last8


def _gram_labels(names, n, kdim):
    return [nm for nm in names if nm.startswith("kernel:k_gemm_mfma<f64> M=%d N=%d K=%d" % (n, n, kdim))]


def test_smallest_tall_side_of_the_shallow_arm_two_slabs():
    """2048 x 133, k = 128: 16 tiles of 128 columns, so gemm's planner cuts K = 133 (no multiple of 16) into two slabs of 80 and
    53 and the spread form must show the same reduction; the last product, Q = q1 w (128 x 2048 x 133), is a shallow one."""
    names, last1, last8 = _pivoted_qr_hint_1_against_8(2048, 133, 128, 2133)
    assert any(nm.startswith("kernel:k_splitk_reduce M=128 N=2048 splits=2") for nm in names), _splits(names)
    assert any(t in last1 for t in SPREAD_SHALLOW_TILES), last1
    assert any(t in last8 for t in PARENT_SHALLOW_TILES), last8


def test_unsplit_shallow_products_and_the_136_row_instance():
    """4096 x 133, k = 128: 32 tiles, no K split.  q1 = y r1i is the 133-row product (136 x 64 tiles of 68 x 16 wave tiles), the
    last one the 128-row product."""
    names, last1, last8 = _pivoted_qr_hint_1_against_8(4096, 133, 128, 4133)
    assert not any("N=4096 splits=" in nm for nm in names), _splits(names)
    assert any(nm.startswith("kernel:k_gemm_mfma<f64> M=133 N=4096 K=133") for nm in names), names
    assert any(t in last1 for t in SPREAD_SHALLOW_TILES), last1
    assert any(t in last8 for t in PARENT_SHALLOW_TILES), last8


def test_smallest_n_of_the_gram_arm():
    """2048 x 81, k = 81: two 48-wide tiles a side, the second with 33 live rows / columns.  The tall products have M = 81 and take
    gemm's 80 < M <= 128 shallow tile too."""
    names, last1, last8 = _pivoted_qr_hint_1_against_8(2048, 81, 81, 2081)
    assert len(_gram_labels(names, 81, 2048)) == 1, names
    assert any(t in last1 for t in SPREAD_SHALLOW_TILES), last1
    assert any(t in last8 for t in PARENT_SHALLOW_TILES), last8


def test_largest_n_of_the_route_gram_spreads_shallow_forwards():
    """2048 x 139, k = 139: the Gram products spread (three tiles a side, the third with 43 live rows); the tall products have
    M = 139 > 136 and must take gemm's launch at either hint."""
    names, last1, last8 = _pivoted_qr_hint_1_against_8(2048, 139, 139, 2139)
    assert len(_gram_labels(names, 139, 2048)) == 1, names
    assert last1 == last8 and not any(t in last1 for t in SPREAD_SHALLOW_TILES), (last1, last8)


def test_tall_side_no_multiple_of_the_tile_and_gram_refused_by_the_pipelined_loop():
    """2049 x 128, k = 128: 65 tiles of 32 columns, the last with one; K = 2049 of the Gram products is no multiple of 16, so the
    pipelined loop refuses them and gemm_chain forwards them to gemm."""
    names, last1, last8 = _pivoted_qr_hint_1_against_8(2049, 128, 128, 2049)
    assert len(_gram_labels(names, 128, 2049)) == 1, names
    assert any(t in last1 for t in SPREAD_SHALLOW_TILES), last1
    assert any(t in last8 for t in PARENT_SHALLOW_TILES), last8


def test_compute_svd_tall_and_wide():
    """rc_compute_svd_f64 of a 4096 x 128 Gaussian and of its transpose: svd_core's tall path (both Gram products and q1 = y r1i
    spread) and, for the wide matrix, svd_finish's vt = small^T q1^T, a shallow product and the last launch.  The tall matrix ends
    with u = q1 small, which is not one of the chain's products of gemm_chain and names gemm's instantiation at either hint.
    (The M- and K-contiguous <1,1,...> layout of vt inside rc_rsvd_id_f64 runs in tests/test_gpu_spread_switch.py.)"""
    a = np.random.default_rng(4128).standard_normal((4096, 128))
    for x, transposed in ((a, False), (np.ascontiguousarray(a.T), True)):
        m, n = x.shape
        runs = _at_hints("rc_compute_svd_f64", x, [((m, 128), torch.float64), ((128,), torch.float64), ((128, n), torch.float64)])
        (u1, s1, v1, n1, last1), (u8, s8, v8, n8, last8) = runs[1], runs[8]
        print("svd %d x %d: hint 1 %s | hint 8 %s | %s" % (m, n, last1, last8, _splits(n1)))
        assert _splits(n1) == _splits(n8), (_splits(n1), _splits(n8))
        assert np.array_equal(s1, s8) and np.array_equal(u1, u8) and np.array_equal(v1, v8)
        assert len(_gram_labels(n1, 128, 4096)) == 1, n1
        if transposed:
            assert any(t in last1 for t in SPREAD_SHALLOW_TILES), last1
        else:
            assert last1 == last8, (last1, last8)
        assert any(t in last8 for t in PARENT_SHALLOW_TILES), last8
        ref = np.linalg.svd(x, compute_uv=False)
        assert np.abs(s1 - ref).max() <= 1e-12 * ref[0]
        assert rel((u1 * s1) @ v1, x) <= 1e-12
