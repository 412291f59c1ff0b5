"""Batched residual norms of low-rank factors against their blocks (rc_lowrank_residual_batched_*, batch.lowrank_residual_batched and its
three wrappers).

Per block the reference's rel_diff_fro(x.to_mat(), a): err = ||a - left mid diag(s) right||_F at the block's rank, nrm = ||a||_F and the
residual itself.  Checked: err, nrm and e against the host in f64 under the bounds of tests/residual_ref.py (derived from the arithmetic
the C header states, not tuned); the rank contract bit for bit; the exact zeros of a column ID's kept columns; the factors of every
batched compressor; both homes of W; the independence of a block's bits from everything but its operands; containment of non-finite
input; the argument checks."""
import ctypes

import numpy as np
import pytest
import torch

import rusty_compression_amd as rc
from oracle import ref_lapack as o
from rusty_compression_amd import _lib
from tests import residual_ref as rr
from tests.helpers import batched_launch, npy

pytestmark = pytest.mark.gpu

ROW_CHUNK = rr.ROW_CHUNK  # BR_ROWS of kernels_batched_residual.hip
COL_TILE = rr.COL_TILE    # BR_COLS
MAX_LDS = 159 * 1024      # BID_MAX_LDS

DTYPES = [np.float64, np.float32]
MODES = ["none", "mid", "s", "both"]
# (m, n, K): the issue's list with its edge values moved to this kernel's tiling: m one below, at and above the 32-row chunk (31, 32, 33),
# n one below, at and above the 64-column tile (63, 64, 65), K below, at and above the 4-term MFMA step (2, 4, 5) and above a 16-row tile of
# W's image (17); several chunks and tiles with ragged ends (257 x 130, 1030 x 300); the widest n and K (W in the workspace); the tallest m
SHAPES = [(1, 1, 1), (3, 5, 2), (31, 63, 4), (32, 64, 5), (33, 65, 17), (257, 130, 40), (1030, 300, 40), (2048, 96, 16), (40, 512, 128), (65536, 8, 4)]


def tt(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def residual(a, left, right, mid=None, s=None, ranks=None, want_e=True):
    """The call on device tensors (or None); NumPy (err, nrm, e)."""
    out = rc.lowrank_residual_batched(a, left, right, mid=mid, s=s, ranks=ranks, want_residual=want_e)
    torch.cuda.synchronize()
    return tuple(npy(t) for t in out) + (() if want_e else (None,))


def bits(x):
    return np.ascontiguousarray(x).view(np.uint8)


def same_bits(p, q):
    return p.shape == q.shape and np.array_equal(bits(p), bits(q))


def stack(fs):
    """Blocks (dicts of residual_ref.gaussian_factors) as one batch of device tensors: (a, left, right, mid, s)."""
    return tuple(None if fs[0][k] is None else tt(np.stack([f[k] for f in fs])) for k in ("a", "left", "right", "mid", "s"))


def check_block(got, f, r, dtype, tag=""):
    """err, nrm, e of one block against the host under residual_ref.bound; returns the two ratios to the bound."""
    err, nrm, e = got
    m, n = f["a"].shape
    _, e_ref = rr.reference(f["a"], f["left"], f["right"], f["mid"], f["s"], r)
    B, err_bound, nrm_bound = rr.bound(f["a"], f["left"], f["right"], f["mid"], f["s"], r, dtype, rr.chain_length(m, n))
    gap = np.abs(e.astype(np.float64) - e_ref)
    r_e = float(np.max(gap / np.maximum(B, np.finfo(np.float64).tiny)))
    r_err = abs(float(err) - float(np.linalg.norm(e_ref))) / max(err_bound, np.finfo(np.float64).tiny)
    print(f"residual {m}x{n} r={r} {np.dtype(dtype).name} {tag}: max |e - e_ref| / B = {r_e:.3e}, |err - ref| / bound = {r_err:.3e}")
    assert err.dtype == np.dtype(dtype) and nrm.dtype == np.dtype(dtype) and e.dtype == np.dtype(dtype)
    assert np.all(gap <= B)
    assert abs(float(err) - float(np.linalg.norm(e_ref))) <= err_bound
    assert abs(float(nrm) - float(np.linalg.norm(f["a"].astype(np.float64)))) <= nrm_bound
    return r_e, r_err


_DATA = {}


def data(m, n, K, dtype, mode):
    """Two blocks per case, Gaussian factors and factors whose core spans six orders of magnitude (made once)."""
    key = (m, n, K, np.dtype(dtype), mode)
    if key not in _DATA:
        rng = np.random.default_rng(1000 * m + 10 * n + K + MODES.index(mode))
        _DATA[key] = [rr.gaussian_factors(rng, m, n, K, dtype, mode), rr.gaussian_factors(rng, m, n, K, dtype, mode, wide_core=True)]
    return _DATA[key]


# ---------------------------------------------------------------- 1. host parity across shapes and modes
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("m,n,K", SHAPES)
def test_against_the_host(m, n, K, mode, dtype):
    fs = data(m, n, K, dtype, mode)
    a, left, right, mid, s = stack(fs)
    err, nrm, e = residual(a, left, right, mid, s)
    assert err.shape == (2,) and nrm.shape == (2,) and e.shape == (2, m, n)
    for i, f in enumerate(fs):
        check_block((err[i], nrm[i], e[i]), f, K, dtype, f"{mode} K={K} block {i}")


# ---------------------------------------------------------------- 2. ranks
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mode", ["none", "both"])
def test_ranks_truncate_bit_for_bit_and_tails_are_never_read(mode, dtype):
    m, n, K = 33, 65, 17
    f = data(m, n, K, dtype, mode)[0]
    rank_list = [0, 1, 3, 4, 5, K - 1, K, -2, K + 23]
    count = len(rank_list)
    ranks = tt(np.array(rank_list, dtype=np.int64))
    one = {k: tt(f[k]) for k in ("a", "left", "right", "mid", "s")}
    rep = lambda t: None if t is None else t.unsqueeze(0).expand(count, *t.shape)  # noqa: E731  (a batch stride of 0)
    err, nrm, e = residual(rep(one["a"]), rep(one["left"]), rep(one["right"]), rep(one["mid"]), rep(one["s"]), ranks)
    # tails filled with NaN, per block at its own rank
    nan = {k: None if f[k] is None else np.stack([f[k]] * count) for k in ("left", "right", "mid", "s")}
    for i, rv in enumerate(rank_list):
        r = min(max(rv, 0), K)
        nan["left"][i][:, r:] = np.nan
        nan["right"][i][r:] = np.nan
        if nan["mid"] is not None:
            nan["mid"][i][r:, :] = np.nan
            nan["mid"][i][:, r:] = np.nan
        if nan["s"] is not None:
            nan["s"][i][r:] = np.nan
    err2, nrm2, e2 = residual(rep(one["a"]), tt(nan["left"]), tt(nan["right"]), tt(nan["mid"]), tt(nan["s"]), ranks)
    assert same_bits(err, err2) and same_bits(nrm, nrm2) and same_bits(e, e2)
    for i, rv in enumerate(rank_list):
        r = min(max(rv, 0), K)
        assert same_bits(nrm[i], nrm[0])
        if r == 0:
            assert same_bits(err[i], nrm[i]) and same_bits(e[i], f["a"])
            continue
        cut = lambda t, rows, cols: None if t is None else t[rows, cols].unsqueeze(0)  # noqa: E731  (strided views of inner width r)
        sl = slice(0, r)
        te, tn, tr = residual(one["a"].unsqueeze(0), cut(one["left"], slice(None), sl), cut(one["right"], sl, slice(None)), cut(one["mid"], sl, sl),
                              None if one["s"] is None else one["s"][:r].unsqueeze(0))
        assert same_bits(err[i], te[0]) and same_bits(nrm[i], tn[0]) and same_bits(e[i], tr[0]), (mode, rv)
        check_block((err[i], nrm[i], e[i]), f, r, dtype, f"{mode} rank {rv}")


# ---------------------------------------------------------------- 3. exact zeros of the column IDs
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("route", ["column_id", "sketch"])
def test_kept_columns_of_a_column_id_leave_exact_zeros(route, dtype):
    tol = 1e-8 if dtype == np.float64 else 1e-4
    rng = np.random.default_rng(31)
    if route == "column_id":
        m, n, k = 70, 66, 12
        a = np.stack([o.random_approximate_low_rank_matrix((m, n), 1.0, 10.0 ** -(6 + 4 * i), rng).astype(dtype) for i in range(3)])
        c, z, ind, ranks = rc.column_id_rank_batched(tt(a), k, tol)
    else:
        m, n, l, k = 2048, 96, 24, 16
        a = np.stack([o.random_approximate_low_rank_matrix((m, n), 1.0, 10.0 ** -(10 + 20 * i), rng).astype(dtype) for i in range(2)])
        c, z, ind, ranks = rc.sketch_column_id_rank_batched(tt(a), k, tol, omega=tt(rng.standard_normal((l, m)).astype(dtype)))
    err, nrm, e = (npy(t) for t in rc.column_id_residual_batched(tt(a), c, z, ranks, want_residual=True))
    c, z, ind, ranks = npy(c), npy(z), npy(ind), npy(ranks)
    for i in range(a.shape[0]):
        r = int(ranks[i])
        assert 1 <= r <= k
        assert not np.any(e[i][:, ind[i][:r]])  # +0.0 or -0.0, nothing else
        f = {"a": a[i], "left": c[i], "right": z[i], "mid": None, "s": None}
        check_block((err[i], nrm[i], e[i]), f, r, dtype, f"{route} block {i}")


# ---------------------------------------------------------------- 4. factors of every compressor
@pytest.mark.parametrize("dtype", DTYPES)
def test_factors_of_every_batched_compressor(dtype):
    tol = 1e-6 if dtype == np.float64 else 1e-3
    m, n, k = 48, 40, 24
    rng = np.random.default_rng(41)
    a = np.stack([o.random_approximate_low_rank_matrix((m, n), 1.0, 10.0 ** -(4 + 3 * i), rng).astype(dtype) for i in range(5)])
    ad = tt(a)
    c, x, r, _, _, ranks = rc.two_sided_id_rank_batched(ad, k, tol)
    got_ts = tuple(npy(t) for t in rc.two_sided_id_residual_batched(ad, c, x, r, ranks, want_residual=True))
    u, s, vt, sranks = rc.svd_rank_batched(ad, k, tol)
    got_svd = tuple(npy(t) for t in rc.svd_residual_batched(ad, u, s, vt, sranks, want_residual=True))
    cc, cz, _, cranks = rc.column_id_rank_batched(ad, k, tol)
    ru, rs, rvt, rranks = rc.column_id_to_svd_batched(cc, cz, cranks, k, tol)
    got_rc = tuple(npy(t) for t in rc.svd_residual_batched(ad, ru, rs, rvt, rranks, want_residual=True))
    assert len(set(npy(ranks).tolist())) > 1 and len(set(npy(sranks).tolist())) > 1  # the ranks differ over the batch
    for i in range(a.shape[0]):
        f = {"a": a[i], "left": npy(c)[i], "right": npy(r)[i], "mid": npy(x)[i], "s": None}
        check_block(tuple(g[i] for g in got_ts), f, int(npy(ranks)[i]), dtype, f"two-sided block {i}")
        rk = int(npy(sranks)[i])
        f = {"a": a[i], "left": npy(u)[i], "right": npy(vt)[i], "mid": None, "s": npy(s)[i]}
        check_block(tuple(g[i] for g in got_svd), f, rk, dtype, f"svd block {i}")
        # err against the discarded singular values.  err_bound covers the rounding of the rebuild alone; the factors carry the batched
        # SVD's own backward error, a few u ||a||_F, which ||B||_F = c (2 r + 4) u || |a| + |u| |s| |vt| ||_F >= 2 (2 r + 4) u ||a||_F
        # covers with r >= 8 here only as long as that error stays below about 40 u ||a||_F: the check passes by that margin, not by a
        # derivation of the SVD's error
        sv = np.linalg.svd(a[i].astype(np.float64), compute_uv=False)
        _, err_bound, _ = rr.bound(f["a"], f["left"], f["right"], None, f["s"], rk, dtype, rr.chain_length(m, n))
        tail = float(np.sqrt(np.sum(sv[rk:] ** 2)))
        print(f"svd block {i} {np.dtype(dtype).name}: err {float(got_svd[0][i]):.6e} tail {tail:.6e} bound {err_bound:.3e}")
        assert abs(float(got_svd[0][i]) - tail) <= err_bound
        f = {"a": a[i], "left": npy(ru)[i], "right": npy(rvt)[i], "mid": None, "s": npy(rs)[i]}
        check_block(tuple(g[i] for g in got_rc), f, int(npy(rranks)[i]), dtype, f"recompressed block {i}")


# ---------------------------------------------------------------- 5. both homes of W
def lds_bytes(K, n, elem, has_mid, w_lds):
    """br_lds_bytes of kernels_batched_residual.hip: red[8] | [W0 [W1]: K4 x (np + 16)] a's tile image | left's chunk image."""
    k4, npad = (K + 3) // 4 * 4, (n + COL_TILE - 1) // COL_TILE * COL_TILE
    a_el = max(ROW_CHUNK * (80 if elem == 8 else 68), COL_TILE * (ROW_CHUNK + 4))
    l_el = max(ROW_CHUNK * ((K + 31) // 32 * 32 + 4), k4 * (ROW_CHUNK + 16))
    return 64 + ((2 if has_mid else 1) * k4 * (npad + 16) * (1 if w_lds else 0) + a_el + l_el) * elem


@pytest.mark.parametrize("dtype", DTYPES)
def test_both_plans_of_w_give_the_same_bits(dtype):
    elem = np.dtype(dtype).itemsize
    m, K = 70, 64
    n_fit = max(n for n in range(1, 513) if lds_bytes(K, n, elem, True, True) <= MAX_LDS)  # the widest block whose W stays in LDS
    assert COL_TILE <= n_fit < 512 and n_fit % COL_TILE == 0
    n_ws = n_fit + 1
    fs = data(m, n_fit, K, dtype, "both")
    a, left, right, mid, s = stack(fs)
    got, lab = batched_launch(lambda: residual(a, left, right, mid, s))
    assert lab["op"] == "batched_residual" and (lab["m"], lab["n"], lab["k"], lab["count"]) == (m, n_fit, K, 2)
    assert lab["plan"].startswith("W:lds,") and lab["plan"].endswith(",mid,s,e,nrm")
    for i, f in enumerate(fs):
        check_block(tuple(g[i] for g in got), f, K, dtype, f"W:lds block {i}")
    # the same blocks one column wider, the extra column of a and of right zero: its residual is +0 and adds nothing to either sum
    wide = lambda t: torch.cat([t, torch.zeros_like(t[:, :, :1])], dim=2)  # noqa: E731
    got_w, lab = batched_launch(lambda: residual(wide(a), left, wide(right), mid, s))
    assert (lab["n"], lab["count"]) == (n_ws, 2) and lab["plan"].startswith("W:ws,")
    assert same_bits(got_w[0], got[0]) and same_bits(got_w[1], got[1])
    assert same_bits(got_w[2][:, :, :n_fit], got[2]) and not np.any(got_w[2][:, :, n_fit:])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m,n,K,plan", [(70, 130, 24, "lds"), (40, 512, 128, "ws")])
def test_right_read_in_place_gives_the_bits_of_an_image(m, n, K, plan, dtype):
    """Without mid and s there is no image of W: the MFMA reads right in place (plan W:right).  With s = 1 the image holds right's
    values exactly, in LDS or in the workspace, so the two calls must agree bit for bit."""
    fs = data(m, n, K, dtype, "none")
    a, left, right, _, _ = stack(fs)
    ranks = tt(np.array([K, max(K - 3, 0)], dtype=np.int64))
    got, lab = batched_launch(lambda: residual(a, left, right, ranks=ranks))
    assert lab["plan"].startswith("W:right,") and lab["plan"].endswith(",e,nrm")
    ones = torch.ones((2, K), dtype=a.dtype, device="cuda")
    img, lab = batched_launch(lambda: residual(a, left, right, s=ones, ranks=ranks))
    assert lab["plan"].startswith(f"W:{plan},") and lab["plan"].endswith(",s,e,nrm")
    assert all(same_bits(p, q) for p, q in zip(got, img))


# ---------------------------------------------------------------- 6. bit independence
def raw(dtype, a, left, right, mid=None, s=None, ranks=None, e=None, err=None, nrm=None, count=None, ctx=None, e_bs=None, null=None):
    """One raw call on 3-D device views (None: absent; null: the name of an operand passed with its shape and a null pointer); returns the status."""
    ctx = ctx or _lib.default_context()
    fn = getattr(_lib.lib(), f"rc_lowrank_residual_batched_{_lib.suffix(dtype)}")

    def view(t):
        if t is None:
            return _lib.mat(None), ctypes.c_int64(0)
        return _lib.rc_matrix(t.data_ptr(), t.shape[1], t.shape[2], t.stride(1), t.stride(2)), ctypes.c_int64(t.stride(0))

    ptr = lambda t: ctypes.c_void_p(None if t is None else t.data_ptr())  # noqa: E731
    ev = list(view(e))
    if e_bs is not None:
        ev[1] = ctypes.c_int64(e_bs)
    views = {"a": view(a), "left": view(left), "right": view(right)}
    if null:
        views[null][0].data = None
    return fn(ctx._h, *views["a"], *views["left"], *view(mid), ptr(s), ctypes.c_int64(0 if s is None else s.stride(0)), *views["right"], ptr(ranks),
              ctypes.c_int32(a.shape[0] if count is None else count), *ev, ptr(err), ptr(nrm))


def test_a_block_does_not_see_its_batch():
    """Tiny blocks, more of them than the grid has workgroups, so that one workgroup handles several: the block at the first, a middle
    and the last position gives the bits of the call on it alone, whatever its neighbours are."""
    m, n, K = 5, 6, 3
    dtype = np.float64
    rng = np.random.default_rng(61)
    probe = [rr.gaussian_factors(rng, m, n, K, dtype, "both") for _ in range(2)]
    _, lab = batched_launch(lambda: residual(*stack(probe * 4096)))
    slots = lab["slots"]
    assert lab["grid"] == min(slots, 8192)
    count = 2 * slots + 3
    target = rr.gaussian_factors(rng, m, n, K, dtype, "both")
    alone = residual(*stack([target]))
    check_block(tuple(g[0] for g in alone), target, K, dtype, "alone")
    for seed in (1, 2):  # different neighbours
        nrng = np.random.default_rng(seed)
        keys = ("a", "left", "right", "mid", "s")
        big = {k: nrng.standard_normal((count,) + target[k].shape) for k in keys}
        pos = (0, count // 2 + 1, count - 1)
        for p in pos:
            for k in keys:
                big[k][p] = target[k]
        got, lab = batched_launch(lambda: residual(*(tt(big[k]) for k in keys)))
        assert lab["count"] == count and lab["grid"] == slots < count
        for p in pos:
            assert all(same_bits(g[p], al[0]) for g, al in zip(got, alone)), (seed, p)


@pytest.mark.parametrize("dtype", DTYPES)
def test_views_strides_and_optional_outputs_do_not_change_the_bits(dtype):
    m, n, K = 45, 70, 9
    tdt = torch.float64 if dtype == np.float64 else torch.float32
    fs = data(m, n, K, dtype, "both")
    a, left, right, mid, s = stack(fs)
    base = residual(a, left, right, mid, s)
    # transposed storage of every operand (the lanes of the staging loops then run along the other index)
    tr = lambda t: t.transpose(1, 2).contiguous().transpose(1, 2)  # noqa: E731
    assert all(same_bits(p, q) for p, q in zip(residual(tr(a), tr(left), tr(right), tr(mid), s), base))
    # padded views: every operand a window of a larger NaN-filled array
    def padded(t):
        big = torch.full((t.shape[0] + 1, t.shape[1] + 3, t.shape[2] + 5), float("nan"), dtype=t.dtype, device="cuda")
        big[1:, 2:2 + t.shape[1], 4:4 + t.shape[2]] = t
        return big[1:, 2:2 + t.shape[1], 4:4 + t.shape[2]]
    sp = torch.full((2, K + 7), float("nan"), dtype=tdt, device="cuda")
    sp[:, :K] = s
    assert all(same_bits(p, q) for p, q in zip(residual(padded(a), padded(left), padded(right), padded(mid), sp), base))
    # a strided e, row-major and column-major, whose gaps stay untouched; with and without e and nrm
    for colmajor in (False, True):
        buf = torch.full((2, n + 3, m + 2) if colmajor else (2, m + 2, n + 3), -7.0, dtype=tdt, device="cuda")
        e = buf.transpose(1, 2)[:, 1:1 + m, 2:2 + n] if colmajor else buf[:, 1:1 + m, 2:2 + n]
        err = torch.zeros(2, dtype=tdt, device="cuda")
        nrm = torch.zeros(2, dtype=tdt, device="cuda")
        assert raw(tdt, a, left, right, mid, s, e=e, err=err, nrm=nrm) == 0
        torch.cuda.synchronize()
        assert same_bits(npy(err), base[0]) and same_bits(npy(nrm), base[1]) and same_bits(npy(e), base[2])
        mask = torch.ones_like(buf, dtype=torch.bool)
        (mask.transpose(1, 2) if colmajor else mask)[:, 1:1 + m, 2:2 + n] = False
        assert bool(torch.all(buf[mask] == -7.0))
    err = torch.zeros(2, dtype=tdt, device="cuda")
    assert raw(tdt, a, left, right, mid, s, err=err) == 0  # neither e nor nrm
    torch.cuda.synchronize()
    assert same_bits(npy(err), base[0])
    # a batch stride of 0 on a and on the factors: every block is block 0
    rep = lambda t: t[:1].expand(3, *t.shape[1:])  # noqa: E731
    got = residual(rep(a), rep(left), rep(right), rep(mid), rep(s))
    for i in range(3):
        assert all(same_bits(g[i], b[0]) for g, b in zip(got, base))


def test_graph_capture_replays_the_eager_bits():
    m, n, K, count = 96, 130, 24, 33
    rng = np.random.default_rng(8)
    fs = [rr.gaussian_factors(rng, m, n, K, np.float64, "both") for _ in range(count)]
    lib = _lib.lib()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        a, left, right, mid, s = stack(fs)
        ranks = tt((np.arange(count) % (K + 3) - 1).astype(np.int64))
        eager = residual(a, left, right, mid, s, ranks)
        ctx = _lib.Context(torch.cuda.current_device(), st.cuda_stream)
        e = torch.zeros((count, m, n), dtype=torch.float64, device="cuda")
        err = torch.zeros(count, dtype=torch.float64, device="cuda")
        nrm = torch.zeros(count, dtype=torch.float64, device="cuda")
        st.synchronize()
        graph = ctypes.c_void_p(None)
        ctx.check(lib.rc_graph_begin_capture(ctx._h))
        assert raw(torch.float64, a, left, right, mid, s, ranks, e, err, nrm, ctx=ctx) == 0
        ctx.check(lib.rc_graph_end_capture(ctx._h, ctypes.byref(graph)))
        try:
            st.synchronize()
            assert not np.any(npy(e)) and not np.any(npy(err))  # captured, not run
            ctx.check(lib.rc_graph_launch(ctx._h, graph))
            ctx.synchronize()
            assert same_bits(npy(err), eager[0]) and same_bits(npy(nrm), eager[1]) and same_bits(npy(e), eager[2])
        finally:
            ctx.check(lib.rc_graph_destroy(ctx._h, graph))
            ctx.close()


# ---------------------------------------------------------------- 7. non-finite input stays in its block
@pytest.mark.parametrize("dtype", DTYPES)
def test_non_finite_input_stays_in_its_block(dtype):
    m, n, K = 40, 70, 6
    rng = np.random.default_rng(71)
    fs = [rr.gaussian_factors(rng, m, n, K, dtype, "both") for _ in range(5)]
    clean = residual(*stack(fs))
    fs[1]["a"][3, 4] = np.nan
    fs[3]["left"][0, 0] = np.inf
    fs[3]["s"][2] = np.nan
    got = residual(*stack(fs))
    for i in (0, 2, 4):
        assert all(same_bits(g[i], c[i]) for g, c in zip(got, clean))
    assert np.isnan(got[0][1]) and np.isnan(got[1][1]) and np.isnan(got[2][1][3, 4]) and np.sum(np.isnan(got[2][1])) == 1
    assert not np.isfinite(got[0][3]) and same_bits(got[1][3], clean[1][3])


# ---------------------------------------------------------------- 8. arguments
def test_arguments():
    dt = torch.float64
    z = lambda *shape: torch.zeros(shape, dtype=dt, device="cuda")  # noqa: E731
    bad = _lib.RC_INVALID_ARGUMENT
    m, n, K, count = 6, 7, 3, 2
    a, left, right, mid, s = z(count, m, n), z(count, m, K), z(count, K, n), z(count, K, K), z(count, K)
    err, nrm, e = z(count), z(count), z(count, m, n)
    assert raw(dt, a, left, right, mid, s, None, e, err, nrm) == 0
    # count = 0 is a no-op, null pointers included
    err.fill_(5.0)
    assert raw(dt, a, left, right, err=None, count=0) == 0
    got = rc.lowrank_residual_batched(z(0, m, n), z(0, m, K), z(0, K, n), want_residual=True)
    assert got[0].shape == (0,) and got[1].shape == (0,) and got[2].shape == (0, m, n)
    torch.cuda.synchronize()
    assert bool(torch.all(err == 5.0))
    assert raw(dt, a, left, right, err=err, count=-1) == bad
    # the domain: one past m, n and K (the views are never dereferenced: the checks come first)
    assert raw(dt, z(1, 1, n).expand(1, 65537, n), z(1, 1, K).expand(1, 65537, K), right[:1], err=err) == bad
    assert raw(dt, z(1, m, 1).expand(1, m, 513), left[:1], z(1, K, 1).expand(1, K, 513), err=err) == bad
    assert raw(dt, a[:1], z(1, m, 1).expand(1, m, 129), z(1, 1, n).expand(1, 129, n), err=err) == bad
    assert raw(dt, z(1, 1, n).expand(1, 65536, n), z(1, 1, K).expand(1, 65536, K), right[:1], err=err) == 0  # the largest m is inside
    # every shape mismatch
    assert raw(dt, a, z(count, m + 1, K), right, err=err) == bad       # left.rows != a.rows
    assert raw(dt, a, left, z(count, K + 1, n), err=err) == bad        # left.cols != right.rows
    assert raw(dt, a, left, z(count, K, n + 1), err=err) == bad        # right.cols != a.cols
    assert raw(dt, a, left, right, z(count, K, K + 1), err=err) == bad  # mid not K x K
    assert raw(dt, a, left, right, z(count, K + 1, K), err=err) == bad
    assert raw(dt, a, left, right, e=z(count, m, n + 1), err=err) == bad  # e not m x n
    assert raw(dt, a, left, right, e=z(count, m + 1, n), err=err) == bad
    # an e batch stride smaller than one view's span: only with more than one block
    assert raw(dt, a, left, right, e=e, err=err, e_bs=m * n - 1) == bad
    assert raw(dt, a[:1], left[:1], right[:1], e=e[:1], err=err, e_bs=0) == 0
    # null pointers
    for which in ("a", "left", "right"):
        assert raw(dt, a, left, right, err=err, null=which) == bad, which
    assert raw(dt, a, left, right, err=None) == bad
    torch.cuda.synchronize()
    # Python: wrong dtypes raise TypeError, the library's INVALID_ARGUMENT an AssertionError
    with pytest.raises(TypeError):
        rc.lowrank_residual_batched(a.to(torch.complex128), left.to(torch.complex128), right.to(torch.complex128))
    with pytest.raises(TypeError):
        rc.lowrank_residual_batched(a, left.float(), right)
    with pytest.raises(TypeError):
        rc.lowrank_residual_batched(a, left, right, s=s.float())
    with pytest.raises(TypeError):
        rc.lowrank_residual_batched(a, left, right, ranks=torch.zeros(count, dtype=torch.int32, device="cuda"))
    with pytest.raises(AssertionError, match="lowrank_residual_batched"):
        rc.lowrank_residual_batched(z(1, m, 513), left[:1], z(1, K, 513))
