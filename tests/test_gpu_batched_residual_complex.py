"""Batched residual norms of complex low-rank factors against their blocks (rc_lowrank_residual_batched_c64 / _c32,
batch.lowrank_residual_batched_complex and its three wrappers).

Per block err = ||a - left mid diag(s) right||_F at the block's rank (nothing conjugated), nrm = ||a||_F and the residual itself.  Checked:
err, nrm and e against the host in complex128 under the bounds of tests/residual_ref_complex.py (derived from the arithmetic the C header
states, not tuned); the rank contract bit for bit; the exact zeros of a column ID's kept columns; the factors of every complex batched
compressor; the conjugate symmetry and the real embedding the header promises; both homes of W and W read in place; the independence of a
block's bits from everything but its operands; containment of non-finite input; the argument checks."""
import ctypes

import numpy as np
import pytest
import torch

import rusty_compression_amd as rc
from oracle import ref_lapack as o
from rusty_compression_amd import _lib
from tests import residual_ref_complex as rrc
from tests.helpers import batched_launch, npy

pytestmark = pytest.mark.gpu

ROW_CHUNK = rrc.ROW_CHUNK  # BRC_ROWS of kernels_batched_residual_c.hip
COL_TILE = rrc.COL_TILE    # BRC_COLS
MAX_LDS = 159 * 1024       # BID_MAX_LDS

DTYPES = [np.complex128, np.complex64]
MODES = ["none", "mid", "s", "both"]
# (m, n, K) at the edges of this kernel's tiling: m one below, at and above the 32-row chunk (31, 32, 33), n one below, at and above the
# 64-column tile (63, 64, 65), K below, at and above the 4-term MFMA step (2, 4, 5) and above a 16-row tile of W's image (17); several
# chunks and tiles with ragged ends (257 x 130, 1030 x 300); the widest n and K (W in the workspace); the tallest m
SHAPES = [(1, 1, 1), (3, 5, 2), (31, 63, 4), (32, 64, 5), (33, 65, 17), (257, 130, 40), (1030, 300, 40), (40, 512, 128), (65536, 8, 4)]
KEYS = ("a", "left", "right", "mid", "s")


def tt(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def residual(a, left, right, mid=None, s=None, ranks=None, want_e=True):
    """The call on device tensors (or None); NumPy (err, nrm, e)."""
    out = rc.lowrank_residual_batched_complex(a, left, right, mid=mid, s=s, ranks=ranks, want_residual=want_e)
    torch.cuda.synchronize()
    return tuple(npy(t) for t in out) + (() if want_e else (None,))


def bits(x):
    return np.ascontiguousarray(x).view(np.uint8)


def same_bits(p, q):
    return p.shape == q.shape and p.dtype == q.dtype and np.array_equal(bits(p), bits(q))


def stack(fs):
    """Blocks (dicts of residual_ref_complex.gaussian_factors) as one batch of device tensors: (a, left, right, mid, s)."""
    return tuple(None if fs[0][k] is None else tt(np.stack([f[k] for f in fs])) for k in KEYS)


def check_block(got, f, r, dtype, tag=""):
    """err, nrm, e of one block against the host under residual_ref_complex.bound; returns the two ratios to the bound."""
    err, nrm, e = got
    m, n = f["a"].shape
    real = rrc.real_dtype(dtype)
    _, e_ref = rrc.reference(f["a"], f["left"], f["right"], f["mid"], f["s"], r)
    B, err_bound, nrm_bound = rrc.bound(f["a"], f["left"], f["right"], f["mid"], f["s"], r, dtype, rrc.chain_length(m, n))
    gap = np.abs(e.astype(np.complex128) - e_ref)
    r_e = float(np.max(gap / np.maximum(B, np.finfo(np.float64).tiny)))
    r_err = abs(float(err) - float(np.linalg.norm(e_ref))) / max(err_bound, np.finfo(np.float64).tiny)
    print(f"residual<complex> {m}x{n} r={r} {np.dtype(dtype).name} {tag}: max |e - e_ref| / B = {r_e:.3e}, |err - ref| / bound = {r_err:.3e}")
    assert err.dtype == real and nrm.dtype == real and e.dtype == np.dtype(dtype)
    assert np.all(gap <= B)
    assert abs(float(err) - float(np.linalg.norm(e_ref))) <= err_bound
    assert abs(float(nrm) - float(np.linalg.norm(f["a"].astype(np.complex128)))) <= nrm_bound
    return r_e, r_err


_DATA = {}


def data(m, n, K, dtype, mode):
    """Two blocks per case, Gaussian factors and factors whose core spans six orders of magnitude (made once)."""
    key = (m, n, K, np.dtype(dtype), mode)
    if key not in _DATA:
        rng = np.random.default_rng(1000 * m + 10 * n + K + MODES.index(mode))
        _DATA[key] = [rrc.gaussian_factors(rng, m, n, K, dtype, mode), rrc.gaussian_factors(rng, m, n, K, dtype, mode, wide_core=True)]
    return _DATA[key]


def decaying_blocks(m, n, sigma_mins, dtype, rng):
    """Complex blocks whose singular values fall geometrically from 1 to sigma_min."""
    return np.stack([o.random_approximate_low_rank_matrix((m, n), 1.0, sm, rng, dtype=np.complex128).astype(dtype) for sm in sigma_mins])


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
    one = {k: tt(f[k]) for k in KEYS}
    rep = lambda t: None if t is None else t.unsqueeze(0).expand(count, *t.shape)  # noqa: E731  (a batch stride of 0)
    err, nrm, e = residual(rep(one["a"]), rep(one["left"]), rep(one["right"]), rep(one["mid"]), rep(one["s"]), ranks)
    # tails filled with NaN (both components), per block at its own rank
    nan = {k: None if f[k] is None else np.stack([f[k]] * count) for k in ("left", "right", "mid", "s")}
    cnan = complex(np.nan, np.nan)
    for i, rv in enumerate(rank_list):
        r = min(max(rv, 0), K)
        nan["left"][i][:, r:] = cnan
        nan["right"][i][r:] = cnan
        if nan["mid"] is not None:
            nan["mid"][i][r:, :] = cnan
            nan["mid"][i][:, r:] = cnan
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


# ---------------------------------------------------------------- 3. exact zeros of the column ID
@pytest.mark.parametrize("dtype", DTYPES)
def test_kept_columns_of_a_column_id_leave_exact_zeros(dtype):
    tol = 1e-8 if dtype == np.complex128 else 1e-4
    m, n, k = 70, 66, 12
    a = decaying_blocks(m, n, [10.0 ** -(6 + 4 * i) for i in range(3)], dtype, np.random.default_rng(31))
    c, z, ind, ranks = rc.column_id_rank_batched(tt(a), k, tol)
    err, nrm, e = (npy(t) for t in rc.column_id_residual_batched_complex(tt(a), c, z, ranks, want_residual=True))
    c, z, ind, ranks = npy(c), npy(z), npy(ind), npy(ranks)
    for i in range(a.shape[0]):
        r = int(ranks[i])
        assert 1 <= r <= k
        kept = e[i][:, ind[i][:r]]
        assert not np.any(kept.real) and not np.any(kept.imag)  # +0.0 or -0.0 in both components, nothing else
        f = {"a": a[i], "left": c[i], "right": z[i], "mid": None, "s": None}
        check_block((err[i], nrm[i], e[i]), f, r, dtype, f"column ID block {i}")


# ---------------------------------------------------------------- 4. factors of every complex compressor
@pytest.mark.parametrize("dtype", DTYPES)
def test_factors_of_every_complex_batched_compressor(dtype):
    tol = 1e-8 if dtype == np.complex128 else 1e-4
    m, n, k = 48, 40, 24
    a = decaying_blocks(m, n, [tol ** (1 + 0.5 * i) for i in range(5)], dtype, np.random.default_rng(41))
    ad = tt(a)
    cc, cz, _, cranks = rc.column_id_rank_batched(ad, k, tol)
    got_id = tuple(npy(t) for t in rc.column_id_residual_batched_complex(ad, cc, cz, cranks, want_residual=True))
    c, x, r, _, _, ranks = rc.two_sided_id_rank_batched(ad, k, tol)
    got_ts = tuple(npy(t) for t in rc.two_sided_id_residual_batched_complex(ad, c, x, r, ranks, want_residual=True))
    u, s, vt, sranks = rc.svd_rank_batched_complex(ad, k, tol)
    got_svd = tuple(npy(t) for t in rc.svd_residual_batched_complex(ad, u, s, vt, sranks, want_residual=True))
    assert len(set(npy(ranks).tolist())) > 1 and len(set(npy(sranks).tolist())) > 1  # the ranks differ over the batch
    for i in range(a.shape[0]):
        f = {"a": a[i], "left": npy(cc)[i], "right": npy(cz)[i], "mid": None, "s": None}
        check_block(tuple(g[i] for g in got_id), f, int(npy(cranks)[i]), dtype, f"column ID block {i}")
        f = {"a": a[i], "left": npy(c)[i], "right": npy(r)[i], "mid": npy(x)[i], "s": None}
        check_block(tuple(g[i] for g in got_ts), f, int(npy(ranks)[i]), dtype, f"two-sided block {i}")
        f = {"a": a[i], "left": npy(u)[i], "right": npy(vt)[i], "mid": None, "s": npy(s)[i]}
        check_block(tuple(g[i] for g in got_svd), f, int(npy(sranks)[i]), dtype, f"svd block {i}")


# ---------------------------------------------------------------- 5. conjugate symmetry
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mode", ["none", "both"])
def test_conjugating_every_operand_conjugates_the_residual(mode, dtype):
    m, n, K = 45, 70, 9
    fs = data(m, n, K, dtype, mode)
    a, left, right, mid, s = stack(fs)
    err, nrm, e = residual(a, left, right, mid, s)
    cj = lambda t: None if t is None else t.conj_physical()  # noqa: E731  (stored conjugates, not lazy views)
    cerr, cnrm, ce = residual(cj(a), cj(left), cj(right), cj(mid), s)
    assert same_bits(cerr, err) and same_bits(cnrm, nrm)
    assert same_bits(ce.real, e.real)
    # Im e is negated bit for bit wherever it is not zero; an Im e that cancelled to zero exactly is +0 in both runs (x - x = +0 in IEEE
    # arithmetic whatever the sign of x), which happens in complex64 at about one element in 10^4 of these blocks
    zero = e.imag == 0
    print(f"conjugate {mode} {np.dtype(dtype).name}: {int(np.count_nonzero(zero))} of {zero.size} Im e are exact zeros")
    assert np.array_equal(ce.imag == 0, zero) and np.count_nonzero(zero) <= zero.size // 100
    assert same_bits(ce.imag[~zero], -e.imag[~zero])


# ---------------------------------------------------------------- 6. real embedding
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mode", ["none", "both"])
def test_operands_with_zero_imaginary_parts_give_the_real_call(mode, dtype):
    m, n, K = 45, 70, 9
    fs = data(m, n, K, dtype, mode)
    re = {k: None if fs[0][k] is None else np.stack([np.ascontiguousarray(f[k].real) for f in fs]) for k in KEYS}
    want = rc.lowrank_residual_batched(tt(re["a"]), tt(re["left"]), tt(re["right"]), mid=tt(re["mid"]), s=tt(re["s"]), want_residual=True)
    emb = {k: None if re[k] is None else (re[k] if k == "s" else re[k].astype(dtype)) for k in KEYS}  # imaginary parts +0
    err, nrm, e = residual(*(tt(emb[k]) for k in KEYS))
    assert np.array_equal(e.real, npy(want[2])) and not np.any(e.imag)
    assert np.array_equal(err, npy(want[0])) and np.array_equal(nrm, npy(want[1]))  # the squares of the zeros add nothing


# ---------------------------------------------------------------- 7. both homes of W, W read in place
def lds_bytes(K, n, real_bytes, has_mid, w_lds):
    """brc_lds_bytes of kernels_batched_residual_c.hip: red[8] | [W0 [W1]: K4 x (np + 16)] a's tile image | left's chunk image, in complex
    elements of 2 * real_bytes."""
    k4, npad = (K + 3) // 4 * 4, (n + COL_TILE - 1) // COL_TILE * COL_TILE
    a_el = max(ROW_CHUNK * (80 if real_bytes == 8 else 68), COL_TILE * (ROW_CHUNK + 2))
    l_el = max(ROW_CHUNK * ((K + 31) // 32 * 32 + 2), k4 * (ROW_CHUNK if real_bytes == 8 else ROW_CHUNK + 16))
    return 64 + ((2 if has_mid else 1) * k4 * (npad + 16) * (1 if w_lds else 0) + a_el + l_el) * 2 * real_bytes


def plan_of(K, n, real_bytes, has_mid, has_s):
    if not has_mid and not has_s:
        return "right"
    return "lds" if lds_bytes(K, n, real_bytes, has_mid, True) <= MAX_LDS else "ws"


@pytest.mark.parametrize("dtype", DTYPES)
def test_both_plans_of_w_give_the_same_bits(dtype):
    rb = rrc.real_dtype(dtype).itemsize
    m, K = 70, (16 if rb == 8 else 64)
    n_fit = max(n for n in range(1, 513) if lds_bytes(K, n, rb, True, True) <= MAX_LDS)  # the widest block whose W stays in LDS
    assert COL_TILE <= n_fit < 512 and n_fit % COL_TILE == 0
    n_ws = n_fit + 1
    fs = data(m, n_fit, K, dtype, "both")
    a, left, right, mid, s = stack(fs)
    got, lab = batched_launch(lambda: residual(a, left, right, mid, s))
    assert lab["op"] == "batched_residual<complex>" and (lab["m"], lab["n"], lab["k"], lab["count"]) == (m, n_fit, K, 2)
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
@pytest.mark.parametrize("m,n,K", [(70, 130, 24), (40, 512, 128)])
def test_right_read_in_place_gives_the_bits_of_an_image(m, n, K, dtype):
    """Without mid and s there is no image of W: the MFMA reads right in place (plan W:right).  With s = 1 the image holds right's
    values exactly, in LDS or in the workspace, so the two calls must agree bit for bit."""
    rb = rrc.real_dtype(dtype).itemsize
    fs = data(m, n, K, dtype, "none")
    a, left, right, _, _ = stack(fs)
    ranks = tt(np.array([K, max(K - 3, 0)], dtype=np.int64))
    got, lab = batched_launch(lambda: residual(a, left, right, ranks=ranks))
    assert lab["plan"].startswith("W:right,") and lab["plan"].endswith(",e,nrm")
    ones = torch.ones((2, K), dtype=torch.float64 if rb == 8 else torch.float32, device="cuda")
    img, lab = batched_launch(lambda: residual(a, left, right, s=ones, ranks=ranks))
    assert lab["plan"].startswith(f"W:{plan_of(K, n, rb, False, True)},") and lab["plan"].endswith(",s,e,nrm")
    if (m, n, K) == (40, 512, 128):
        assert plan_of(K, n, rb, False, True) == "ws"  # the widest n and K: no image of that size fits LDS in either precision
    assert all(same_bits(p, q) for p, q in zip(got, img))


# ---------------------------------------------------------------- 8. bit independence
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
    dtype = np.complex128
    rng = np.random.default_rng(61)
    probe = [rrc.gaussian_factors(rng, m, n, K, dtype, "both") for _ in range(2)]
    _, lab = batched_launch(lambda: residual(*stack(probe * 4096)))
    slots = lab["slots"]
    assert lab["grid"] == min(slots, 8192)
    count = 2 * slots + 3
    target = rrc.gaussian_factors(rng, m, n, K, dtype, "both")
    alone = residual(*stack([target]))
    check_block(tuple(g[0] for g in alone), target, K, dtype, "alone")
    for seed in (1, 2):  # different neighbours
        nrng = np.random.default_rng(seed)
        big = {k: nrng.standard_normal((count,) + target[k].shape).astype(target[k].dtype) for k in KEYS}
        pos = (0, count // 2 + 1, count - 1)
        for p in pos:
            for k in KEYS:
                big[k][p] = target[k]
        got, lab = batched_launch(lambda: residual(*(tt(big[k]) for k in KEYS)))
        assert lab["count"] == count and lab["grid"] == slots < count
        for p in pos:
            assert all(same_bits(g[p], al[0]) for g, al in zip(got, alone)), (seed, p)


@pytest.mark.parametrize("dtype", DTYPES)
def test_views_strides_and_optional_outputs_do_not_change_the_bits(dtype):
    m, n, K = 45, 70, 9
    tdt = torch.complex128 if dtype == np.complex128 else torch.complex64
    rdt = torch.float64 if dtype == np.complex128 else torch.float32
    fs = data(m, n, K, dtype, "both")
    a, left, right, mid, s = stack(fs)
    base = residual(a, left, right, mid, s)
    # transposed storage of every operand (the lanes of the staging loops then run along the other index)
    tr = lambda t: t.transpose(1, 2).contiguous().transpose(1, 2)  # noqa: E731
    assert all(same_bits(p, q) for p, q in zip(residual(tr(a), tr(left), tr(right), tr(mid), s), base))
    # padded views: every operand a window of a larger NaN-filled array
    def padded(t):
        big = torch.full((t.shape[0] + 1, t.shape[1] + 3, t.shape[2] + 5), complex(float("nan"), float("nan")), dtype=t.dtype, device="cuda")
        big[1:, 2:2 + t.shape[1], 4:4 + t.shape[2]] = t
        return big[1:, 2:2 + t.shape[1], 4:4 + t.shape[2]]
    sp = torch.full((2, K + 7), float("nan"), dtype=rdt, device="cuda")
    sp[:, :K] = s
    assert all(same_bits(p, q) for p, q in zip(residual(padded(a), padded(left), padded(right), padded(mid), sp), base))
    # a strided e, row-major and column-major, whose gaps stay untouched; with and without e and nrm
    fill = complex(-7.0, 3.0)
    for colmajor in (False, True):
        buf = torch.full((2, n + 3, m + 2) if colmajor else (2, m + 2, n + 3), fill, dtype=tdt, device="cuda")
        e = buf.transpose(1, 2)[:, 1:1 + m, 2:2 + n] if colmajor else buf[:, 1:1 + m, 2:2 + n]
        err = torch.zeros(2, dtype=rdt, device="cuda")
        nrm = torch.zeros(2, dtype=rdt, device="cuda")
        assert raw(tdt, a, left, right, mid, s, e=e, err=err, nrm=nrm) == 0
        torch.cuda.synchronize()
        assert same_bits(npy(err), base[0]) and same_bits(npy(nrm), base[1]) and same_bits(npy(e), base[2])
        mask = torch.ones(buf.shape, dtype=torch.bool, device="cuda")
        (mask.transpose(1, 2) if colmajor else mask)[:, 1:1 + m, 2:2 + n] = False
        assert bool(torch.all(buf[mask] == fill))
    err = torch.zeros(2, dtype=rdt, device="cuda")
    assert raw(tdt, a, left, right, mid, s, err=err) == 0  # neither e nor nrm
    torch.cuda.synchronize()
    assert same_bits(npy(err), base[0])
    got = residual(a, left, right, mid, s, want_e=False)  # nrm without e
    assert same_bits(got[0], base[0]) and same_bits(got[1], base[1])
    # a batch stride of 0 on a and on the factors: every block is block 0
    rep = lambda t: t[:1].expand(3, *t.shape[1:])  # noqa: E731
    got = residual(rep(a), rep(left), rep(right), rep(mid), rep(s))
    for i in range(3):
        assert all(same_bits(g[i], b[0]) for g, b in zip(got, base))


def test_graph_capture_replays_the_eager_bits():
    m, n, K, count = 96, 130, 24, 33
    rng = np.random.default_rng(8)
    fs = [rrc.gaussian_factors(rng, m, n, K, np.complex128, "both") for _ in range(count)]
    lib = _lib.lib()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        a, left, right, mid, s = stack(fs)
        ranks = tt((np.arange(count) % (K + 3) - 1).astype(np.int64))
        eager = residual(a, left, right, mid, s, ranks)
        ctx = _lib.Context(torch.cuda.current_device(), st.cuda_stream)
        e = torch.zeros((count, m, n), dtype=torch.complex128, device="cuda")
        err = torch.zeros(count, dtype=torch.float64, device="cuda")
        nrm = torch.zeros(count, dtype=torch.float64, device="cuda")
        # W of these blocks lives in the workspace: the context's arena is sized by one eager call before the capture, as the library asks
        assert raw(torch.complex128, a, left, right, mid, s, ranks, e, err, nrm, ctx=ctx) == 0
        ctx.synchronize()
        e.zero_(), err.zero_(), nrm.zero_()
        st.synchronize()
        graph = ctypes.c_void_p(None)
        ctx.check(lib.rc_graph_begin_capture(ctx._h))
        assert raw(torch.complex128, a, left, right, mid, s, ranks, e, err, nrm, ctx=ctx) == 0
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


# ---------------------------------------------------------------- 9. non-finite input stays in its block
@pytest.mark.parametrize("dtype", DTYPES)
def test_non_finite_input_stays_in_its_block(dtype):
    m, n, K = 40, 70, 6
    rng = np.random.default_rng(71)
    fs = [rrc.gaussian_factors(rng, m, n, K, dtype, "both") for _ in range(5)]
    clean = residual(*stack(fs))
    fs[1]["a"][3, 4] = complex(np.nan, 1.0)
    fs[3]["left"][0, 0] = complex(1.0, np.inf)
    fs[3]["s"][2] = np.nan
    got = residual(*stack(fs))
    for i in (0, 2, 4):
        assert all(same_bits(g[i], c[i]) for g, c in zip(got, clean))
    assert np.isnan(got[0][1]) and np.isnan(got[1][1]) and np.isnan(got[2][1][3, 4]) and np.sum(np.isnan(got[2][1])) == 1
    assert not np.isfinite(got[0][3]) and same_bits(got[1][3], clean[1][3])


# ---------------------------------------------------------------- 10. arguments
def test_arguments():
    dt, rt = torch.complex128, torch.float64
    z = lambda *shape: torch.zeros(shape, dtype=dt, device="cuda")  # noqa: E731
    zr = lambda *shape: torch.zeros(shape, dtype=rt, device="cuda")  # noqa: E731
    bad = _lib.RC_INVALID_ARGUMENT
    m, n, K, count = 6, 7, 3, 2
    a, left, right, mid, s = z(count, m, n), z(count, m, K), z(count, K, n), z(count, K, K), zr(count, K)
    err, nrm, e = zr(count), zr(count), z(count, m, n)
    assert raw(dt, a, left, right, mid, s, None, e, err, nrm) == 0
    assert raw(torch.complex64, a.to(torch.complex64), left.to(torch.complex64), right.to(torch.complex64), err=err.float()) == 0
    # count = 0 is a no-op, null pointers included
    err.fill_(5.0)
    assert raw(dt, a, left, right, err=None, count=0) == 0
    got = rc.lowrank_residual_batched_complex(z(0, m, n), z(0, m, K), z(0, K, n), want_residual=True)
    assert got[0].shape == (0,) and got[1].shape == (0,) and got[2].shape == (0, m, n) and got[0].dtype == rt and got[2].dtype == dt
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
    # an e batch stride (in complex elements) smaller than one view's span: only with more than one block
    assert raw(dt, a, left, right, e=e, err=err, e_bs=m * n - 1) == bad
    assert raw(dt, a[:1], left[:1], right[:1], e=e[:1], err=err, e_bs=0) == 0
    # null pointers
    for which in ("a", "left", "right"):
        assert raw(dt, a, left, right, err=err, null=which) == bad, which
    assert raw(dt, a, left, right, err=None) == bad
    torch.cuda.synchronize()
    # Python: wrong dtypes raise TypeError, the library's INVALID_ARGUMENT an AssertionError
    with pytest.raises(TypeError):
        rc.lowrank_residual_batched_complex(a.real.contiguous(), left.real.contiguous(), right.real.contiguous())
    with pytest.raises(TypeError):
        rc.lowrank_residual_batched_complex(a, left.to(torch.complex64), right)
    with pytest.raises(TypeError):
        rc.lowrank_residual_batched_complex(a, left, right, s=s.to(dt))
    with pytest.raises(TypeError):
        rc.lowrank_residual_batched_complex(a, left, right, s=s.float())
    with pytest.raises(TypeError):
        rc.lowrank_residual_batched_complex(a, left, right, ranks=torch.zeros(count, dtype=torch.int32, device="cuda"))
    with pytest.raises(TypeError):  # the real call keeps refusing complex data
        rc.lowrank_residual_batched(a, left, right)
    with pytest.raises(AssertionError, match="lowrank_residual_batched"):
        rc.lowrank_residual_batched_complex(z(1, m, 513), left[:1], z(1, K, 513))
