"""Batched recompression of complex factor pairs with both factors tall (rc_lowrank_recompress_complex_large_batched_c64 / _c32,
batch.lowrank_recompress_large_batched_complex and its wrapper svd_add_large_batched_complex): the complex twin of
tests/test_gpu_batched_recompress_large.py.

The oracle, the bounds and the block generators are those of tests/test_gpu_batched_recompress_complex.py (check_block: 4 TOL sigma with
sigma the product of the factors' 2-norms, TOL keyed by the real dtype), the vector and phase checks those of
tests/test_gpu_batched_svd_complex.py, phase_normalise that of tests/test_gpu_batched_recompress_tall_complex.py.  For n > 512 the right
factor goes, as its plain transpose, through exactly the flat Householder TSQR the left factor goes through in the tall complex call
(stages of H = 512 rows; stage 0 holds rows 0 .. 511 and every later stage the next 512 - q rows, so the stage edges of a side of length x
are at x = 512 + j (512 - q)); the numpy model of that scheme quoted in the tall complex test therefore covers both sides.  For n <= 512
the call is the tall complex call bit for bit.

A dense reference SVD is the cost of a case, so no side goes above about 2100; the one block with n = 65536 is checked from thin QRs of its
factors in c128 (check_from_factors), never formed."""
import ctypes

import numpy as np
import pytest
import torch

import rusty_compression_amd as rc
from rusty_compression_amd import _lib
from tests.helpers import TOL, batched_launch, npy
from tests.test_gpu_batched_recompress_complex import check_block, clamp, dense, factors, gaussian, orthonormal, stack
from tests.test_gpu_batched_recompress_tall_complex import phase_normalise
from tests.test_gpu_batched_svd_complex import check_phases, check_vectors, clear_top, gaps, real_of

pytestmark = pytest.mark.gpu

C64, C32 = np.complex128, np.complex64
INVALID = 5
H = 512
MODES = ("none", "mid", "s", "both")
DTYPES = [C64, C32]
KINDS = ("gauss", "spectrum", "scaled")
NAME = "lowrank_recompress_complex_large_batched"
OP = "batched_recompress_large<complex>"


def cuda(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def recompress_large(left, right, k, tol=0.0, mid=None, s=None, ranks=None):
    out = rc.lowrank_recompress_large_batched_complex(cuda(left), cuda(right), k, tol, mid=cuda(mid), s=cuda(s), ranks=cuda(ranks))
    torch.cuda.synchronize()
    return tuple(npy(t) for t in out)


def stages(x, q):
    return 1 if x <= H else 1 + -(-(x - H) // (H - q))


def chunks(x, q):
    """The row ranges of a side of length x that the stages write, first to last: [0, 512), then 512 - q rows each."""
    edges = [0, min(H, x)]
    while edges[-1] < x:
        edges.append(min(edges[-1] + H - q, x))
    return list(zip(edges[:-1], edges[1:]))


def check_from_factors(left, right, mid, s, q, u, s_out, vt, r, kk, dtype):
    """check_block's checks for a block too large to form: the reference SVD from thin QRs of the factors in c128 (left = Ql Rl, the plain
    transpose right^T = Qr Rr, the SVD of Rl core Rr^T = Uc S Vc^H, so u = Ql Uc and vt = Vc^H Qr^T), and ||A - U S Vt||_2 as the 2-norm of
    [left_q, U] [core right_q; -S Vt], again through thin QRs.  Returns the reference (u, s, vt) at full inner rank q."""
    rd = real_of(dtype)
    t = TOL[rd]
    lf, rt = left[:, :q].astype(C64), right[:q].astype(C64)
    core = np.eye(q, dtype=C64) if mid is None else mid[:q, :q].astype(C64)
    if s is not None:
        core = core * s[:q].astype(np.float64)[None, :]
    ql, rl = np.linalg.qr(lf)
    qr, rr = np.linalg.qr(rt.T)
    sigma = float(np.linalg.norm(rl, 2) * np.linalg.norm(core, 2) * np.linalg.norm(rr, 2))
    uc, sref, vch = np.linalg.svd(rl @ core @ rr.T)
    ref_u, ref_vt = ql @ uc, vch @ qr.T
    assert s_out.dtype == rd and u.dtype == np.dtype(dtype) and vt.dtype == np.dtype(dtype)
    assert 0 <= r <= min(kk, q)
    assert not np.any(s_out[q:])
    sv = s_out[:q].astype(np.float64)
    assert np.all(np.diff(sv) <= 0)
    err_s = np.abs(sv - sref).max()
    print(f"    sval err {err_s:.3e} bound {4 * t['sval'] * sigma:.3e}")
    assert err_s <= 4 * t["sval"] * sigma, (err_s, sigma)
    assert not np.any(u[:, r:]) and not np.any(vt[r:])
    ur, vr = u[:, :r].astype(C64), vt[:r].astype(C64)
    orth_u, orth_v = np.abs(ur.conj().T @ ur - np.eye(r)).max(), np.abs(vr @ vr.conj().T - np.eye(r)).max()
    q1, r1 = np.linalg.qr(np.concatenate([lf, ur], axis=1))
    q2, r2 = np.linalg.qr(np.concatenate([core @ rt, -(sv[:r, None] * vr)], axis=0).T)  # the plain transpose: the product is q1 r1 r2^T q2^T
    err = np.linalg.norm(r1 @ r2.T, 2)
    tail = sref[r] if r < q else 0.0
    print(f"    orth u {orth_u:.3e} vt {orth_v:.3e} bound {4 * t['orth']:.3e}; recon {err:.3e} tail {tail:.3e} bound {4 * t['recon'] * sigma:.3e}")
    assert max(orth_u, orth_v) <= 4 * t["orth"]
    assert err <= 4 * t["recon"] * sigma + tail, (err, tail, sigma)
    check_phases(u, r)
    return ref_u, sref, ref_vt


def report(tag, a, sigma, u, s_out, vt, ref, r, dtype):
    """The block's ratios to the family's bounds (singular values, orthonormality of u and of vt, reconstruction), one line."""
    t = TOL[real_of(dtype)]
    sv, ur, vr = s_out[:r].astype(np.float64), u[:, :r].astype(C64), vt[:r].astype(C64)
    rs = np.abs(s_out[:len(ref.s)].astype(np.float64) - ref.s[:len(s_out)]).max() / (4 * t["sval"] * sigma)
    ru = np.abs(ur.conj().T @ ur - np.eye(r)).max() / (4 * t["orth"])
    rv = np.abs(vr @ vr.conj().T - np.eye(r)).max() / (4 * t["orth"])
    rr = max(np.linalg.norm(a - (ur * sv) @ vr, 2) - (ref.s[r] if r < len(ref.s) else 0.0), 0.0) / (4 * t["recon"] * sigma)
    print(f"  RATIO {tag} sval {rs:.4f} orth_u {ru:.4f} orth_vt {rv:.4f} recon {rr:.4f}")


# ---------------------------------------------------------------- 1. n <= 512: the bits of the tall complex call
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m,n,K", [(64, 64, 40), (512, 512, 128), (513, 130, 128), (2100, 64, 64), (1500, 512, 40)])
def test_up_to_512_columns_the_bits_are_the_tall_complex_calls(m, n, K, dtype):
    rng = np.random.default_rng(100 + m + n)
    qs = np.array([K, K // 2, 0, K + 3, K - 1], dtype=np.int64)
    k = max(1, (2 * K) // 3)
    ran = 0
    for mode in MODES:
        left, right, mid, s = (cuda(x) for x in stack([factors(rng, "gauss", m, n, K, mode, dtype) for _ in qs]))
        for tol in (0.0, 1e-3):
            for ranks in (None, cuda(qs)):
                want = rc.lowrank_recompress_tall_batched_complex(left, right, k, tol, mid=mid, s=s, ranks=ranks)
                got = rc.lowrank_recompress_large_batched_complex(left, right, k, tol, mid=mid, s=s, ranks=ranks)
                for name, v, w in zip(("u", "s_out", "vt", "ranks"), want, got):
                    assert torch.equal(v, w), (m, n, K, mode, tol, name)
                ran += 1
    assert ran == 16


# ---------------------------------------------------------------- 2. oracle parity at the right factor's stage edges
# the first extra column, the edge between stages 1 and 2 at q = 128 (896 | 897) and at q = 17 (1021 | 1022) on the right, the left side on
# either side of 512, four to five stages on the right under a short left factor
EDGES = [(513, 513, 3), (130, 513, 128), (130, 896, 128), (130, 897, 128), (600, 897, 128), (897, 600, 128), (17, 1021, 17), (1022, 1022, 17),
         (1100, 1500, 40), (64, 2100, 64)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("m,n,K", EDGES)
def test_oracle_parity_at_the_stage_edges(m, n, K, mode, dtype):
    """The seeds and the draw order (KINDS) are fixed: at exactly these, the oracle's own phase-normalised vectors pass check_vectors on 6-9
    triplets in c64 and 4-6 in c32 for K >= 6 and on 2-3 at K = 3 (checked on the host over all 80 spectrum blocks), which is what the cap
    got >= 3 or K < 6 rests on."""
    rng = np.random.default_rng(m * 100000 + n * 100 + K + MODES.index(mode))
    blocks = [factors(rng, kind, m, n, K, mode, dtype) for kind in KINDS]
    left, right, mid, s = stack(blocks)
    u, s_out, vt, ranks = recompress_large(left, right, K, 0.0, mid, s)
    assert u.shape == (3, m, K) and s_out.shape == (3, K) and vt.shape == (3, K, n)
    for i, kind in enumerate(KINDS):
        tag = f"{m}x{n} K={K} {np.dtype(dtype).name} {mode} {kind} stages={stages(m, K)},{stages(n, K)}"
        print("  " + tag)
        a, sigma = dense(*blocks[i], K)
        assert ranks[i] == K
        ref = check_block(a, sigma, u[i], s_out[i], vt[i], K, K, K, dtype)
        report(tag, a, sigma, u[i], s_out[i], vt[i], ref, K, dtype)
        if kind == "spectrum":  # sigma = s_0: the gap rule of the batched SVD's vectors applies as it stands
            own = check_vectors(*phase_normalise(ref.u[:, :K], ref.vt[:K]), ref.u, ref.vt, ref.s, K, dtype)
            got = check_vectors(u[i], vt[i], ref.u, ref.vt, ref.s, K, dtype)
            assert got == own
            assert got >= 3 or K < 6, (got, K)


# ---------------------------------------------------------------- 3. the last column of the domain
@pytest.mark.parametrize("dtype", DTYPES)
def test_the_last_column_of_the_domain(dtype):
    """n = 65536, K = 8: 1 + ceil(65024 / 504) = 131 stages on the right, two on the left (m = 600); column indices and chunk offsets of vt at
    their largest values.  The reference comes from thin QRs of the factors."""
    rng = np.random.default_rng(65536)
    m, n, K = 600, 65536, 8
    assert stages(n, K) == 131 and stages(m, K) == 2
    b = list(factors(rng, "spectrum", m, n, K, "s", dtype))
    left, right, mid, s = stack([tuple(b)])
    (u, s_out, vt, ranks), lab = batched_launch(lambda: recompress_large(left, right, K, 0.0, mid, s))
    assert lab["op"] == OP and lab["plan"].startswith("stages=2,rstages=131,L:ws,R:ws,")
    assert ranks[0] == K and vt.shape == (1, K, n)
    ref_u, ref_s, ref_vt = check_from_factors(b[0], b[1], b[2], b[3], K, u[0], s_out[0], vt[0], K, K, dtype)
    assert check_vectors(u[0], vt[0], ref_u, ref_vt, ref_s, K, dtype) >= 3
    assert np.all(np.abs(vt[0][:, -1]) > 0)  # the last column is written


# ---------------------------------------------------------------- 4. the phase rule's row at the end of a staged left factor
@pytest.mark.parametrize("dtype", DTYPES)
def test_phase_rule_finds_a_dominant_entry_in_the_last_row(dtype):
    """Both sides staged (m = 1100: three stages, n = 1500: four): the dominant entry of a column of u sits in the last row, so the last
    chunk's last lane decides a phase; the entry comes out exactly (|x|, 0)."""
    rng = np.random.default_rng(1100)
    m, n, K = 1100, 1500, 40
    assert stages(m, K) == 3 and stages(n, K) == 4
    b = factors(rng, "gauss", m, n, K, "s", dtype)
    b[0][:-1, 0] *= 0.01
    b[0][-1, 0] = 30.0 * np.exp(0.7j)
    left, right, mid, s = stack([b])
    u, s_out, vt, ranks = recompress_large(left, right, K, 0.0, mid, s)
    col = int(np.argmax(np.abs(u[0]).max(axis=0)))
    assert int(np.argmax(np.abs(u[0][:, col]))) == m - 1
    assert u[0][m - 1, col].imag == 0 and u[0][m - 1, col].real > 0
    a, sigma = dense(*b, K)
    assert ranks[0] == K
    check_block(a, sigma, u[0], s_out[0], vt[0], K, K, K, dtype)


# ---------------------------------------------------------------- 5. the inner rank sets the stage height on both sides
@pytest.mark.parametrize("dtype", DTYPES)
def test_in_ranks_give_the_truncated_calls_bits_and_tails_are_never_read(dtype):
    rng = np.random.default_rng(31)
    m, n, K, k = 1100, 1100, 64, 40
    qs = np.array([1, 17, 64, 0, -3, 99], dtype=np.int64)
    blocks = [factors(rng, "gauss", m, n, K, "both", dtype) for _ in qs]
    left, right, mid, s = (x.copy() for x in stack(blocks))
    for i, q in enumerate(qs):
        q = clamp(q, K)
        left[i][:, q:] = np.nan
        right[i][q:] = np.nan
        mid[i][q:] = np.nan
        mid[i][:, q:] = np.nan
        s[i][q:] = np.nan
    u, s_out, vt, ranks = recompress_large(left, right, k, 0.0, mid, s, qs)
    for i, q in enumerate(qs):
        q = clamp(q, K)
        print(f"  q={q} {np.dtype(dtype).name}")
        assert ranks[i] == min(k, q)
        if q == 0:
            assert not np.any(u[i]) and not np.any(vt[i]) and not np.any(s_out[i])
            continue
        tl, tr, tm, ts = blocks[i]
        check_from_factors(tl, tr, tm, ts, q, u[i], s_out[i], vt[i], int(ranks[i]), k, dtype)
        # the truncated factors as a call of their own (inner width q): the same bits
        tu, tsv, tvt, trk = recompress_large(tl[None, :, :q], tr[None, :q], k, 0.0, tm[None, :q, :q], ts[None, :q])
        r = int(ranks[i])
        assert trk[0] == r
        assert np.array_equal(tsv[0], s_out[i][:q]) and np.array_equal(tu[0][:, :r], u[i][:, :r]) and np.array_equal(tvt[0][:r], vt[i][:r])


# ---------------------------------------------------------------- 6. stage counts differ across one batch
@pytest.mark.parametrize("dtype", DTYPES)
def test_the_stage_counts_differ_across_inner_ranks_of_one_batch(dtype):
    """1534 x 1470 at q = 17, 64, 128 (and the clamped 0 and K + 5): the right factor takes three stages at q = 17 (512 + 2 * 495 = 1502) and
    four above, the left factor four at every q with last stages of different heights; one workgroup runs blocks of different stage counts
    one after the other, and each block's bits are those of the call that holds it alone."""
    rng = np.random.default_rng(32)
    m, n, K = 1534, 1470, 128
    qs = np.array([17, 64, 128, 0, K + 5, 17], dtype=np.int64)
    assert [stages(m, q) for q in (17, 64, 128)] == [4, 4, 4] and [stages(n, q) for q in (17, 64, 128)] == [3, 4, 4]
    blocks = [factors(rng, "gauss", m, n, K, "s", dtype) for _ in qs]
    left, right, mid, s = stack(blocks)
    u, s_out, vt, ranks = recompress_large(left, right, K, 0.0, mid, s, qs)
    for i, q in enumerate(qs):
        q = clamp(q, K)
        assert ranks[i] == q
        if q == 0:
            assert not np.any(u[i]) and not np.any(vt[i]) and not np.any(s_out[i])
            continue
        lone = recompress_large(left[i:i + 1], right[i:i + 1], K, 0.0, None, s[i:i + 1], qs[i:i + 1])
        for name, v, w in zip(("u", "s_out", "vt", "ranks"), lone, (u, s_out, vt, ranks)):
            assert np.array_equal(v[0], w[i]), (i, q, name)
        if i < 3:
            check_from_factors(*blocks[i], q, u[i], s_out[i], vt[i], q, K, dtype)


# ---------------------------------------------------------------- 7. exact zeros and rank deficiency
@pytest.mark.parametrize("dtype", DTYPES)
def test_zero_columns_of_left_and_zero_rows_of_right_give_exactly_zero_singular_values(dtype):
    """Zero columns of left, zero rows of right, and both together (the zero tails the batched calls write past a rank, which is what a
    concatenation hands to this call): each is an exactly zero singular value, the rank stops there at tol = 0, and the block meets
    check_block's bounds.  A zero row of right is a zero column of every stack of the right factor (pivoted last, tau = 0) and a zero row
    of R_R; where R_R has fewer nonzero rows than R_L the kernel runs the iteration on C instead of C^H, so that the zero rows are zero
    columns there as those of R_L are in C^H."""
    rng = np.random.default_rng(42)
    m, n, K = 700, 900, 24
    for mode in MODES:
        zl, zr, zm, zs = factors(rng, "gauss", m, n, K, mode, dtype)
        zl[:, [3, 7, 20]] = 0                  # zero in every stage
        bl, br, bm, bs = factors(rng, "gauss", m, n, K, mode, dtype)
        bl[:, [2, 11]] = 0                     # a truncated SVD's tails: the column of left and the row of right
        br[[2, 11]] = 0
        rl, rr, rm, rs = factors(rng, "gauss", m, n, K, mode, dtype)
        rr[[4, 9, 23]] = 0                     # zero rows of right alone: zero in every stage of the right factor
        pl, pr, pm, ps = factors(rng, "gauss", m, n, K, mode, dtype)
        pl[H:, 5] = 0                          # zero only below the first stage: not a zero column
        pr[6, H:] = 0                          # likewise on the right
        xl, xr, xm, xs = factors(rng, "gauss", m, n, K, mode, dtype)
        xl[:, [5]] = 0                         # more zero rows on the right than zero columns on the left, the column among them
        xr[[5, 6, 22]] = 0
        blocks = [(zl, zr, zm, zs), (bl, br, bm, bs), (pl, pr, pm, ps), (rl, rr, rm, rs), (xl, xr, xm, xs)]
        want = [21, 22, 24, 21, 21]
        left, right, mid, s = stack(blocks)
        ctx = _lib.default_context()
        ctx.synchronize()
        ctx.get_health()
        u, s_out, vt, ranks = recompress_large(left, right, K, 0.0, mid, s)
        assert ctx.get_health() == 0
        for i, w in enumerate(want):
            print(f"  {mode} {np.dtype(dtype).name} block {i}: s[{w}:] = {s_out[i][w:]}, rank {ranks[i]}")
            assert np.all(np.isfinite(s_out[i])), (mode, i, s_out[i])
            assert np.all(s_out[i][:w] > 0) and not np.any(s_out[i][w:]), (mode, i, s_out[i])
        assert list(ranks) == want
        for i in range(len(blocks)):
            a, sigma = dense(*blocks[i], K)
            check_block(a, sigma, u[i], s_out[i], vt[i], int(ranks[i]), K, K, dtype)


# ---------------------------------------------------------------- 8. rounded addition
@pytest.mark.parametrize("dtype", DTYPES)
def test_svd_add_of_a_block_with_itself(dtype):
    """x + x through the rank-deficient factors [U U], [Vt; Vt] truncated to k: rank k, the singular values are 2 s, the other k are rounding of
    sigma.  ranks1 / ranks2 cut the addends: NaN past them is not seen."""
    rng = np.random.default_rng(43)
    cnt, m, n, k = 3, 900, 700, 12
    rd = real_of(dtype)
    t = TOL[rd]
    u0 = np.stack([orthonormal(rng, m, k) for _ in range(cnt)]).astype(dtype)
    vt0 = np.stack([orthonormal(rng, n, k).conj().T for _ in range(cnt)]).astype(dtype)
    s0 = np.stack([np.sort(rng.uniform(0.5, 2.0, k))[::-1] for _ in range(cnt)]).astype(rd)
    u, s_out, vt, ranks = (npy(x) for x in rc.svd_add_large_batched_complex(cuda(u0), cuda(s0), cuda(vt0), cuda(u0), cuda(s0), cuda(vt0), k, 0.0))
    torch.cuda.synchronize()
    assert s_out.shape == (cnt, 2 * k) and u.shape == (cnt, m, k) and vt.shape == (cnt, k, n) and s_out.dtype == rd
    for i in range(cnt):
        lf, rt = np.concatenate([u0[i]] * 2, axis=1), np.concatenate([vt0[i]] * 2, axis=0)
        a, sigma = dense(lf, rt, None, np.concatenate([s0[i]] * 2), 2 * k)
        err = np.abs(s_out[i][:k].astype(np.float64) - 2.0 * s0[i].astype(np.float64)).max()
        rest = np.abs(s_out[i][k:]).max()
        print(f"  block {i} {np.dtype(dtype).name}: |s - 2 s0| {err:.3e}, rest {rest:.3e}, bound {4 * t['sval'] * sigma:.3e}")
        assert err <= 4 * t["sval"] * sigma and rest <= 4 * t["sval"] * sigma
        assert ranks[i] == k
        check_block(a, sigma, u[i], s_out[i], vt[i], k, 2 * k, k, dtype)
    # the addends cut at their ranks: what lies past them may be anything
    r1, r2 = np.array([k, 5, 0], dtype=np.int64), np.array([3, k, 7], dtype=np.int64)
    un, sn, vn = u0.copy(), s0.copy(), vt0.copy()
    u2, s2, v2 = u0.copy(), s0.copy(), vt0.copy()
    for i in range(cnt):
        un[i][:, r1[i]:], sn[i][r1[i]:], vn[i][r1[i]:] = complex(np.nan, 3.0), np.nan, complex(-7.0, np.nan)
        u2[i][:, r2[i]:], s2[i][r2[i]:], v2[i][r2[i]:] = 1e30, -5.0, complex(np.nan, np.nan)
    cu, cs, cv, cr = (npy(x) for x in rc.svd_add_large_batched_complex(cuda(un), cuda(sn), cuda(vn), cuda(u2), cuda(s2), cuda(v2), k, 0.0,
                                                                       ranks1=cuda(r1), ranks2=cuda(r2)))
    torch.cuda.synchronize()
    for i in range(cnt):
        assert cr[i] == max(r1[i], r2[i])  # the addends share their leading triplets, so the sum has the larger rank
        w = np.zeros(k)
        w[:r1[i]] += s0[i][:r1[i]].astype(np.float64)
        w[:r2[i]] += s0[i][:r2[i]].astype(np.float64)
        a = (u0[i].astype(C64) * w) @ vt0[i].astype(C64)
        check_block(a, 2.0 * float(s0[i][0]), cu[i], cs[i], cv[i], int(cr[i]), 2 * k, k, dtype)


# ---------------------------------------------------------------- 9. phases
@pytest.mark.parametrize("dtype", DTYPES)
def test_phase_rule_with_the_right_factor_in_three_stages(dtype):
    """K = 3, m = n = 1100: u's chunks of rows are [0, 512), [512, 1021), [1021, 1100) and vt's chunks of columns are the same.  u's first
    column is, up to a phase, the first column of left, which carries one dominant entry in a chosen chunk.  Multiplying that column of left
    by a unit-modulus number changes nothing in u after the rule, and rotates row 0 of vt by that number: the conjugate of the phase the rule
    applies to u.  Every chunk of a row of vt carries the one phase: each is compared on its own with conj(ph) times the reference's row, ph
    the phase the rule applies to the reference's column, under check_vectors' bound 200 eps / min(gap, 1)."""
    rng = np.random.default_rng(51)
    m, n, K = 1100, 1100, 3
    rd = real_of(dtype)
    eps = np.finfo(rd).eps
    assert stages(m, K) == 3 and stages(n, K) == 3 and chunks(n, K) == [(0, 512), (512, 1021), (1021, 1100)]
    turns = [np.exp(0.9j), -1.0, 1j, np.exp(-2.3j), np.exp(0.1j)]
    blocks, rows = [], []
    for row, turn in zip((1090, 5, 700, 1021, 511), turns):
        spike = 0.01 * gaussian(rng, m, 1)[:, 0]
        spike[row] = np.exp(0.4j)
        q1 = np.linalg.qr(np.column_stack([spike, gaussian(rng, m, K - 1)]))[0]
        rt = orthonormal(rng, n, K).conj().T
        for f in (1.0, turn):
            lf = q1.copy()
            lf[:, 0] *= f
            blocks.append((lf.astype(dtype), rt.astype(dtype), None, np.array([4.0, 2.0, 1.0], dtype=rd)))
            rows.append(row)
    left, right, mid, s = stack(blocks)
    u, s_out, vt, ranks = recompress_large(left, right, K, 0.0, mid, s)
    for i, row in enumerate(rows):
        assert ranks[i] == K
        assert int(np.argmax(np.abs(u[i][:, 0]))) == row, (i, row)
        assert u[i][row, 0].imag == 0 and u[i][row, 0].real > 0, (i, row, u[i][row, 0])
        ref_u, ref_s, ref_vt = check_from_factors(*blocks[i], K, u[i], s_out[i], vt[i], K, K, dtype)
        assert check_vectors(u[i], vt[i], ref_u, ref_vt, ref_s, K, dtype) >= 1  # gaps of 1/4 of s_0; the spiked column's top entry is clear
        g = gaps(ref_s)
        assert clear_top(ref_u[:, 0])
        for j in range(K):
            if not clear_top(ref_u[:, j]):  # check_vectors' guard: two entries of almost the same modulus make the rule fragile
                continue
            x = ref_u[int(np.argmax(np.abs(ref_u[:, j]))), j]
            ph = np.conj(x) / abs(x)
            bound = 200 * eps / min(g[j], 1.0)
            for lo, hi in chunks(n, K):
                d = np.abs(vt[i][j, lo:hi] - np.conj(ph) * ref_vt[j, lo:hi]).max()
                assert d <= bound, (i, j, lo, hi, d, bound)
    for i in range(0, len(blocks), 2):  # the pair: the same u column, row 0 of vt rotated by the factor applied to left's column
        turn = turns[i // 2]
        bound = 2 * 200 * eps / 0.5  # each of the two is within 200 eps / gap of its reference (above), and the first gap is 1/2 of s_0
        assert np.abs(u[i + 1][:, 0] - u[i][:, 0]).max() <= bound
        for lo, hi in chunks(n, K):
            assert np.abs(vt[i + 1][0, lo:hi] - turn * vt[i][0, lo:hi]).max() <= bound, (i, lo, hi)


@pytest.mark.parametrize("dtype", DTYPES)
def test_phase_rule_on_entries_of_equal_modulus_in_different_chunks(dtype):
    """Left factors of one column built from exact entries in {1, -1, i, -i} in two or three chunks (K = 1, m = 1100: chunks [0, 512),
    [512, 1023), [1023, 1100)) beside a right factor of 600 columns in two stages: u's column has entries of the same modulus up to rounding
    in different chunks, and where they come out equal to the last bit the earlier row decides.  Either way the first largest entry must be
    real positive and the others follow it.  The product by the phase moves the other entries' moduli by up to an ulp, so where numpy's
    first largest modulus of the output is not the real positive entry, that entry must be an earlier or later row of the same modulus to
    2 eps."""
    m, n = 1100, 600
    cases = [{3: -1j, 800: 1.0}, {3: 1.0, 800: -1j}, {600: -1.0, 1050: 1j}, {0: -1j, 512: 1.0, 1023: 1j}, {511: 1j, 1099: -1.0}, {3: 1j, 800: 1j}]
    left = np.zeros((len(cases), m, 1), dtype=dtype)
    for i, c in enumerate(cases):
        for row, v in c.items():
            left[i, row, 0] = v
    right = np.zeros((len(cases), 1, n), dtype=dtype)
    right[:, 0, 1] = 1.0
    (u, s_out, vt, ranks), lab = batched_launch(lambda: recompress_large(left, right, 1, 0.0))
    assert lab["op"] == OP and lab["plan"].startswith("stages=3,rstages=2,")
    ties = 0
    eps = np.finfo(real_of(dtype)).eps
    for i, c in enumerate(cases):
        col = u[i][:, 0]
        rows = sorted(c)
        assert ranks[i] == 1 and not np.any(np.delete(col, rows))
        first = int(np.argmax(np.abs(col)))
        assert first in rows
        if not (col[first].imag == 0 and col[first].real > 0):
            pivots = [r for r in rows if col[r].imag == 0 and col[r].real > 0 and abs(col[r]) >= abs(col[first]) * (1 - 2 * eps)]
            assert pivots, (i, first, col[rows])
            first = pivots[0]
        want = col[first] * np.array([c[r] for r in rows]) / c[first]
        assert np.abs(col[rows] - want).max() <= 4 * eps, (i, col[rows], want)
        assert abs(float(s_out[i][0]) - np.sqrt(len(c))) <= 4 * TOL[real_of(dtype)]["sval"] * np.sqrt(len(c))
        # vt = conj(phase) times the input's row: u s vt rebuilds the block
        assert np.abs((col[:, None] * s_out[i][0]) @ vt[i] - left[i] @ right[i]).max() <= 8 * eps
        ties += int(np.sum(np.abs(col[rows]) == np.abs(col[first])) > 1)
    print(f"  {np.dtype(dtype).name}: {ties} of {len(cases)} columns hold an exact tie")


# ---------------------------------------------------------------- 10. symmetries
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m,n,K", [(600, 897, 128), (1022, 1022, 17)])
def test_conjugated_inputs_give_conjugated_outputs_bit_for_bit(m, n, K, dtype):
    rng = np.random.default_rng(65 + m)
    k = max(1, (2 * K) // 3)
    left, right, mid, s = stack([factors(rng, kind, m, n, K, "both", dtype) for kind in ("gauss", "spectrum", "scaled", "gauss")])
    qs = np.array([K, K, K, K // 2 + 1], dtype=np.int64)
    u, s_out, vt, ranks = recompress_large(left, right, k, 1e-6, mid, s, qs)
    cu, cs, cvt, cranks = recompress_large(left.conj(), right.conj(), k, 1e-6, mid.conj(), s, qs)
    assert np.array_equal(cs, s_out) and np.array_equal(cranks, ranks)
    assert np.array_equal(cu, u.conj()) and np.array_equal(cvt, vt.conj())
    # a lazily conjugated tensor is materialised by the Python call
    lazy = cuda(left.conj()).conj()
    assert lazy.is_conj()
    lz = rc.lowrank_recompress_large_batched_complex(lazy, cuda(right), k, 1e-6, mid=cuda(mid), s=cuda(s), ranks=cuda(qs))
    for v, w in zip((u, s_out, vt, ranks), lz):
        assert np.array_equal(v, npy(w))


@pytest.mark.parametrize("dtype", DTYPES)
def test_zero_imaginary_parts_stay_zero_and_match_the_real_large_call(dtype):
    rng = np.random.default_rng(66)
    cnt, m, n, K, k = 3, 1100, 900, 20, 20
    rd = real_of(dtype)
    t = TOL[rd]
    blocks = []
    for kind in KINDS:
        lf, rt, md, s = factors(rng, kind, m, n, K, "both", dtype)
        blocks.append((lf.real.astype(dtype), rt.real.astype(dtype), md.real.astype(dtype), s))
    left, right, mid, s = stack(blocks)
    u, s_out, vt, ranks = recompress_large(left, right, k, 0.0, mid, s)
    assert not np.any(u.imag) and not np.any(vt.imag), "real inputs must give exactly real singular vectors"
    ru, rs, rvt, rranks = (npy(x) for x in rc.lowrank_recompress_large_batched(cuda(left.real.astype(rd)), cuda(right.real.astype(rd)), k, 0.0,
                                                                               mid=cuda(mid.real.astype(rd)), s=cuda(s)))
    torch.cuda.synchronize()
    for i in range(cnt):
        a, sigma = dense(*blocks[i], K)
        assert ranks[i] == k and rranks[i] == k
        check_block(a, sigma, u[i], s_out[i], vt[i], k, K, k, dtype)
        # each call is within 4 TOL[sval] sigma of the oracle, so the two are within 8 of each other
        gap = np.abs(s_out[i].astype(np.float64) - rs[i].astype(np.float64)).max()
        print(f"  complex vs real singular values {gap:.3e} bound {8 * t['sval'] * sigma:.3e}")
        assert gap <= 8 * t["sval"] * sigma


# ---------------------------------------------------------------- 11. the batch contract
def _view(t):
    if t is None:
        return _lib.mat(None), ctypes.c_int64(0)
    return _lib.rc_matrix(t.data_ptr(), t.shape[1], t.shape[2], t.stride(1), t.stride(2)), ctypes.c_int64(t.stride(0))


def _raw(left, mid, s, right, in_ranks, cnt, k, tol, u, ubs, s_out, vt, vbs, ranks, ctx=None, dtype=torch.complex128):
    ctx = ctx or _lib.default_context()
    fn = getattr(_lib.lib(), f"rc_lowrank_recompress_complex_large_batched_{_lib.suffix(dtype)}")
    tol_arg = ctypes.c_double(tol) if dtype == torch.complex128 else ctypes.c_float(tol)  # tol has the real type of the data
    return fn(ctx._h, *_view(left), *_view(mid), ctypes.c_void_p(s.data_ptr() if s is not None else None),
              ctypes.c_int64(s.stride(0) if s is not None else 0), *_view(right), _lib.i64p(in_ranks), ctypes.c_int32(cnt), ctypes.c_int64(k),
              tol_arg, u, ctypes.c_int64(ubs), ctypes.c_void_p(s_out.data_ptr() if s_out is not None else None), vt, ctypes.c_int64(vbs),
              _lib.i64p(ranks))


def test_bits_independent_of_count_position_and_neighbours():
    rng = np.random.default_rng(61)
    m, n, K, k, tol = 513, 513, 8, 6, 1e-9
    protos = [factors(rng, kind, m, n, K, "both", C64) for kind in ("gauss", "spectrum", "scaled", "gauss", "gauss", "scaled", "gauss")]
    qs = [K, K, 5, 0, 1, K + 2, 3]
    alone = []
    labels = None
    for b, q in zip(protos, qs):
        out, labels = batched_launch(lambda: recompress_large(b[0][None], b[1][None], k, tol, b[2][None], b[3][None], np.array([q], dtype=np.int64)))
        alone.append(out)
    assert labels["op"] == OP and (labels["m"], labels["n"], labels["k"], labels["count"], labels["grid"]) == (m, n, K, 1, 1)
    cnt = 2 * labels["slots"] + 37  # every workgroup runs two blocks, 37 of them a third
    pick = [(5 * i + i // 7) % 7 for i in range(cnt)]
    left, right, mid, s = stack([protos[p] for p in pick])
    got, lab = batched_launch(lambda: recompress_large(left, right, k, tol, mid, s, np.array([qs[p] for p in pick], dtype=np.int64)))
    assert lab["count"] == cnt and lab["grid"] == lab["slots"] and lab["plan"] == labels["plan"]
    for i, p in enumerate(pick):
        for v, w in zip(alone[p], got):
            assert np.array_equal(v[0], w[i]), (i, p)


@pytest.mark.parametrize("dtype", DTYPES)
def test_input_views_give_the_same_bits(dtype):
    rng = np.random.default_rng(62)
    cnt, m, n, K, k = 4, 700, 1100, 12, 9
    left, right, mid, s = (cuda(x) for x in stack([factors(rng, "gauss", m, n, K, "both", dtype) for _ in range(cnt)]))
    ref = tuple(npy(x) for x in rc.lowrank_recompress_large_batched_complex(left, right, k, 1e-6, mid=mid, s=s))

    def colmajor(t):
        return t.transpose(1, 2).contiguous().transpose(1, 2)

    def padded(t):
        p = torch.zeros((t.shape[0], t.shape[1] + 3, t.shape[2] + 5), dtype=t.dtype, device=t.device)
        p[:, :t.shape[1], :t.shape[2]] = t
        return p[:, :t.shape[1], :t.shape[2]]

    def batch_last(t):
        return t.permute(1, 2, 0).contiguous().permute(2, 0, 1)

    spad = torch.zeros((cnt, K + 7), dtype=s.dtype, device=s.device)
    spad[:, :K] = s
    for f in (colmajor, padded, batch_last):
        got = rc.lowrank_recompress_large_batched_complex(f(left), f(right), k, 1e-6, mid=f(mid), s=spad)
        for v, w in zip(ref, got):
            assert np.array_equal(v, npy(w)), f.__name__
    shared = right[2:3].expand(cnt, K, n)  # right_batch_stride = 0
    assert shared.stride(0) == 0
    got = rc.lowrank_recompress_large_batched_complex(left, shared, k, 1e-6, mid=mid, s=s)
    one = rc.lowrank_recompress_large_batched_complex(left[2:3], right[2:3], k, 1e-6, mid=mid[2:3], s=s[2:3])
    for v, w, x in zip(ref, got, one):
        assert np.array_equal(v[2], npy(w)[2]) and np.array_equal(v[2], npy(x)[0])


def test_strided_outputs_leave_the_gaps_untouched():
    rng = np.random.default_rng(63)
    cnt, m, n, K, k = 4, 700, 1100, 14, 10
    left, right, mid, s = (cuda(x) for x in stack([factors(rng, "gauss", m, n, K, "mid", C64) for _ in range(cnt)]))
    # ranks below k in two blocks, so that zero columns and rows are written through the strided views too
    in_ranks = cuda(np.array([K, 4, K, 7], dtype=np.int64))
    ref = tuple(npy(x) for x in rc.lowrank_recompress_large_batched_complex(left, right, k, 1e-3, mid=mid, ranks=in_ranks))
    ut = torch.full((cnt, k, m + 1), 7.0, dtype=left.dtype, device=left.device)   # u column-major, padded
    vtt = torch.full((cnt, n, k + 2), 7.0, dtype=left.dtype, device=left.device)  # vt column-major, padded
    s_out = torch.zeros((cnt, K), dtype=torch.float64, device=left.device)
    ranks = torch.zeros(cnt, dtype=torch.int64, device=left.device)
    uv = _lib.rc_matrix(ut.data_ptr(), m, k, 1, m + 1)
    vv = _lib.rc_matrix(vtt.data_ptr(), k, n, 1, k + 2)
    assert _raw(left, mid, None, right, in_ranks, cnt, k, 1e-3, uv, k * (m + 1), s_out, vv, n * (k + 2), ranks) == 0
    torch.cuda.synchronize()
    assert np.array_equal(npy(ut)[:, :, :m].transpose(0, 2, 1), ref[0])
    assert np.array_equal(npy(vtt)[:, :, :k].transpose(0, 2, 1), ref[2])
    assert np.all(npy(ut)[:, :, m:] == 7.0) and np.all(npy(vtt)[:, :, k:] == 7.0)
    assert np.array_equal(npy(s_out), ref[1]) and np.array_equal(npy(ranks), ref[3])
    # both row-major with padded rows: the chunks of a column of u are written and re-read for the phase through the row stride, the chunks of
    # a row of vt are written through the column stride, each next to an untouched gap
    up = torch.full((cnt, m, k + 3), 7.0, dtype=left.dtype, device=left.device)
    vp = torch.full((cnt, k, n + 3), 7.0, dtype=left.dtype, device=left.device)
    assert _raw(left, mid, None, right, in_ranks, cnt, k, 1e-3, _lib.rc_matrix(up.data_ptr(), m, k, k + 3, 1), m * (k + 3), s_out,
                _lib.rc_matrix(vp.data_ptr(), k, n, n + 3, 1), k * (n + 3), ranks) == 0
    torch.cuda.synchronize()
    assert np.array_equal(npy(up)[:, :, :k], ref[0]) and np.all(npy(up)[:, :, k:] == 7.0)
    assert np.array_equal(npy(vp)[:, :, :n], ref[2]) and np.all(npy(vp)[:, :, n:] == 7.0)


def test_graph_capture_replays_the_eager_bits():
    rng = np.random.default_rng(64)
    cnt, m, n, K, k = 6, 600, 700, 24, 16
    lib = _lib.lib()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        left, right, mid, s = (cuda(x) for x in stack([factors(rng, "gauss", m, n, K, "both", C64) for _ in range(cnt)]))
        in_ranks = cuda(rng.integers(0, K + 1, cnt).astype(np.int64))
        eager = tuple(npy(x) for x in rc.lowrank_recompress_large_batched_complex(left, right, k, 1e-9, mid=mid, s=s, ranks=in_ranks))
        ctx = _lib.Context(torch.cuda.current_device(), st.cuda_stream)
        u = torch.zeros((cnt, m, k), dtype=left.dtype, device=left.device)
        s_out = torch.zeros((cnt, K), dtype=torch.float64, device=left.device)
        vt = torch.zeros((cnt, k, n), dtype=left.dtype, device=left.device)
        ranks = torch.zeros(cnt, dtype=torch.int64, device=left.device)
        st.synchronize()
        args = (left, mid, s, right, in_ranks, cnt, k, 1e-9, _lib.mat(u[0]), m * k, s_out, _lib.mat(vt[0]), k * n, ranks)
        assert _raw(*args, ctx=ctx) == 0  # eager once: sizes the workspace
        ctx.synchronize()
        ctx.get_health()
        for t in (u, s_out, vt, ranks):
            t.zero_()
        st.synchronize()
        graph = ctypes.c_void_p(None)
        ctx.check(lib.rc_graph_begin_capture(ctx._h))
        assert _raw(*args, ctx=ctx) == 0
        ctx.check(lib.rc_graph_end_capture(ctx._h, ctypes.byref(graph)))
        try:
            ctx.check(lib.rc_graph_launch(ctx._h, graph))
            ctx.synchronize()
            for v, w in zip(eager, (u, s_out, vt, ranks)):
                assert np.array_equal(v, npy(w))
            assert ctx.get_health() == 0
        finally:
            ctx.check(lib.rc_graph_destroy(ctx._h, graph))
            ctx.close()


def test_count_zero_is_a_no_op():
    e = lambda *shape: torch.zeros(shape, dtype=torch.complex64, device="cuda")  # noqa: E731
    u, s, vt, r = rc.lowrank_recompress_large_batched_complex(e(0, 600, 8), e(0, 8, 700), 5)
    assert u.shape == (0, 600, 5) and s.shape == (0, 8) and vt.shape == (0, 5, 700) and r.shape == (0,)
    assert u.dtype == torch.complex64 and s.dtype == torch.float32


@pytest.mark.parametrize("dtype", DTYPES)
def test_nan_stays_in_its_block(dtype):
    rng = np.random.default_rng(71)
    cnt, m, n, K, k = 6, 600, 700, 30, 20
    left, right, mid, s = stack([factors(rng, "gauss", m, n, K, "both", dtype) for _ in range(cnt)])
    ref = recompress_large(left, right, k, 1e-5, mid, s)
    left, right, mid, s = left.copy(), right.copy(), mid.copy(), s.copy()
    left[4, 590, 3] = np.nan  # in the second stage's rows
    right[1, 5, 690] = np.inf  # in the right factor's second stage
    mid[2, 1, 1] = complex(0.0, np.nan)
    got = recompress_large(left, right, k, 1e-5, mid, s)
    for i in range(cnt):
        assert 0 <= got[3][i] <= k
        if i in (1, 2, 4):
            continue
        for v, w in zip(ref, got):
            assert np.array_equal(v[i], w[i])
    _lib.default_context().get_health()  # whatever the bad blocks raised


@pytest.mark.parametrize("dtype", DTYPES)
def test_clean_inputs_leave_the_health_word_clear(dtype):
    rng = np.random.default_rng(81)
    ctx = _lib.default_context()
    ctx.synchronize()
    ctx.get_health()
    m, n, K = 600, 1100, 128
    rd = real_of(dtype)
    blocks = [factors(rng, kind, m, n, K, "both", dtype) for kind in KINDS]
    clustered = np.concatenate([np.ones(10), 0.5 * np.ones(40), 1e-3 * (1 + 1e-9 * np.arange(78))])
    blocks.append((orthonormal(rng, m, K).astype(dtype), orthonormal(rng, n, K).conj().T.astype(dtype), np.eye(K, dtype=dtype), clustered.astype(rd)))
    left, right, mid, s = stack(blocks)
    u, s_out, vt, ranks = recompress_large(left, right, 64, 0.0, mid, s)
    ctx.synchronize()
    assert ctx.get_health() == 0
    for i, b in enumerate(blocks):
        a, sigma = dense(*b, K)
        assert ranks[i] == 64
        check_block(a, sigma, u[i], s_out[i], vt[i], 64, K, 64, dtype)


# ---------------------------------------------------------------- 12. the label
@pytest.mark.parametrize("m,n,K", [(513, 600, 8), (1100, 130, 128), (300, 2100, 64), (300, 64, 16)])
def test_label_shows_the_stages_of_both_sides(m, n, K):
    rng = np.random.default_rng(m + n)
    blocks = [factors(rng, "gauss", m, n, K, "s", C32) for _ in range(3)]
    left, right, mid, s = stack(blocks)
    _, lab = batched_launch(lambda: recompress_large(left, right, K, 0.0, mid, s))
    assert lab["op"] == OP and (lab["m"], lab["n"], lab["k"], lab["count"], lab["grid"]) == (m, n, K, 3, 3)
    fields = lab["plan"].split(",")
    assert fields[0] == f"stages={stages(m, K)}" and fields[1] == f"rstages={stages(n, K)}", lab["plan"]
    assert fields[2] == ("L:ws" if m > H else fields[2]) and fields[3] == ("R:ws" if n > H else fields[3])
    assert [f[:2] for f in fields[2:6]] == ["L:", "R:", "V:", "G:"] and fields[-1] == "s" and f"kk={K}" in fields
    # the 2 GiB bound on the workspace does not bind at these sizes: the family's grid rule stands
    sl, sr, slot, grid = (ctypes.c_int64(0) for _ in range(4))
    assert _lib.lib().rc_lowrank_recompress_complex_large_batched_plan(ctypes.c_int64(m), ctypes.c_int64(n), ctypes.c_int64(K), ctypes.c_int32(4),
                                                                     ctypes.c_int64(lab["slots"]), ctypes.byref(sl), ctypes.byref(sr),
                                                                     ctypes.byref(slot), ctypes.byref(grid)) == 0
    assert (sl.value, sr.value) == (stages(m, K), stages(n, K)) and grid.value == lab["slots"]
    if n <= H:  # one stage on the right: the tall complex call's plan
        _, old = batched_launch(lambda: tuple(npy(x) for x in rc.lowrank_recompress_tall_batched_complex(cuda(left), cuda(right), K, 0.0, s=cuda(s))))
        assert lab["plan"] == old["plan"].replace(",", ",rstages=1,", 1)


# ---------------------------------------------------------------- 13. the arguments
def test_argument_checks():
    e = lambda c, r, q: torch.zeros((c, r, q), dtype=torch.complex128, device="cuda")  # noqa: E731
    sbuf = torch.zeros((2, 600), dtype=torch.float64, device="cuda")
    ranks = torch.zeros(2, dtype=torch.int64, device="cuda")

    def call(left, right, k, tol, u, ubs, vt, vbs, mid=None, cnt=2, s_out=sbuf, rk=ranks):
        return _raw(left, mid, None, right, None, cnt, k, tol, _lib.mat(u[0]) if u is not None else _lib.mat(None), ubs, s_out,
                    _lib.mat(vt[0]) if vt is not None else _lib.mat(None), vbs, rk)

    def message():
        return _lib.lib().rc_last_error_message(_lib.default_context()._h).decode()

    lf, rt, u, vt = e(2, 700, 16), e(2, 16, 900), e(2, 700, 8), e(2, 8, 900)
    assert call(lf, rt, 8, 0.0, u, 5600, vt, 7200) == 0                                            # the valid call the rest departs from
    assert call(lf, e(2, 16, 513), 8, 0.0, u, 5600, e(2, 8, 513), 4104) == 0                       # n = 513: the first column past the tall call
    big = torch.zeros((1, 65537, 16), dtype=torch.complex128, device="cuda")
    ubig = torch.zeros((1, 65537, 8), dtype=torch.complex128, device="cuda")
    assert call(big[:, :65536], rt[:1], 8, 0.0, ubig[:, :65536], 65536 * 8, vt[:1], 7200, cnt=1) == 0      # m = 65536
    assert call(big, rt[:1], 8, 0.0, ubig, 65537 * 8, vt[:1], 7200, cnt=1) == INVALID             # m = 65537
    assert message().startswith(NAME) and "65536" in message()
    wide, vwide = big.mT, ubig.mT                                                                  # 16 x 65537 and 8 x 65537 views
    assert call(lf[:1], wide[:, :, :65536], 8, 0.0, u[:1], 5600, vwide[:, :, :65536], 65537 * 8, cnt=1) == 0  # n = 65536
    assert call(lf[:1], wide, 8, 0.0, u[:1], 5600, vwide, 65537 * 8, cnt=1) == INVALID            # n = 65537
    assert message().startswith(NAME) and "65536" in message()
    assert call(e(2, 700, 129), e(2, 129, 900), 8, 0.0, u, 5600, vt, 7200) == INVALID             # K = 129
    assert message().startswith(NAME)
    assert call(lf, e(2, 16, 12), 8, 0.0, u, 5600, e(2, 8, 12), 96) == INVALID                     # K > min(m, n)
    assert message().startswith(NAME) and "rc_svd_rank_batched" in message()
    assert call(e(2, 12, 16), rt, 8, 0.0, e(2, 12, 8), 96, vt, 7200) == INVALID
    assert call(lf, e(2, 15, 900), 8, 0.0, u, 5600, vt, 7200) == INVALID                          # left.cols != right.rows
    assert message().startswith(NAME)
    assert call(lf, rt, 8, 0.0, u, 5600, vt, 7200, mid=e(2, 16, 15)) == INVALID                   # mid not K x K
    assert message().startswith(NAME)
    assert call(lf, rt, 0, 0.0, e(2, 700, 1), 700, e(2, 1, 900), 900) == INVALID                  # k < 1
    assert call(lf, rt, 8, 1.0, u, 5600, vt, 7200) == INVALID                                     # tol = 1
    assert call(lf, rt, 8, -1e-3, u, 5600, vt, 7200) == INVALID                                   # tol < 0
    assert call(lf, rt, 8, 0.0, u, 5599, vt, 7200) == INVALID                                     # a short batch stride of u
    assert message().startswith(NAME)
    assert call(lf, rt, 8, 0.0, u, 5600, vt, 7199) == INVALID                                     # and of vt
    assert call(lf, rt, 8, 0.0, e(2, 700, 7), 4900, vt, 7200) == INVALID                          # u not m x kk
    assert message().startswith(NAME)
    assert call(lf, rt, 8, 0.0, e(2, 699, 8), 5592, vt, 7200) == INVALID
    assert call(lf, rt, 8, 0.0, u, 5600, e(2, 8, 899), 7192) == INVALID                           # vt not kk x n
    assert call(lf, rt, 8, 0.0, u, 5600, e(2, 7, 900), 6300) == INVALID
    assert call(lf, rt, 8, 0.0, u, 5600, vt, 7200, cnt=-1) == INVALID                             # count < 0
    assert message().startswith(NAME)
    assert call(lf, rt, 8, 0.0, u, 5600, vt, 7200, s_out=None) == INVALID                         # null outputs
    assert message().startswith(NAME)
    assert call(lf, rt, 8, 0.0, u, 5600, vt, 7200, rk=None) == INVALID
    assert call(lf, rt, 8, 0.0, None, 5600, vt, 7200) == INVALID
    assert call(lf, rt, 8, 0.0, u, 5600, None, 7200) == INVALID
    assert call(lf, rt, 8, 0.0, u, 5600, vt, 7200, cnt=0) == 0                                    # count = 0: nothing to do
    # the c32 entry point takes its tol as a float
    c32 = lambda c, r, q: torch.zeros((c, r, q), dtype=torch.complex64, device="cuda")  # noqa: E731
    s32 = torch.zeros((2, 16), dtype=torch.float32, device="cuda")
    args32 = (c32(2, 700, 16), None, None, c32(2, 16, 900), None, 2, 8)
    outs32 = (_lib.mat(c32(2, 700, 8)[0]), 5600, s32, _lib.mat(c32(2, 8, 900)[0]), 7200, ranks)
    assert _raw(*args32, 0.5, *outs32, dtype=torch.complex64) == 0
    assert _raw(*args32, 1.0, *outs32, dtype=torch.complex64) == INVALID
    torch.cuda.synchronize()
    # the real large name keeps refusing complex data; the complex names refuse real data and mixed dtypes
    for bad in (torch.complex128, torch.complex64):
        with pytest.raises(TypeError, match="lowrank_recompress_large_batched"):
            rc.lowrank_recompress_large_batched(torch.zeros((1, 600, 4), dtype=bad, device="cuda"), torch.zeros((1, 4, 700), dtype=bad, device="cuda"), 2)
    for bad in (torch.float64, torch.float32):
        z = lambda *shape: torch.zeros(shape, dtype=bad, device="cuda")  # noqa: E731
        with pytest.raises(TypeError, match="lowrank_recompress_large_batched_complex"):
            rc.lowrank_recompress_large_batched_complex(z(1, 600, 4), z(1, 4, 700), 2)
        with pytest.raises(TypeError):
            rc.svd_add_large_batched_complex(*[z(1, 600, 2), z(1, 2), z(1, 2, 700)] * 2, 2)
    with pytest.raises(TypeError):
        rc.lowrank_recompress_large_batched_complex(e(1, 600, 4), e(1, 4, 700).to(torch.complex64), 2)                  # mixed complex dtypes
    with pytest.raises(TypeError):
        rc.lowrank_recompress_large_batched_complex(e(1, 600, 4), e(1, 4, 700), 2, s=torch.zeros((1, 4), dtype=torch.complex128, device="cuda"))
    with pytest.raises(AssertionError, match=NAME):  # RC_INVALID_ARGUMENT: the reference asserts
        rc.lowrank_recompress_large_batched_complex(e(1, 600, 16), e(1, 16, 12), 4)
    # the existing entry points keep their domains
    with pytest.raises(AssertionError, match="lowrank_recompress_tall_complex_batched"):
        rc.lowrank_recompress_tall_batched_complex(e(1, 600, 16), e(1, 16, 513), 4)
    with pytest.raises(AssertionError, match="lowrank_recompress_large_batched"):
        rc.lowrank_recompress_large_batched(e(1, 600, 16).real.contiguous(), e(1, 16, 12).real.contiguous(), 4)
