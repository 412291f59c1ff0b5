"""Batched recompression of factor pairs with both factors tall (rc_lowrank_recompress_large_batched_*, batch.lowrank_recompress_large_batched and
its wrapper svd_add_large_batched).

The oracle, the bounds and the block generators are those of tests/test_gpu_batched_recompress.py (check_block: 4 TOL sigma with sigma the
product of the factors' 2-norms).  For n > 512 the right factor goes, as right^T, through exactly the flat Householder TSQR the left factor
goes through in tests/test_gpu_batched_recompress_tall.py (stages of H = 512 rows; stage 0 holds rows 0 .. 511 and every later stage the next
512 - q rows, so the stage edges of a side of length x are at x = 512 + j (512 - q)); the numpy model of that scheme quoted there, which
stayed 9-400x inside these bounds, therefore covers both sides.  For n <= 512 the call is the tall call bit for bit.

A dense reference SVD is the cost of a case, so no side goes above about 2100; the one block with n = 65536 is checked from thin QRs of its
factors in f64 (check_from_factors), never formed."""
import ctypes

import numpy as np
import pytest
import torch

import rusty_compression_amd as rc
from rusty_compression_amd import _lib
from tests.helpers import TOL, batched_launch, npy, sign_normalise
from tests.test_gpu_batched_recompress import check_block, clamp, dense, factors, stack
from tests.test_gpu_batched_svd import check_signs, check_vectors

pytestmark = pytest.mark.gpu

INVALID = 5
H = 512
MODES = ("none", "mid", "s", "both")
DTYPES = [np.float64, np.float32]
KINDS = ("gauss", "spectrum", "scaled")


def cuda(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def recompress_large(left, right, k, tol=0.0, mid=None, s=None, ranks=None):
    out = rc.lowrank_recompress_large_batched(cuda(left), cuda(right), k, tol, mid=cuda(mid), s=cuda(s), ranks=cuda(ranks))
    torch.cuda.synchronize()
    return tuple(npy(t) for t in out)


def stages(x, q):
    return 1 if x <= H else 1 + -(-(x - H) // (H - q))


def orthonormal(rng, rows, cols):
    return np.linalg.qr(rng.standard_normal((rows, cols)))[0]


def check_from_factors(left, right, mid, s, q, u, s_out, vt, r, kk, dtype):
    """check_block's checks for a block too large to form: the reference SVD from thin QRs of the factors in f64 (left = Ql Rl, right^T = Qr Rr,
    the SVD of Rl core Rr^T), and ||A - U S Vt||_2 as the 2-norm of [left_q, U] [core right_q; -S Vt], again through thin QRs.  Returns the
    reference (u, s, vt) at full inner rank q."""
    t = TOL[np.dtype(dtype)]
    lf, rt = left[:, :q].astype(np.float64), right[:q].astype(np.float64)
    core = np.eye(q) if mid is None else mid[:q, :q].astype(np.float64)
    if s is not None:
        core = core * s[:q].astype(np.float64)[None, :]
    ql, rl = np.linalg.qr(lf)
    qr, rr = np.linalg.qr(rt.T)
    sigma = float(np.linalg.norm(rl, 2) * np.linalg.norm(core, 2) * np.linalg.norm(rr, 2))
    uc, sref, vct = np.linalg.svd(rl @ core @ rr.T)
    ref_u, ref_vt = ql @ uc, vct @ qr.T
    assert 0 <= r <= min(kk, q)
    assert not np.any(s_out[q:])
    sv = s_out[:q].astype(np.float64)
    assert np.all(np.diff(sv) <= 0)
    err_s = np.abs(sv - sref).max()
    print(f"    sval err {err_s:.3e} bound {4 * t['sval'] * sigma:.3e}")
    assert err_s <= 4 * t["sval"] * sigma, (err_s, sigma)
    assert not np.any(u[:, r:]) and not np.any(vt[r:])
    ur, vr = u[:, :r].astype(np.float64), vt[:r].astype(np.float64)
    orth_u, orth_v = np.abs(ur.T @ ur - np.eye(r)).max(), np.abs(vr @ vr.T - np.eye(r)).max()
    q1, r1 = np.linalg.qr(np.concatenate([lf, ur], axis=1))
    q2, r2 = np.linalg.qr(np.concatenate([core @ rt, -(sv[:r, None] * vr)], axis=0).T)
    err = np.linalg.norm(r1 @ r2.T, 2)
    tail = sref[r] if r < q else 0.0
    print(f"    orth u {orth_u:.3e} vt {orth_v:.3e} bound {4 * t['orth']:.3e}; recon {err:.3e} tail {tail:.3e} bound {4 * t['recon'] * sigma:.3e}")
    assert max(orth_u, orth_v) <= 4 * t["orth"]
    assert err <= 4 * t["recon"] * sigma + tail, (err, tail, sigma)
    check_signs(u, vt, r)
    return ref_u, sref, ref_vt


def report(tag, a, sigma, u, s_out, vt, ref, r, dtype):
    """The block's ratios to the family's bounds (singular values, orthonormality of u and of vt, reconstruction), one line."""
    t = TOL[np.dtype(dtype)]
    sv, ur, vr = s_out[:r].astype(np.float64), u[:, :r].astype(np.float64), vt[:r].astype(np.float64)
    rs = np.abs(s_out[:len(ref.s)].astype(np.float64) - ref.s[:len(s_out)]).max() / (4 * t["sval"] * sigma)
    ru = np.abs(ur.T @ ur - np.eye(r)).max() / (4 * t["orth"])
    rv = np.abs(vr @ vr.T - np.eye(r)).max() / (4 * t["orth"])
    rr = max(np.linalg.norm(a - (ur * sv) @ vr, 2) - (ref.s[r] if r < len(ref.s) else 0.0), 0.0) / (4 * t["recon"] * sigma)
    print(f"  RATIO {tag} sval {rs:.4f} orth_u {ru:.4f} orth_vt {rv:.4f} recon {rr:.4f}")


# ---------------------------------------------------------------- 1. n <= 512: the bits of the existing calls
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m,n,K", [(64, 64, 40), (512, 512, 128), (513, 130, 128), (2100, 64, 64), (1500, 512, 40)])
def test_up_to_512_columns_the_bits_are_the_tall_calls(m, n, K, dtype):
    rng = np.random.default_rng(100 + m + n)
    qs = np.array([K, K // 2, 0, K + 3, K - 1], dtype=np.int64)
    k = max(1, (2 * K) // 3)
    ran = 0
    for mode in MODES:
        left, right, mid, s = (cuda(x) for x in stack([factors(rng, "gauss", m, n, K, mode, dtype) for _ in qs]))
        for tol in (0.0, 1e-3):
            for ranks in (None, cuda(qs)):
                want = rc.lowrank_recompress_tall_batched(left, right, k, tol, mid=mid, s=s, ranks=ranks)
                got = rc.lowrank_recompress_large_batched(left, right, k, tol, mid=mid, s=s, ranks=ranks)
                for name, v, w in zip(("u", "s_out", "vt", "ranks"), want, got):
                    assert torch.equal(v, w), (m, n, K, mode, tol, name)
                if m <= H:
                    base = rc.lowrank_recompress_batched(left, right, k, tol, mid=mid, s=s, ranks=ranks)
                    for name, v, w in zip(("u", "s_out", "vt", "ranks"), base, want):
                        assert torch.equal(v, w), (m, n, K, mode, tol, name, "base")
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
            own = check_vectors(*sign_normalise(ref.u[:, :K], ref.vt[:K]), ref.u, ref.vt, ref.s, K, dtype)
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
    assert lab["op"] == "batched_recompress_large" and lab["plan"].startswith("stages=2,rstages=131,L:ws,R:ws,")
    assert ranks[0] == K and vt.shape == (1, K, n)
    ref_u, ref_s, ref_vt = check_from_factors(b[0], b[1], b[2], b[3], K, u[0], s_out[0], vt[0], K, K, dtype)
    assert check_vectors(u[0], vt[0], ref_u, ref_vt, ref_s, K, dtype) >= 3
    assert np.all(np.abs(vt[0][:, -1]) > 0)  # the last column is written


# ---------------------------------------------------------------- 4. the inner rank sets the stage height on both sides
@pytest.mark.parametrize("dtype", DTYPES)
def test_in_ranks_give_the_truncated_calls_bits_and_tails_are_never_read(dtype):
    rng = np.random.default_rng(31)
    m, n, K, k = 1100, 1100, 64, 40
    qs = np.array([1, 17, 64], dtype=np.int64)
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
        tl, tr, tm, ts = blocks[i]
        check_from_factors(tl, tr, tm, ts, q, u[i], s_out[i], vt[i], int(ranks[i]), k, dtype)
        # the truncated factors as a call of their own (inner width q): the same bits
        tu, tsv, tvt, trk = recompress_large(tl[None, :, :q], tr[None, :q], k, 0.0, tm[None, :q, :q], ts[None, :q])
        r = int(ranks[i])
        assert trk[0] == r
        assert np.array_equal(tsv[0], s_out[i][:q]) and np.array_equal(tu[0][:, :r], u[i][:, :r]) and np.array_equal(tvt[0][:r], vt[i][:r])


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_stage_counts_differ_across_inner_ranks_of_one_batch(dtype):
    """1534 = 512 + 2 * 511: q = 1 fills exactly three stages, q = 64 needs a fourth; n = 1470 keeps q = 1 and q = 17 at three stages
    (512 + 2 * 495 = 1502) and gives q = 64 four: the stage counts differ across the batch on both sides, and not in the same blocks."""
    rng = np.random.default_rng(32)
    m, n, K = 1534, 1470, 64
    qs = np.array([1, 17, 64, 0, -2, 70], dtype=np.int64)
    assert [stages(m, q) for q in (1, 17, 64)] == [3, 4, 4] and [stages(n, q) for q in (1, 17, 64)] == [3, 3, 4]
    blocks = [factors(rng, "gauss", m, n, K, "s", dtype) for _ in qs]
    left, right, mid, s = stack(blocks)
    u, s_out, vt, ranks = recompress_large(left, right, K, 0.0, mid, s, qs)
    for i, q in enumerate(qs):
        q = clamp(q, K)
        assert ranks[i] == q
        if q == 0:
            assert not np.any(u[i]) and not np.any(vt[i]) and not np.any(s_out[i])
            continue
        check_from_factors(*blocks[i], q, u[i], s_out[i], vt[i], q, K, dtype)


# ---------------------------------------------------------------- 5. exact zeros and rank deficiency
@pytest.mark.parametrize("dtype", DTYPES)
def test_zero_columns_of_left_give_exactly_zero_singular_values(dtype):
    rng = np.random.default_rng(42)
    m, n, K = 700, 900, 24
    for mode in MODES:
        zl, zr, zm, zs = factors(rng, "gauss", m, n, K, mode, dtype)
        zl[:, [3, 7, 20]] = 0                  # zero in every stage
        pl, pr, pm, ps = factors(rng, "gauss", m, n, K, mode, dtype)
        pl[H:, 5] = 0                          # zero only below the first stage: not a zero column
        blocks = [(zl, zr, zm, zs), (pl, pr, pm, ps)]
        left, right, mid, s = stack(blocks)
        u, s_out, vt, ranks = recompress_large(left, right, K, 0.0, mid, s)
        assert np.all(s_out[0][:21] > 0) and not np.any(s_out[0][21:]), (mode, s_out[0])
        assert np.all(s_out[1] > 0), (mode, s_out[1])
        assert list(ranks) == [21, 24]
        for i in range(2):
            a, sigma = dense(*blocks[i], K)
            check_block(a, sigma, u[i], s_out[i], vt[i], int(ranks[i]), K, K, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_svd_add_of_a_block_with_itself(dtype):
    """x + x through the rank-deficient factors [U U], [Vt; Vt] truncated to k: rank k, the singular values are 2 s, the other k are rounding of
    sigma.  ranks1 / ranks2 cut the addends: NaN past them is not seen."""
    rng = np.random.default_rng(43)
    cnt, m, n, k = 3, 900, 700, 12
    t = TOL[np.dtype(dtype)]
    u0 = np.stack([orthonormal(rng, m, k) for _ in range(cnt)]).astype(dtype)
    vt0 = np.stack([orthonormal(rng, n, k).T for _ in range(cnt)]).astype(dtype)
    s0 = np.stack([np.sort(rng.uniform(0.5, 2.0, k))[::-1] for _ in range(cnt)]).astype(dtype)
    u, s_out, vt, ranks = (npy(x) for x in rc.svd_add_large_batched(cuda(u0), cuda(s0), cuda(vt0), cuda(u0), cuda(s0), cuda(vt0), k, 0.0))
    torch.cuda.synchronize()
    assert s_out.shape == (cnt, 2 * k) and u.shape == (cnt, m, k) and vt.shape == (cnt, k, n)
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
        un[i][:, r1[i]:], sn[i][r1[i]:], vn[i][r1[i]:] = np.nan, np.nan, np.nan
        u2[i][:, r2[i]:], s2[i][r2[i]:], v2[i][r2[i]:] = np.nan, np.nan, np.nan
    cu, cs, cv, cr = (npy(x) for x in rc.svd_add_large_batched(cuda(un), cuda(sn), cuda(vn), cuda(u2), cuda(s2), cuda(v2), k, 0.0, ranks1=cuda(r1),
                                                               ranks2=cuda(r2)))
    torch.cuda.synchronize()
    for i in range(cnt):
        assert cr[i] == max(r1[i], r2[i])  # the addends share their leading triplets, so the sum has the larger rank
        w = np.zeros(k)
        w[:r1[i]] += s0[i][:r1[i]].astype(np.float64)
        w[:r2[i]] += s0[i][:r2[i]].astype(np.float64)
        a = (u0[i].astype(np.float64) * w) @ vt0[i].astype(np.float64)
        check_block(a, 2.0 * float(s0[i][0]), cu[i], cs[i], cv[i], int(cr[i]), 2 * k, k, dtype)


# ---------------------------------------------------------------- 6. signs
@pytest.mark.parametrize("dtype", DTYPES)
def test_sign_rule_over_chunks_with_the_right_factor_in_three_stages(dtype):
    """K = 3, m = n = 1100: u's chunks of rows are [0, 512), [512, 1021), [1021, 1100) and the right factor has three stages as well.  u's first
    column is, up to sign, the first column of left, which carries one dominant entry of either sign in a chosen chunk (1090 and 1021: the
    last one).  vt takes u's signs: sign-normalising the oracle's pair by its u reproduces the signs of vt's rows."""
    rng = np.random.default_rng(51)
    m, n, K = 1100, 1100, 3
    assert stages(m, K) == 3 and stages(n, K) == 3
    blocks, rows = [], []
    for row in (1090, 5, 700, 1021, 511):
        for sign in (1.0, -1.0):
            spike = 0.01 * rng.standard_normal(m)
            spike[row] = sign
            q1 = np.linalg.qr(np.column_stack([spike, rng.standard_normal((m, K - 1))]))[0]
            blocks.append((q1.astype(dtype), orthonormal(rng, n, K).T.astype(dtype), None, np.array([4.0, 2.0, 1.0], dtype=dtype)))
            rows.append(row)
    left, right, mid, s = stack(blocks)
    u, s_out, vt, ranks = recompress_large(left, right, K, 0.0, mid, s)
    for i, row in enumerate(rows):
        assert ranks[i] == K
        assert int(np.argmax(np.abs(u[i][:, 0]))) == row and u[i][row, 0] > 0, (i, row)
        check_signs(u[i], vt[i], K)
        ref_u, ref_s, ref_vt = check_from_factors(*blocks[i], K, u[i], s_out[i], vt[i], K, K, dtype)
        nu, nvt = sign_normalise(ref_u, ref_vt)
        for j in range(K):  # gaps of 1/4 of s_0: the vectors are determined
            assert float(np.dot(nvt[j], vt[i][j].astype(np.float64))) > 0.99, (i, j)
            assert float(np.dot(nu[:, j], u[i][:, j].astype(np.float64))) > 0.99, (i, j)
        assert check_vectors(u[i], vt[i], ref_u, ref_vt, ref_s, K, dtype) >= 1


# ---------------------------------------------------------------- 7. the batch contract
def _view(t):
    if t is None:
        return _lib.mat(None), ctypes.c_int64(0)
    return _lib.rc_matrix(t.data_ptr(), t.shape[1], t.shape[2], t.stride(1), t.stride(2)), ctypes.c_int64(t.stride(0))


def _raw(left, mid, s, right, in_ranks, cnt, k, tol, u, ubs, s_out, vt, vbs, ranks, ctx=None, dtype=torch.float64):
    ctx = ctx or _lib.default_context()
    fn = getattr(_lib.lib(), f"rc_lowrank_recompress_large_batched_{_lib.suffix(dtype)}")
    return fn(ctx._h, *_view(left), *_view(mid), ctypes.c_void_p(s.data_ptr() if s is not None else None),
              ctypes.c_int64(s.stride(0) if s is not None else 0), *_view(right), _lib.i64p(in_ranks), ctypes.c_int32(cnt), ctypes.c_int64(k),
              ctypes.c_double(tol), u, ctypes.c_int64(ubs), ctypes.c_void_p(s_out.data_ptr() if s_out is not None else None), vt, ctypes.c_int64(vbs),
              _lib.i64p(ranks))


def test_bits_independent_of_count_position_and_neighbours():
    rng = np.random.default_rng(61)
    m, n, K, k, tol = 513, 513, 8, 6, 1e-9
    protos = [factors(rng, kind, m, n, K, "both", np.float64) for kind in ("gauss", "spectrum", "scaled", "gauss", "gauss", "scaled", "gauss")]
    qs = [K, K, 5, 0, 1, K + 2, 3]
    alone = []
    labels = None
    for b, q in zip(protos, qs):
        out, labels = batched_launch(lambda: recompress_large(b[0][None], b[1][None], k, tol, b[2][None], b[3][None], np.array([q], dtype=np.int64)))
        alone.append(out)
    assert labels["op"] == "batched_recompress_large" and (labels["m"], labels["n"], labels["k"], labels["count"], labels["grid"]) == (m, n, K, 1, 1)
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
    ref = tuple(npy(x) for x in rc.lowrank_recompress_large_batched(left, right, k, 1e-6, mid=mid, s=s))

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
        got = rc.lowrank_recompress_large_batched(f(left), f(right), k, 1e-6, mid=f(mid), s=spad)
        for v, w in zip(ref, got):
            assert np.array_equal(v, npy(w)), f.__name__
    shared = right[2:3].expand(cnt, K, n)  # right_batch_stride = 0
    assert shared.stride(0) == 0
    got = rc.lowrank_recompress_large_batched(left, shared, k, 1e-6, mid=mid, s=s)
    one = rc.lowrank_recompress_large_batched(left[2:3], right[2:3], k, 1e-6, mid=mid[2:3], s=s[2:3])
    for v, w, x in zip(ref, got, one):
        assert np.array_equal(v[2], npy(w)[2]) and np.array_equal(v[2], npy(x)[0])


def test_strided_outputs_leave_the_gaps_untouched():
    rng = np.random.default_rng(63)
    cnt, m, n, K, k = 4, 700, 1100, 14, 10
    left, right, mid, s = (cuda(x) for x in stack([factors(rng, "gauss", m, n, K, "mid", np.float64) for _ in range(cnt)]))
    # ranks below k in two blocks, so that zero columns and rows are written through the strided views too
    in_ranks = cuda(np.array([K, 4, K, 7], dtype=np.int64))
    ref = tuple(npy(x) for x in rc.lowrank_recompress_large_batched(left, right, k, 1e-3, mid=mid, ranks=in_ranks))
    ut = torch.full((cnt, k, m + 1), 7.0, dtype=left.dtype, device=left.device)   # u column-major, padded
    vtt = torch.full((cnt, n, k + 2), 7.0, dtype=left.dtype, device=left.device)  # vt column-major, padded
    s_out = torch.zeros((cnt, K), dtype=left.dtype, device=left.device)
    ranks = torch.zeros(cnt, dtype=torch.int64, device=left.device)
    uv = _lib.rc_matrix(ut.data_ptr(), m, k, 1, m + 1)
    vv = _lib.rc_matrix(vtt.data_ptr(), k, n, 1, k + 2)
    assert _raw(left, mid, None, right, in_ranks, cnt, k, 1e-3, uv, k * (m + 1), s_out, vv, n * (k + 2), ranks) == 0
    torch.cuda.synchronize()
    assert np.array_equal(npy(ut)[:, :, :m].transpose(0, 2, 1), ref[0])
    assert np.array_equal(npy(vtt)[:, :, :k].transpose(0, 2, 1), ref[2])
    assert np.all(npy(ut)[:, :, m:] == 7.0) and np.all(npy(vtt)[:, :, k:] == 7.0)
    assert np.array_equal(npy(s_out), ref[1]) and np.array_equal(npy(ranks), ref[3])
    # vt row-major with a padded row: the chunks of a row of vt are written through the column stride, next to an untouched gap
    u = torch.zeros((cnt, m, k), dtype=left.dtype, device=left.device)
    vp = torch.full((cnt, k, n + 3), 7.0, dtype=left.dtype, device=left.device)
    assert _raw(left, mid, None, right, in_ranks, cnt, k, 1e-3, _lib.mat(u[0]), m * k, s_out, _lib.rc_matrix(vp.data_ptr(), k, n, n + 3, 1), k * (n + 3),
                ranks) == 0
    torch.cuda.synchronize()
    assert np.array_equal(npy(vp)[:, :, :n], ref[2]) and np.all(npy(vp)[:, :, n:] == 7.0) and np.array_equal(npy(u), ref[0])


def test_graph_capture_replays_the_eager_bits():
    rng = np.random.default_rng(64)
    cnt, m, n, K, k = 6, 600, 700, 24, 16
    lib = _lib.lib()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        left, right, mid, s = (cuda(x) for x in stack([factors(rng, "gauss", m, n, K, "both", np.float64) for _ in range(cnt)]))
        in_ranks = cuda(rng.integers(0, K + 1, cnt).astype(np.int64))
        eager = tuple(npy(x) for x in rc.lowrank_recompress_large_batched(left, right, k, 1e-9, mid=mid, s=s, ranks=in_ranks))
        ctx = _lib.Context(torch.cuda.current_device(), st.cuda_stream)
        u = torch.zeros((cnt, m, k), dtype=left.dtype, device=left.device)
        s_out = torch.zeros((cnt, K), dtype=left.dtype, device=left.device)
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
    e = lambda *shape: torch.zeros(shape, dtype=torch.float32, device="cuda")  # noqa: E731
    u, s, vt, r = rc.lowrank_recompress_large_batched(e(0, 600, 8), e(0, 8, 700), 5)
    assert u.shape == (0, 600, 5) and s.shape == (0, 8) and vt.shape == (0, 5, 700) and r.shape == (0,)


@pytest.mark.parametrize("dtype", DTYPES)
def test_nan_stays_in_its_block(dtype):
    rng = np.random.default_rng(71)
    cnt, m, n, K, k = 6, 600, 700, 30, 20
    left, right, mid, s = stack([factors(rng, "gauss", m, n, K, "both", dtype) for _ in range(cnt)])
    ref = recompress_large(left, right, k, 1e-5, mid, s)
    left, right, mid, s = left.copy(), right.copy(), mid.copy(), s.copy()
    left[4, 590, 3] = np.nan  # in the second stage's rows
    right[1, 5, 690] = np.inf  # in the right factor's second stage
    mid[2, 1, 1] = np.nan
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
    blocks = [factors(rng, kind, m, n, K, "both", dtype) for kind in KINDS]
    clustered = np.concatenate([np.ones(10), 0.5 * np.ones(40), 1e-3 * (1 + 1e-9 * np.arange(78))])
    blocks.append((orthonormal(rng, m, K).astype(dtype), orthonormal(rng, n, K).T.astype(dtype), np.eye(K, dtype=dtype), clustered.astype(dtype)))
    left, right, mid, s = stack(blocks)
    u, s_out, vt, ranks = recompress_large(left, right, 64, 0.0, mid, s)
    ctx.synchronize()
    assert ctx.get_health() == 0
    for i, b in enumerate(blocks):
        a, sigma = dense(*b, K)
        assert ranks[i] == 64
        check_block(a, sigma, u[i], s_out[i], vt[i], 64, K, 64, dtype)


# ---------------------------------------------------------------- 8. the label
@pytest.mark.parametrize("m,n,K", [(513, 600, 8), (1100, 130, 128), (300, 2100, 64), (300, 64, 16)])
def test_label_shows_the_stages_of_both_sides(m, n, K):
    rng = np.random.default_rng(m + n)
    blocks = [factors(rng, "gauss", m, n, K, "s", np.float32) for _ in range(3)]
    left, right, mid, s = stack(blocks)
    _, lab = batched_launch(lambda: recompress_large(left, right, K, 0.0, mid, s))
    assert lab["op"] == "batched_recompress_large" and (lab["m"], lab["n"], lab["k"], lab["count"], lab["grid"]) == (m, n, K, 3, 3)
    fields = lab["plan"].split(",")
    assert fields[0] == f"stages={stages(m, K)}" and fields[1] == f"rstages={stages(n, K)}", lab["plan"]
    assert fields[2] == ("L:ws" if m > H else fields[2]) and fields[3] == ("R:ws" if n > H else fields[3])
    assert fields[2] in ("L:lds", "L:ws") and fields[3] in ("R:lds", "R:ws") and fields[-1] == "s" and f"kk={K}" in fields
    # the 2 GiB bound on the workspace does not bind at these sizes: the family's grid rule stands
    sl, sr, slot, grid = (ctypes.c_int64(0) for _ in range(4))
    assert _lib.lib().rc_lowrank_recompress_large_batched_plan(ctypes.c_int64(m), ctypes.c_int64(n), ctypes.c_int64(K), ctypes.c_int32(4),
                                                             ctypes.c_int64(lab["slots"]), ctypes.byref(sl), ctypes.byref(sr), ctypes.byref(slot),
                                                             ctypes.byref(grid)) == 0
    assert (sl.value, sr.value) == (stages(m, K), stages(n, K)) and grid.value == lab["slots"]


# ---------------------------------------------------------------- 9. the arguments
def test_argument_checks():
    e = lambda c, r, q: torch.zeros((c, r, q), dtype=torch.float64, device="cuda")  # noqa: E731
    sbuf = torch.zeros((2, 600), dtype=torch.float64, device="cuda")
    ranks = torch.zeros(2, dtype=torch.int64, device="cuda")

    def call(left, right, k, tol, u, ubs, vt, vbs, mid=None, cnt=2, s_out=sbuf, rk=ranks):
        return _raw(left, mid, None, right, None, cnt, k, tol, _lib.mat(u[0]) if u is not None else _lib.mat(None), ubs, s_out,
                    _lib.mat(vt[0]) if vt is not None else _lib.mat(None), vbs, rk)

    lf, rt, u, vt = e(2, 700, 16), e(2, 16, 900), e(2, 700, 8), e(2, 8, 900)
    assert call(lf, rt, 8, 0.0, u, 5600, vt, 7200) == 0                                            # the valid call the rest departs from
    assert call(lf, e(2, 16, 513), 8, 0.0, u, 5600, e(2, 8, 513), 4104) == 0                       # n = 513: the first column past the tall call
    big = torch.zeros((1, 65537, 16), dtype=torch.float64, device="cuda")
    ubig = torch.zeros((1, 65537, 8), dtype=torch.float64, device="cuda")
    assert call(big[:, :65536], rt[:1], 8, 0.0, ubig[:, :65536], 65536 * 8, vt[:1], 7200, cnt=1) == 0      # m = 65536
    assert call(big, rt[:1], 8, 0.0, ubig, 65537 * 8, vt[:1], 7200, cnt=1) == INVALID             # m = 65537
    msg = _lib.lib().rc_last_error_message(_lib.default_context()._h).decode()
    assert "lowrank_recompress_large_batched" in msg and "65536" in msg
    wide, vwide = big.mT, ubig.mT                                                                  # 16 x 65537 and 8 x 65537 views
    assert call(lf[:1], wide[:, :, :65536], 8, 0.0, u[:1], 5600, vwide[:, :, :65536], 65537 * 8, cnt=1) == 0  # n = 65536
    assert call(lf[:1], wide, 8, 0.0, u[:1], 5600, vwide, 65537 * 8, cnt=1) == INVALID            # n = 65537
    msg = _lib.lib().rc_last_error_message(_lib.default_context()._h).decode()
    assert "lowrank_recompress_large_batched" in msg and "65536" in msg
    assert call(e(2, 700, 129), e(2, 129, 900), 8, 0.0, u, 5600, vt, 7200) == INVALID             # K = 129
    assert call(lf, e(2, 16, 12), 8, 0.0, u, 5600, e(2, 8, 12), 96) == INVALID                     # K > min(m, n)
    assert call(e(2, 12, 16), rt, 8, 0.0, e(2, 12, 8), 96, vt, 7200) == INVALID
    assert call(lf, e(2, 15, 900), 8, 0.0, u, 5600, vt, 7200) == INVALID                          # left.cols != right.rows
    assert call(lf, rt, 8, 0.0, u, 5600, vt, 7200, mid=e(2, 16, 15)) == INVALID                   # mid not K x K
    assert call(lf, rt, 0, 0.0, e(2, 700, 1), 700, e(2, 1, 900), 900) == INVALID                  # k < 1
    assert call(lf, rt, 8, 1.0, u, 5600, vt, 7200) == INVALID                                     # tol = 1
    assert call(lf, rt, 8, -1e-3, u, 5600, vt, 7200) == INVALID                                   # tol < 0
    assert call(lf, rt, 8, 0.0, u, 5599, vt, 7200) == INVALID                                     # a short batch stride of u
    assert call(lf, rt, 8, 0.0, u, 5600, vt, 7199) == INVALID                                     # and of vt
    assert call(lf, rt, 8, 0.0, e(2, 700, 7), 4900, vt, 7200) == INVALID                          # u not m x kk
    assert call(lf, rt, 8, 0.0, e(2, 699, 8), 5592, vt, 7200) == INVALID
    assert call(lf, rt, 8, 0.0, u, 5600, e(2, 8, 899), 7192) == INVALID                           # vt not kk x n
    assert call(lf, rt, 8, 0.0, u, 5600, e(2, 7, 900), 6300) == INVALID
    assert call(lf, rt, 8, 0.0, u, 5600, vt, 7200, cnt=-1) == INVALID                             # count < 0
    assert call(lf, rt, 8, 0.0, u, 5600, vt, 7200, s_out=None) == INVALID                         # null outputs
    assert call(lf, rt, 8, 0.0, u, 5600, vt, 7200, rk=None) == INVALID
    assert call(lf, rt, 8, 0.0, None, 5600, vt, 7200) == INVALID
    assert call(lf, rt, 8, 0.0, u, 5600, None, 7200) == INVALID
    assert call(lf, rt, 8, 0.0, u, 5600, vt, 7200, cnt=0) == 0                                    # count = 0: nothing to do
    for bad in (torch.complex128, torch.complex64):  # real scalars only
        with pytest.raises(TypeError, match="lowrank_recompress_large_batched"):
            rc.lowrank_recompress_large_batched(torch.zeros((1, 600, 4), dtype=bad, device="cuda"), torch.zeros((1, 4, 700), dtype=bad, device="cuda"), 2)
    with pytest.raises(TypeError):
        rc.lowrank_recompress_large_batched(e(1, 600, 4), e(1, 4, 700).float(), 2)
    with pytest.raises(AssertionError, match="lowrank_recompress_large_batched"):  # RC_INVALID_ARGUMENT: the reference asserts
        rc.lowrank_recompress_large_batched(e(1, 600, 16), e(1, 16, 12), 4)
    # the existing entry points keep their domains
    with pytest.raises(AssertionError, match="lowrank_recompress_tall_batched"):
        rc.lowrank_recompress_tall_batched(e(1, 600, 16), e(1, 16, 513), 4)
