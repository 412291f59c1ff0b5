"""Batched recompression of low-rank factors to truncated SVDs (rc_lowrank_recompress_batched_*, batch.lowrank_recompress_batched and
its wrappers column_id_to_svd_batched, two_sided_id_to_svd_batched, svd_add_batched).

Per block the oracle is o.SVD.compute_from of A = left[:, :q] mid[:q, :q] diag(s[:q]) right[:q, :] formed in f64 on the host.  The
recompression is backward stable with respect to the factors, not to A, so every absolute bound is scaled by
sigma = ||left_q||_2 ||mid diag(s)||_2 ||right_q||_2 (f64, host) rather than by s_0:
    |s - s_ref| <= 4 TOL[sval] sigma,   ||U S V^T - A||_2 <= 4 TOL[recon] sigma + the discarded tail,   orthonormality <= 4 TOL[orth],
with TOL from tests/helpers.py and the factor 4 of test_gpu_batched_svd.py.  SciPy's pivoted QR + LAPACK SVD run as the same
method on the host sat 20-400x inside these bounds (1.0e-14 sigma in f64, 4.4e-7 sigma in f32, 1.2e-6 f32 orthogonality).  Singular
vectors are compared under test_gpu_batched_svd.check_vectors' gap rule on blocks whose factors are orthonormal, so that sigma = s_0."""
import ctypes

import numpy as np
import pytest
import torch

import rusty_compression_amd as rc
from oracle import ref_lapack as o
from rusty_compression_amd import _lib
from tests.helpers import TOL, batched_launch, npy
from tests.test_gpu_batched_svd import check_signs, check_vectors

pytestmark = pytest.mark.gpu

INVALID = 5
MODES = ("none", "mid", "s", "both")
DTYPES = [np.float64, np.float32]


def cuda(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def recompress(left, right, k, tol=0.0, mid=None, s=None, ranks=None):
    out = rc.lowrank_recompress_batched(cuda(left), cuda(right), k, tol, mid=cuda(mid), s=cuda(s), ranks=cuda(ranks))
    torch.cuda.synchronize()
    return tuple(npy(t) for t in out)


def clamp(q, K):
    return int(min(max(int(q), 0), K))


def dense(left, right, mid, s, q):
    """A = left[:, :q] mid[:q, :q] diag(s[:q]) right[:q, :] in f64 and the scale sigma of the error bounds."""
    lf, rt = left[:, :q].astype(np.float64), right[:q].astype(np.float64)
    core = np.eye(q) if mid is None else mid[:q, :q].astype(np.float64)
    if s is not None:
        core = core * s[:q].astype(np.float64)[None, :]
    if q == 0:
        return np.zeros((left.shape[0], right.shape[1])), 0.0
    sigma = np.linalg.norm(lf, 2) * np.linalg.norm(core, 2) * np.linalg.norm(rt, 2)
    return lf @ core @ rt, float(sigma)


def check_block(a, sigma, u, s_out, vt, r, q, kk, dtype, ref=None):
    """One block against the f64 oracle: the q singular values and the zero tail of s_out, orthonormality, the truncation error, zero
    tails of u and vt, signs.  Returns the oracle's SVD."""
    t = TOL[np.dtype(dtype)]
    ref = ref or o.SVD.compute_from(a)
    K = s_out.shape[0]
    assert 0 <= r <= min(kk, q)
    assert not np.any(s_out[q:]), "s_out past the inner rank is not zero"
    sv = s_out[:q].astype(np.float64)
    assert np.all(np.diff(sv) <= 0), "singular values not descending"
    want = np.zeros(K)
    want[:min(K, len(ref.s))] = ref.s[:K]
    err_s = np.abs(sv - want[:q]).max() if q else 0.0
    print(f"    sval err {err_s:.3e} bound {4 * t['sval'] * sigma:.3e}")
    assert err_s <= 4 * t["sval"] * sigma, (err_s, sigma)
    assert not np.any(u[:, r:]) and not np.any(vt[r:])
    if r == 0:
        return ref
    ur, vr = u[:, :r].astype(np.float64), vt[:r].astype(np.float64)
    orth = max(np.abs(ur.T @ ur - np.eye(r)).max(), np.abs(vr @ vr.T - np.eye(r)).max())
    err = np.linalg.norm(a - (ur * sv[:r]) @ vr, 2)
    tail = ref.s[r] if r < len(ref.s) else 0.0
    print(f"    orth {orth:.3e} bound {4 * t['orth']:.3e}; recon {err:.3e} tail {tail:.3e} bound {4 * t['recon'] * sigma:.3e}")
    assert orth <= 4 * t["orth"]
    assert err <= 4 * t["recon"] * sigma + tail, (err, tail, sigma)
    check_signs(u, vt, r)
    return ref


def orthonormal(rng, rows, cols):
    return np.linalg.qr(rng.standard_normal((rows, cols)))[0]


def spectrum(K):
    """2^-j, floored at 2^-30: the first triplets have gaps >= GAP, the floor keeps every value a normal f32 number."""
    return 2.0 ** -np.minimum(np.arange(K), 30).astype(np.float64)


def factors(rng, kind, m, n, K, mode, dtype):
    """One block's (left, right, mid, s) of inner width K in the given mode; mid / s are None when the mode has none.
    gauss: Gaussian factors.  spectrum: orthonormal outer factors and a core with singular values spectrum(K), so sigma = s_0 = 1.
    scaled: Gaussian factors, a core whose rows and diagonal span six orders of magnitude."""
    if kind == "spectrum":
        q1, q2, spec = orthonormal(rng, m, K), orthonormal(rng, n, K), spectrum(K)
        if mode == "none":
            left, right, mid, s = q1 * spec, q2.T, None, None
        elif mode == "s":
            left, right, mid, s = q1, q2.T, None, spec
        else:
            w1, w2 = orthonormal(rng, K, K), orthonormal(rng, K, K)
            mid, s = (w1 * spec) @ w2.T, None
            if mode == "both":
                s = rng.uniform(0.5, 2.0, K)
                mid = mid / s[None, :]
            left, right = q1, q2.T
    else:
        left, right = rng.standard_normal((m, K)), rng.standard_normal((K, n))
        mid = rng.standard_normal((K, K)) if mode in ("mid", "both") else None
        s = rng.uniform(0.5, 2.0, K) if mode in ("s", "both") else None
        if kind == "scaled":
            d = 10.0 ** -rng.uniform(0.0, 6.0, K)
            if mid is not None:
                mid = d[:, None] * mid
            elif s is not None:
                s = s * d
            else:
                left = left * d
    cast = lambda x: None if x is None else x.astype(dtype)  # noqa: E731
    return cast(left), cast(right), cast(mid), cast(s)


def stack(blocks):
    """[(left, right, mid, s), ...] -> the four batched operands (None where the mode has none)."""
    cols = list(zip(*blocks))
    return tuple(None if c[0] is None else np.stack(c) for c in cols)


# ---------------------------------------------------------------- 1. oracle parity across shapes
SHAPES = [(1, 1, 1), (7, 5, 3), (33, 17, 17), (64, 64, 64), (128, 128, 128), (200, 96, 40), (512, 128, 128), (128, 512, 64), (512, 512, 128)]
KINDS = ("gauss", "spectrum", "scaled")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m,n,K", SHAPES)
def test_oracle_parity_across_shapes(m, n, K, dtype):
    rng = np.random.default_rng(m * 100000 + n * 100 + K)
    for mode in MODES:
        blocks = [factors(rng, kind, m, n, K, mode, dtype) for kind in KINDS]
        left, right, mid, s = stack(blocks)
        refs = []
        for b in blocks:
            a, sigma = dense(*b, K)
            refs.append((a, sigma, o.SVD.compute_from(a)))
        seen = {}
        for k in sorted({1, max(1, K // 3), K, 200}):
            kk = min(k, K)
            u, s_out, vt, ranks = recompress(left, right, k, 0.0, mid, s)
            assert u.shape == (3, m, kk) and s_out.shape == (3, K) and vt.shape == (3, kk, n) and ranks.shape == (3,)
            if kk in seen:  # k past K is k = K: the same bits, checked once
                for v, w in zip(seen[kk], (u, s_out, vt, ranks)):
                    assert np.array_equal(v, w)
                continue
            seen[kk] = (u, s_out, vt, ranks)
            for i, kind in enumerate(KINDS):
                a, sigma, ref = refs[i]
                print(f"  {m}x{n} K={K} {np.dtype(dtype).name} {mode} k={k} {kind}")
                assert ranks[i] == kk
                check_block(a, sigma, u[i], s_out[i], vt[i], kk, K, kk, dtype, ref)
                if kind == "spectrum":  # sigma = s_0: the gap rule of the batched SVD's vectors applies as it stands
                    own = check_vectors(*_normalised(ref, kk), ref.u, ref.vt, ref.s, kk, dtype)
                    got = check_vectors(u[i], vt[i], ref.u, ref.vt, ref.s, kk, dtype)
                    assert got == own
                    assert got >= 3 or kk < 6, (got, kk)


def _normalised(ref, r):
    from tests.helpers import sign_normalise

    return sign_normalise(ref.u[:, :r], ref.vt[:r])


# ---------------------------------------------------------------- 2. dispatch edges
@pytest.mark.parametrize("dtype", DTYPES)
def test_inner_ranks_at_the_jacobi_switches(dtype):
    rng = np.random.default_rng(21)
    m = n = 130
    K = 128
    qs = [15, 16, 17, 32, 33, 64, 65, 128]
    blocks = [factors(rng, "gauss", m, n, K, "both", dtype) for _ in qs]
    left, right, mid, s = stack(blocks)
    u, s_out, vt, ranks = recompress(left, right, K, 0.0, mid, s, np.array(qs, dtype=np.int64))
    for i, q in enumerate(qs):
        print(f"  q={q} {np.dtype(dtype).name}")
        a, sigma = dense(*blocks[i], q)
        assert ranks[i] == q
        check_block(a, sigma, u[i], s_out[i], vt[i], q, q, K, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m", [64, 65, 128, 129, 256, 257])
def test_rows_at_the_reflector_switches(m, dtype):
    rng = np.random.default_rng(22 + m)
    K = 8
    for mm, nn in ((m, m), (m, 40), (40, m)):
        blocks = [factors(rng, kind, mm, nn, K, "s", dtype) for kind in ("gauss", "spectrum")]
        left, right, mid, s = stack(blocks)
        u, s_out, vt, ranks = recompress(left, right, K, 0.0, mid, s)
        for i in range(2):
            print(f"  {mm}x{nn} {np.dtype(dtype).name}")
            a, sigma = dense(*blocks[i], K)
            assert ranks[i] == K
            ref = check_block(a, sigma, u[i], s_out[i], vt[i], K, K, K, dtype)
            if i == 1:
                assert check_vectors(u[i], vt[i], ref.u, ref.vt, ref.s, K, dtype) >= 3


def test_odd_core_pitch():
    """K = 96 in f64 is the width at which the padded core pitch (112) no longer leaves room for the rotations and the odd one (97) does."""
    rng = np.random.default_rng(23)
    m, n, K = 150, 140, 96
    blocks = [factors(rng, kind, m, n, K, "both", np.float64) for kind in ("gauss", "spectrum")]
    left, right, mid, s = stack(blocks)
    (u, s_out, vt, ranks), lab = batched_launch(lambda: recompress(left, right, K, 0.0, mid, s))
    assert "ld=97" in lab["plan"], lab["plan"]
    for i in range(2):
        a, sigma = dense(*blocks[i], K)
        assert ranks[i] == K
        ref = check_block(a, sigma, u[i], s_out[i], vt[i], K, K, K, np.float64)
        if i == 1:
            assert check_vectors(u[i], vt[i], ref.u, ref.vt, ref.s, K, np.float64) >= 3


@pytest.mark.parametrize("m,n,plan", [(512, 64, "L:ws,R:lds"), (64, 512, "L:lds,R:ws")])
def test_the_larger_copy_leaves_lds_first(m, n, plan):
    """f64, K = 64: the copy of the 512-row factor (64 x 513 x 8 B = 257 KiB) cannot share LDS with the core and the rotations (2 x 64 x
    80 x 8 B = 80 KiB of the 159 KiB cap), the copy of the 64-row factor (64 x 65 x 8 B = 33 KiB) can: the plan moves the larger copy
    alone to the workspace, whichever side it is on."""
    rng = np.random.default_rng(24 + m)
    K = 64
    blocks = [factors(rng, kind, m, n, K, "both", np.float64) for kind in KINDS]
    left, right, mid, s = stack(blocks)
    (u, s_out, vt, ranks), lab = batched_launch(lambda: recompress(left, right, K, 0.0, mid, s))
    assert lab["plan"] == plan + f",V:lds,G:lds,ld=80,kk={K},mid,s", lab["plan"]
    for i in range(3):
        a, sigma = dense(*blocks[i], K)
        assert ranks[i] == K
        check_block(a, sigma, u[i], s_out[i], vt[i], K, K, K, np.float64)


# ---------------------------------------------------------------- 3. rank-aware
@pytest.mark.parametrize("dtype", DTYPES)
def test_inner_ranks_are_honoured_and_tails_are_never_read(dtype):
    rng = np.random.default_rng(31)
    m, n, K, k = 50, 44, 20, 12
    qs = np.array([0, 1, K // 2, K, -3, K + 5], dtype=np.int64)
    blocks = [factors(rng, "gauss", m, n, K, "both", dtype) for _ in qs]
    left, right, mid, s = stack(blocks)
    poisoned = [x.copy() for x in (left, right, mid, s)]
    zeroed = [x.copy() for x in (left, right, mid, s)]
    for fill, (pl, pr, pm, ps) in ((np.nan, poisoned), (0.0, zeroed)):
        for i, q in enumerate(qs):
            q = clamp(q, K)
            pl[i][:, q:] = fill
            pr[i][q:] = fill
            pm[i][q:] = fill
            pm[i][:, q:] = fill
            ps[i][q:] = fill
    got = recompress(poisoned[0], poisoned[1], k, 0.0, poisoned[2], poisoned[3], qs)
    clean = recompress(zeroed[0], zeroed[1], k, 0.0, zeroed[2], zeroed[3], qs)
    for v, w in zip(got, clean):
        assert np.array_equal(v, w)
    u, s_out, vt, ranks = got
    for i, q in enumerate(qs):
        q = clamp(q, K)
        print(f"  q={q} {np.dtype(dtype).name}")
        assert ranks[i] == min(k, q)
        a, sigma = dense(*blocks[i], q)
        check_block(a, sigma, u[i], s_out[i], vt[i], int(ranks[i]), q, k, dtype)
        if q == 0:
            assert not np.any(u[i]) and not np.any(vt[i]) and not np.any(s_out[i])
            continue
        # the truncated factors as a call of their own (inner width q): the same bits
        tl, tr, tm, ts = blocks[i]
        tu, tsv, tvt, trk = recompress(tl[None, :, :q], tr[None, :q], k, 0.0, tm[None, :q, :q], ts[None, :q])
        r = int(ranks[i])
        assert trk[0] == r
        assert np.array_equal(tsv[0], s_out[i][:q]) and np.array_equal(tu[0][:, :r], u[i][:, :r]) and np.array_equal(tvt[0][:r], vt[i][:r])


# ---------------------------------------------------------------- 4. rank rule
@pytest.mark.parametrize("dtype", DTYPES)
def test_rank_rule_on_known_spectra(dtype):
    rng = np.random.default_rng(41)
    m, n, K = 60, 48, 16
    # s_j / s_0 = 10^(-0.4 j) and 10^(-0.7 j); the second is floored in f32, whose rounding level is 1e-7 s_0
    specs = [10.0 ** (-0.4 * np.arange(K)), 10.0 ** (-0.7 * np.arange(K))]
    if dtype == np.float32:
        specs[1] = np.maximum(specs[1], 1e-5)
    blocks = []
    for spec in specs:
        blocks.append((orthonormal(rng, m, K).astype(dtype), orthonormal(rng, n, K).T.astype(dtype), None, spec.astype(dtype)))
    left, right, mid, s = stack(blocks)
    for tol in (0.0, 1e-8, 1e-3):
        for k in (5, K, 200):
            kk = min(k, K)
            u, s_out, vt, ranks = recompress(left, right, k, tol, mid, s)
            for i, spec in enumerate(specs):
                ratio = spec / spec[0]
                assert tol == 0.0 or np.all((ratio > 1.5 * tol) | (ratio < tol / 1.5))  # no ratio near the tolerance
                below = np.nonzero(ratio[:kk] < tol)[0]
                want = int(below[0]) if below.size else kk
                assert ranks[i] == want, (tol, k, i, ranks[i], want)
                a, sigma = dense(*blocks[i], K)
                check_block(a, sigma, u[i], s_out[i], vt[i], want, K, kk, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_zero_columns_of_left_give_exactly_zero_singular_values(dtype):
    rng = np.random.default_rng(42)
    m, n, K = 40, 36, 12
    blocks = []
    for mode in MODES:
        left, right, mid, s = factors(rng, "gauss", m, n, K, mode, dtype)
        left[:, [3, 7, 8]] = 0
        blocks.append((left, right, mid, s))
    for b, mode in zip(blocks, MODES):
        u, s_out, vt, ranks = recompress(b[0][None], b[1][None], K, 0.0, None if b[2] is None else b[2][None], None if b[3] is None else b[3][None])
        assert np.all(s_out[0][:9] > 0) and not np.any(s_out[0][9:]), (mode, s_out[0])
        assert ranks[0] == 9
        a, sigma = dense(*b, K)
        check_block(a, sigma, u[0], s_out[0], vt[0], 9, K, K, dtype)


# ---------------------------------------------------------------- 5. round trips
def low_rank_batch(rng, cnt, m, n, r, dtype):
    return (rng.standard_normal((cnt, m, r)) @ rng.standard_normal((cnt, r, n))).astype(dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_ids_convert_to_svds(dtype):
    rng = np.random.default_rng(51)
    cnt, m, n, k, r0 = 4, 70, 52, 16, 6
    tol = 1e-8 if dtype == np.float64 else 1e-4
    t = TOL[np.dtype(dtype)]
    exact = low_rank_batch(rng, cnt, m, n, r0, dtype)
    full = rng.standard_normal((cnt, m, n)).astype(dtype)
    for a_np, lowrank in ((exact, True), (full, False)):
        a = cuda(a_np)
        su, ss, svt, sr = (npy(x) for x in rc.svd_rank_batched(a, k, tol))
        c, z, _, ranks = rc.column_id_rank_batched(a, k, tol)
        cid = tuple(npy(x) for x in rc.column_id_to_svd_batched(c, z, ranks, k, tol))
        c2, x2, r2, _, _, ranks2 = rc.two_sided_id_rank_batched(a, k, tol)
        tsd = tuple(npy(x) for x in rc.two_sided_id_to_svd_batched(c2, x2, r2, ranks2, k, tol))
        torch.cuda.synchronize()
        for name, (u, s_out, vt, rk), fac, q_all in (("column", cid, (npy(c), npy(z), None, None), npy(ranks)),
                                                     ("two-sided", tsd, (npy(c2), npy(r2), npy(x2), None), npy(ranks2))):
            for i in range(cnt):
                q = int(q_all[i])
                print(f"  {name} ID block {i} q={q} {np.dtype(dtype).name} lowrank={lowrank}")
                prod, sigma = dense(fac[0][i], fac[1][i], None if fac[2] is None else fac[2][i], None, q)
                check_block(prod, sigma, u[i], s_out[i], vt[i], int(rk[i]), q, k, dtype)
                if lowrank:
                    # the ID is exact, so both routes hold the SVD of the block itself.  Three errors separate them, each within
                    # 4 TOL sigma: the recompression's, the ID's residual c z - a, and the batched SVD's (s_0(a) <= sigma)
                    assert q == r0 and rk[i] == r0 and sr[i] == r0
                    assert np.abs(s_out[i][:r0].astype(np.float64) - ss[i][:r0]).max() <= 12 * t["sval"] * sigma
                    rec = (u[i][:, :r0].astype(np.float64) * s_out[i][:r0]) @ vt[i][:r0]
                    srec = (su[i][:, :r0].astype(np.float64) * ss[i][:r0]) @ svt[i][:r0]
                    assert np.linalg.norm(rec - srec, 2) <= 12 * t["recon"] * sigma


@pytest.mark.parametrize("dtype", DTYPES)
def test_svd_add_of_low_rank_batches(dtype):
    rng = np.random.default_rng(52)
    cnt, m, n, k, r1, r2 = 4, 64, 80, 12, 5, 7
    tol = 1e-8 if dtype == np.float64 else 1e-4
    a1, a2 = low_rank_batch(rng, cnt, m, n, r1, dtype), low_rank_batch(rng, cnt, m, n, r2, dtype)
    f1, f2 = rc.svd_rank_batched(cuda(a1), k, tol), rc.svd_rank_batched(cuda(a2), k, tol)
    assert list(npy(f1[3])) == [r1] * cnt and list(npy(f2[3])) == [r2] * cnt
    u, s_out, vt, ranks = (npy(x) for x in rc.svd_add_batched(*f1[:3], *f2[:3], 2 * k, tol))
    torch.cuda.synchronize()
    assert s_out.shape == (cnt, 2 * k)
    for i in range(cnt):
        print(f"  add block {i} {np.dtype(dtype).name}")
        left = np.concatenate([npy(f1[0])[i], npy(f2[0])[i]], axis=1)
        right = np.concatenate([npy(f1[2])[i], npy(f2[2])[i]], axis=0)
        s = np.concatenate([npy(f1[1])[i][:k], npy(f2[1])[i][:k]])
        prod, sigma = dense(left, right, None, s, 2 * k)
        assert ranks[i] == r1 + r2
        assert not np.any(s_out[i][r1 + r2:]), "zero tails of the summands must give exactly zero singular values"
        check_block(prod, sigma, u[i], s_out[i], vt[i], r1 + r2, 2 * k, 2 * k, dtype)
        # and against the dense sum itself: next to the recompression's 4 TOL sigma, each summand's batched SVD is within
        # 4 TOL s_0 of its block, and s_0 of either block is at most sigma
        ref = o.SVD.compute_from(a1[i].astype(np.float64) + a2[i].astype(np.float64))
        assert np.abs(s_out[i][:r1 + r2] - ref.s[:r1 + r2]).max() <= 12 * TOL[np.dtype(dtype)]["sval"] * sigma


@pytest.mark.parametrize("dtype", DTYPES)
def test_cancelling_sum_meets_the_factor_scaled_bound(dtype):
    rng = np.random.default_rng(53)
    cnt, m, n, k = 3, 48, 40, 10
    a = rng.standard_normal((cnt, m, n)).astype(dtype)
    u0, s0, vt0, _ = rc.svd_rank_batched(cuda(a), k, 0.0)
    s1 = (-(1.0 - 1e-6) * s0).to(s0.dtype)  # A_k - (1 - 1e-6) A_k
    u, s_out, vt, ranks = (npy(x) for x in rc.svd_add_batched(u0, s0, vt0, u0, s1, vt0, k, 0.0))
    torch.cuda.synchronize()
    for i in range(cnt):
        print(f"  cancelling block {i} {np.dtype(dtype).name}")
        left = np.concatenate([npy(u0)[i]] * 2, axis=1)
        right = np.concatenate([npy(vt0)[i]] * 2, axis=0)
        s = np.concatenate([npy(s0)[i][:k], npy(s1)[i][:k]])
        prod, sigma = dense(left, right, None, s, 2 * k)
        assert 0 <= ranks[i] <= k
        check_block(prod, sigma, u[i], s_out[i], vt[i], int(ranks[i]), 2 * k, k, dtype)


# ---------------------------------------------------------------- 6. the batch contract
def _view(t):
    if t is None:
        return _lib.mat(None), ctypes.c_int64(0)
    return _lib.rc_matrix(t.data_ptr(), t.shape[1], t.shape[2], t.stride(1), t.stride(2)), ctypes.c_int64(t.stride(0))


def _raw(left, mid, s, right, in_ranks, cnt, k, tol, u, ubs, s_out, vt, vbs, ranks, ctx=None, dtype=torch.float64):
    ctx = ctx or _lib.default_context()
    fn = getattr(_lib.lib(), f"rc_lowrank_recompress_batched_{_lib.suffix(dtype)}")
    return fn(ctx._h, *_view(left), *_view(mid), ctypes.c_void_p(s.data_ptr() if s is not None else None),
              ctypes.c_int64(s.stride(0) if s is not None else 0), *_view(right), _lib.i64p(in_ranks), ctypes.c_int32(cnt), ctypes.c_int64(k),
              ctypes.c_double(tol), u, ctypes.c_int64(ubs), ctypes.c_void_p(s_out.data_ptr() if s_out is not None else None), vt, ctypes.c_int64(vbs),
              _lib.i64p(ranks))


def test_bits_independent_of_count_position_and_neighbours():
    rng = np.random.default_rng(61)
    m, n, K, k, tol = 24, 20, 8, 6, 1e-9
    protos = [factors(rng, kind, m, n, K, "both", np.float64) for kind in ("gauss", "spectrum", "scaled", "gauss", "gauss", "scaled", "gauss")]
    qs = [K, K, 5, 0, 1, K + 2, 3]
    alone = []
    labels = None
    for b, q in zip(protos, qs):
        out, labels = batched_launch(lambda: recompress(b[0][None], b[1][None], k, tol, b[2][None], b[3][None], np.array([q], dtype=np.int64)))
        alone.append(out)
    assert labels["op"] == "batched_recompress" and (labels["m"], labels["n"], labels["k"], labels["count"], labels["grid"]) == (m, n, K, 1, 1)
    cnt = labels["slots"] + 3  # the last three blocks are some workgroup's second
    pick = [(5 * i + i // 7) % 7 for i in range(cnt)]
    left, right, mid, s = stack([protos[p] for p in pick])
    got, lab = batched_launch(lambda: recompress(left, right, k, tol, mid, s, np.array([qs[p] for p in pick], dtype=np.int64)))
    assert lab["count"] == cnt and lab["grid"] == lab["slots"] and lab["plan"] == labels["plan"]
    for i, p in enumerate(pick):
        for v, w in zip(alone[p], got):
            assert np.array_equal(v[0], w[i]), (i, p)


@pytest.mark.parametrize("dtype", DTYPES)
def test_input_views_give_the_same_bits(dtype):
    rng = np.random.default_rng(62)
    cnt, m, n, K, k = 5, 70, 50, 12, 9
    left, right, mid, s = (cuda(x) for x in stack([factors(rng, "gauss", m, n, K, "both", dtype) for _ in range(cnt)]))
    ref = tuple(npy(x) for x in rc.lowrank_recompress_batched(left, right, k, 1e-6, mid=mid, s=s))

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
        got = rc.lowrank_recompress_batched(f(left), f(right), k, 1e-6, mid=f(mid), s=spad)
        for v, w in zip(ref, got):
            assert np.array_equal(v, npy(w))
    shared = right[2:3].expand(cnt, K, n)  # right_batch_stride = 0
    assert shared.stride(0) == 0
    got = rc.lowrank_recompress_batched(left, shared, k, 1e-6, mid=mid, s=s)
    one = rc.lowrank_recompress_batched(left[2:3], right[2:3], k, 1e-6, mid=mid[2:3], s=s[2:3])
    for v, w, x in zip(ref, got, one):
        assert np.array_equal(v[2], npy(w)[2]) and np.array_equal(v[2], npy(x)[0])


def test_strided_outputs_leave_the_gaps_untouched():
    rng = np.random.default_rng(63)
    cnt, m, n, K, k = 6, 90, 40, 14, 10
    left, right, mid, s = (cuda(x) for x in stack([factors(rng, "gauss", m, n, K, "mid", np.float64) for _ in range(cnt)]))
    ref = tuple(npy(x) for x in rc.lowrank_recompress_batched(left, right, k, 1e-3, mid=mid))
    ut = torch.full((cnt, k, m + 1), 7.0, dtype=left.dtype, device=left.device)   # u column-major, padded
    vtt = torch.full((cnt, n, k + 2), 7.0, dtype=left.dtype, device=left.device)  # vt column-major, padded
    s_out = torch.zeros((cnt, K), dtype=left.dtype, device=left.device)
    ranks = torch.zeros(cnt, dtype=torch.int64, device=left.device)
    uv = _lib.rc_matrix(ut.data_ptr(), m, k, 1, m + 1)
    vv = _lib.rc_matrix(vtt.data_ptr(), k, n, 1, k + 2)
    assert _raw(left, mid, None, right, None, cnt, k, 1e-3, uv, k * (m + 1), s_out, vv, n * (k + 2), ranks) == 0
    torch.cuda.synchronize()
    assert np.array_equal(npy(ut)[:, :, :m].transpose(0, 2, 1), ref[0])
    assert np.array_equal(npy(vtt)[:, :, :k].transpose(0, 2, 1), ref[2])
    assert np.all(npy(ut)[:, :, m:] == 7.0) and np.all(npy(vtt)[:, :, k:] == 7.0)
    assert np.array_equal(npy(s_out), ref[1]) and np.array_equal(npy(ranks), ref[3])


def test_graph_capture_replays_the_eager_bits():
    rng = np.random.default_rng(64)
    cnt, m, n, K, k = 33, 96, 128, 24, 16
    lib = _lib.lib()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        left, right, mid, s = (cuda(x) for x in stack([factors(rng, "gauss", m, n, K, "both", np.float64) for _ in range(cnt)]))
        in_ranks = cuda(rng.integers(0, K + 1, cnt).astype(np.int64))
        eager = tuple(npy(x) for x in rc.lowrank_recompress_batched(left, right, k, 1e-9, mid=mid, s=s, ranks=in_ranks))
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
    u, s, vt, r = rc.lowrank_recompress_batched(e(0, 30, 8), e(0, 8, 20), 5)
    assert u.shape == (0, 30, 5) and s.shape == (0, 8) and vt.shape == (0, 5, 20) and r.shape == (0,)


# ---------------------------------------------------------------- 7. containment of non-finite input
@pytest.mark.parametrize("dtype", DTYPES)
def test_nan_stays_in_its_block(dtype):
    rng = np.random.default_rng(71)
    cnt, m, n, K, k = 12, 90, 70, 30, 20
    left, right, mid, s = stack([factors(rng, "gauss", m, n, K, "both", dtype) for _ in range(cnt)])
    ref = recompress(left, right, k, 1e-5, mid, s)
    left, right, mid, s = left.copy(), right.copy(), mid.copy(), s.copy()
    left[4, 17, 3] = np.nan
    right[8, 5, :] = np.inf
    mid[2, 1, 1] = np.nan
    s[10, 0] = -np.inf
    got = recompress(left, right, k, 1e-5, mid, s)
    for i in range(cnt):
        assert 0 <= got[3][i] <= k
        if i in (2, 4, 8, 10):
            continue
        for v, w in zip(ref, got):
            assert np.array_equal(v[i], w[i])
    _lib.default_context().get_health()  # whatever the bad blocks raised


# ---------------------------------------------------------------- 8. arguments and health
def test_argument_checks():
    e = lambda c, r, q: torch.zeros((c, r, q), dtype=torch.float64, device="cuda")  # noqa: E731
    sbuf = torch.zeros((2, 600), dtype=torch.float64, device="cuda")
    ranks = torch.zeros(2, dtype=torch.int64, device="cuda")

    def call(left, right, k, tol, u, ubs, vt, vbs, mid=None, cnt=2, s_out=sbuf, rk=ranks, in_ranks=None):
        return _raw(left, mid, None, right, in_ranks, cnt, k, tol, _lib.mat(u[0]) if u is not None else _lib.mat(None), ubs, s_out,
                    _lib.mat(vt[0]) if vt is not None else _lib.mat(None), vbs, rk)

    lf, rt, u, vt = e(2, 200, 16), e(2, 16, 100), e(2, 200, 8), e(2, 8, 100)
    assert call(lf, rt, 8, 0.0, u, 1600, vt, 800) == 0                                             # the valid call the rest departs from
    assert call(e(2, 520, 16), rt, 8, 0.0, e(2, 520, 8), 4160, vt, 800) == INVALID                # m > 512
    assert call(lf, e(2, 16, 520), 8, 0.0, u, 1600, e(2, 8, 520), 4160) == INVALID                # n > 512
    assert call(e(2, 200, 129), e(2, 129, 200), 8, 0.0, u, 1600, e(2, 8, 200), 1600) == INVALID   # K > 128
    assert call(e(2, 200, 16), e(2, 16, 12), 8, 0.0, u, 1600, e(2, 8, 12), 96) == INVALID         # K > min(m, n)
    msg = _lib.lib().rc_last_error_message(_lib.default_context()._h).decode()
    assert "rc_svd_rank_batched" in msg
    assert call(lf, e(2, 15, 100), 8, 0.0, u, 1600, vt, 800) == INVALID                           # left.cols != right.rows
    assert call(lf, rt, 8, 0.0, u, 1600, vt, 800, mid=e(2, 16, 15)) == INVALID                    # mid not K x K
    assert call(lf, rt, 0, 0.0, e(2, 200, 1), 200, e(2, 1, 100), 100) == INVALID                  # k < 1
    assert call(lf, rt, 8, 1.0, u, 1600, vt, 800) == INVALID                                      # tol >= 1
    assert call(lf, rt, 8, -1e-3, u, 1600, vt, 800) == INVALID                                    # tol < 0
    assert call(lf, rt, 8, 0.0, u, 1599, vt, 800) == INVALID                                      # u of two blocks overlap
    assert call(lf, rt, 8, 0.0, u, 1600, vt, 799) == INVALID                                      # vt of two blocks overlap
    assert call(lf, rt, 8, 0.0, e(2, 200, 7), 1400, vt, 800) == INVALID                           # wrong u shape
    assert call(lf, rt, 8, 0.0, u, 1600, e(2, 8, 99), 792) == INVALID                             # wrong vt shape
    assert call(lf, rt, 200, 0.0, u, 1600, vt, 800) == INVALID                                    # k clamps to K = 16, not to 8
    assert call(lf, rt, 8, 0.0, u, 1600, vt, 800, cnt=-1) == INVALID                              # count < 0
    assert call(lf, rt, 8, 0.0, u, 1600, vt, 800, s_out=None) == INVALID                          # null s_out
    assert call(lf, rt, 8, 0.0, u, 1600, vt, 800, rk=None) == INVALID                             # null ranks
    assert call(lf, rt, 8, 0.0, None, 1600, vt, 800) == INVALID                                   # null u
    assert call(lf, rt, 8, 0.0, u, 1600, None, 800) == INVALID                                    # null vt
    fn = _lib.lib().rc_lowrank_recompress_batched_f64
    zero, ctx = ctypes.c_int64(0), _lib.default_context()
    for null_left in (True, False):                                                                # null left, null right
        lv = (_lib.rc_matrix(None, 200, 16, 16, 1), ctypes.c_int64(3200)) if null_left else _view(lf)
        rv = _view(rt) if null_left else (_lib.rc_matrix(None, 16, 100, 100, 1), ctypes.c_int64(1600))
        assert fn(ctx._h, *lv, _lib.mat(None), zero, None, zero, *rv, None, ctypes.c_int32(2), ctypes.c_int64(8), ctypes.c_double(0.0), _lib.mat(u[0]),
                  ctypes.c_int64(1600), ctypes.c_void_p(sbuf.data_ptr()), _lib.mat(vt[0]), ctypes.c_int64(800), _lib.i64p(ranks)) == INVALID
    assert fn(ctypes.c_void_p(None), *_view(lf), _lib.mat(None), zero, None, zero, *_view(rt), None, ctypes.c_int32(2), ctypes.c_int64(8),
              ctypes.c_double(0.0), _lib.mat(u[0]), ctypes.c_int64(1600), ctypes.c_void_p(sbuf.data_ptr()), _lib.mat(vt[0]), ctypes.c_int64(800),
              _lib.i64p(ranks)) == INVALID                                                         # null ctx
    assert call(lf, rt, 8, 0.0, u, 1600, vt, 800, cnt=0) == 0                                     # count = 0: nothing to do
    with pytest.raises(AssertionError, match="rc_svd_rank_batched"):  # RC_INVALID_ARGUMENT: the reference asserts
        rc.lowrank_recompress_batched(e(1, 20, 16), e(1, 16, 12), 4)
    for bad in (torch.complex128, torch.complex64):
        with pytest.raises(TypeError):
            rc.lowrank_recompress_batched(torch.zeros((1, 8, 4), dtype=bad, device="cuda"), torch.zeros((1, 4, 8), dtype=bad, device="cuda"), 2)
    with pytest.raises(TypeError):
        rc.lowrank_recompress_batched(e(1, 8, 4), e(1, 4, 8).float(), 2)
    with pytest.raises(TypeError):
        rc.svd_add_batched(*[torch.zeros((1, 8, 2), dtype=torch.complex64, device="cuda"), torch.zeros((1, 2), device="cuda"),
                             torch.zeros((1, 2, 8), dtype=torch.complex64, device="cuda")] * 2, 2)


@pytest.mark.parametrize("dtype", DTYPES)
def test_clean_inputs_leave_the_health_word_clear(dtype):
    rng = np.random.default_rng(81)
    ctx = _lib.default_context()
    ctx.synchronize()
    ctx.get_health()
    m, n, K = 140, 130, 128
    blocks = [factors(rng, kind, m, n, K, "both", dtype) for kind in KINDS]
    clustered = np.concatenate([np.ones(10), 0.5 * np.ones(40), 1e-3 * (1 + 1e-9 * np.arange(78))])
    blocks.append((orthonormal(rng, m, K).astype(dtype), orthonormal(rng, n, K).T.astype(dtype), np.eye(K, dtype=dtype), clustered.astype(dtype)))
    left, right, mid, s = stack(blocks)
    u, s_out, vt, ranks = recompress(left, right, 64, 0.0, mid, s)
    ctx.synchronize()
    assert ctx.get_health() == 0
    for i, b in enumerate(blocks):
        a, sigma = dense(*b, K)
        assert ranks[i] == 64
        check_block(a, sigma, u[i], s_out[i], vt[i], 64, K, 64, dtype)
