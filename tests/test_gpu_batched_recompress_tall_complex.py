"""Batched recompression of complex factor pairs with a tall left factor (rc_lowrank_recompress_tall_complex_batched_c64 / _c32,
batch.lowrank_recompress_tall_batched_complex and its wrappers column_id_to_svd_tall_batched_complex, svd_add_tall_batched_complex,
sketch_svd_rank_batched_complex): the complex twin of tests/test_gpu_batched_recompress_tall.py.

The oracle, the bounds and the block generators are those of tests/test_gpu_batched_recompress_complex.py (check_block: 4 TOL sigma with
sigma the product of the factors' 2-norms, TOL keyed by the real dtype), the vector and phase checks those of
tests/test_gpu_batched_svd_complex.py.  The left factor goes through a flat Householder TSQR in stages of H = 512 rows; a numpy model of
that scheme on complex data (per-stage pivoted complex Householder in the working type, backward pass through the stored reflectors; the
eight edge shapes below and 4000 x 130, K = 128 with 11 stages; Gaussian, duplicated-column and cond 1e14 (c64) / 1e7 (c32) left factors)
stays at most 0.0004 / 0.0009 / 0.0011 of the sval / recon / orth bounds in c64 and 0.003 / 0.021 / 0.029 in c32: 35 times inside at
the tightest (c32 orthonormality).  With q the inner rank, stage 0 holds rows 0 .. 511 and every later stage the next 512 - q rows, so the
stage edges of a shape are at m = 512 + j (512 - q)."""
import ctypes

import numpy as np
import pytest
import torch

import rusty_compression_amd as rc
from rusty_compression_amd import _lib
from tests.helpers import TOL, batched_launch, npy
from tests.test_gpu_batched_recompress_complex import check_block, clamp, dense, factors, gaussian, orthonormal, stack
from tests.test_gpu_batched_svd_complex import check_phases, check_vectors, real_of

pytestmark = pytest.mark.gpu

C64, C32 = np.complex128, np.complex64
INVALID = 5
H = 512
MODES = ("none", "mid", "s", "both")
DTYPES = [C64, C32]
KINDS = ("gauss", "spectrum", "scaled")


def cuda(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def recompress_tall(left, right, k, tol=0.0, mid=None, s=None, ranks=None):
    out = rc.lowrank_recompress_tall_batched_complex(cuda(left), cuda(right), k, tol, mid=cuda(mid), s=cuda(s), ranks=cuda(ranks))
    torch.cuda.synchronize()
    return tuple(npy(t) for t in out)


def stages(m, q):
    return 1 if m <= H else 1 + -(-(m - H) // (H - q))


def phase_normalise(u, vt):
    """The contract's phase rule applied to reference vectors: each column of u times conj(x) / |x| of its first largest-modulus entry x,
    the matching row of vt times the conjugate phase."""
    u, vt = np.array(u, dtype=C64), np.array(vt, dtype=C64)
    for j in range(u.shape[1]):
        i = int(np.argmax(np.abs(u[:, j])))
        ph = np.conj(u[i, j]) / abs(u[i, j])
        u[:, j] *= ph
        vt[j] *= np.conj(ph)
    return u, vt


# ---------------------------------------------------------------- 1. m <= 512: the bits of the existing call
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m", [1, 64, 257, 512])
def test_up_to_512_rows_the_bits_are_the_existing_calls(m, dtype):
    rng = np.random.default_rng(100 + m)
    ran = 0
    for n, K in ((5, 1), (96, 40), (128, 128)):
        if K > min(m, n):
            continue
        qs = np.array([K, K // 2, 0, K + 3, max(K - 1, 0)], dtype=np.int64)
        for mode in MODES:
            left, right, mid, s = (cuda(x) for x in stack([factors(rng, "gauss", m, n, K, mode, dtype) for _ in qs]))
            for tol in (0.0, 1e-3):
                for ranks in (None, cuda(qs)):
                    k = max(1, (2 * K) // 3)
                    want = rc.lowrank_recompress_batched_complex(left, right, k, tol, mid=mid, s=s, ranks=ranks)
                    got = rc.lowrank_recompress_tall_batched_complex(left, right, k, tol, mid=mid, s=s, ranks=ranks)
                    for name, v, w in zip(("u", "s_out", "vt", "ranks"), want, got):
                        assert torch.equal(v, w), (m, n, K, mode, tol, name)
                    ran += 1
    assert ran >= 16  # m = 1 admits (5, 1) alone: four modes, two tolerances, with and without ranks


# ---------------------------------------------------------------- 2. oracle parity at the stage edges
# the first extra row, the edge between stages 1 and 2 at q = 128 (896 | 897) and at q = 17 (1021 | 1022), four to five stages
EDGES = [(513, 5, 3), (513, 130, 128), (896, 130, 128), (897, 130, 128), (1021, 17, 17), (1022, 17, 17), (1500, 96, 40), (2100, 64, 64)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m,n,K", EDGES)
def test_oracle_parity_at_the_stage_edges(m, n, K, dtype):
    rng = np.random.default_rng(m * 100000 + n * 100 + K)
    for mode in MODES:
        blocks = [factors(rng, kind, m, n, K, mode, dtype) for kind in KINDS]
        left, right, mid, s = stack(blocks)
        u, s_out, vt, ranks = recompress_tall(left, right, K, 0.0, mid, s)
        assert u.shape == (3, m, K) and s_out.shape == (3, K) and vt.shape == (3, K, n)
        for i, kind in enumerate(KINDS):
            print(f"  {m}x{n} K={K} {np.dtype(dtype).name} {mode} {kind} stages={stages(m, K)}")
            a, sigma = dense(*blocks[i], K)
            assert ranks[i] == K
            ref = check_block(a, sigma, u[i], s_out[i], vt[i], K, K, K, dtype)
            if kind == "spectrum":  # sigma = s_0: the gap rule of the batched SVD's vectors applies as it stands
                own = check_vectors(*phase_normalise(ref.u[:, :K], ref.vt[:K]), ref.u, ref.vt, ref.s, K, dtype)
                got = check_vectors(u[i], vt[i], ref.u, ref.vt, ref.s, K, dtype)
                assert got == own
                assert got >= 3 or K < 6, (got, K)


# ---------------------------------------------------------------- 3. the last row of the domain
@pytest.mark.parametrize("dtype", DTYPES)
def test_the_last_row_of_the_domain(dtype):
    """m = 65536, K = 8: 1 + ceil(65024 / 504) = 131 stages; row indices, chunk offsets and the phase rule's row at their largest values."""
    rng = np.random.default_rng(65536)
    m, n, K = 65536, 16, 8
    assert stages(m, K) == 131
    blocks = [factors(rng, kind, m, n, K, "s", dtype) for kind in ("gauss", "spectrum")]
    blocks[0][0][:-1, 0] *= 0.01  # the dominant entry of a column of u in the last row: the last chunk's last lane decides a phase
    blocks[0][0][-1, 0] = 30.0 * np.exp(0.7j)
    left, right, mid, s = stack(blocks)
    (u, s_out, vt, ranks), lab = batched_launch(lambda: recompress_tall(left, right, K, 0.0, mid, s))
    assert lab["op"] == "batched_recompress_tall<complex>"
    assert lab["plan"].startswith("stages=131,L:ws,")
    col = int(np.argmax(np.abs(u[0]).max(axis=0)))
    assert int(np.argmax(np.abs(u[0][:, col]))) == m - 1
    assert u[0][m - 1, col].imag == 0 and u[0][m - 1, col].real > 0
    for i in range(2):
        a, sigma = dense(*blocks[i], K)
        assert ranks[i] == K
        ref = check_block(a, sigma, u[i], s_out[i], vt[i], K, K, K, dtype)
        if i == 1:
            assert check_vectors(u[i], vt[i], ref.u, ref.vt, ref.s, K, dtype) >= 3


# ---------------------------------------------------------------- 4. the inner rank sets the stage height
@pytest.mark.parametrize("dtype", DTYPES)
def test_in_ranks_change_the_stage_height_and_tails_are_never_read(dtype):
    rng = np.random.default_rng(31)
    m, n, K, k = 1100, 70, 64, 40
    qs = np.array([0, 1, 17, 64, -3, 99], dtype=np.int64)
    # three stages at every q, with the second stage's last row at 512 + (512 - q) - 1: 1022, 1006, 959
    assert [stages(m, q) for q in (1, 17, 64)] == [3, 3, 3]
    blocks = [factors(rng, "gauss", m, n, K, "both", dtype) for _ in qs]
    left, right, mid, s = (x.copy() for x in stack(blocks))
    for i, q in enumerate(qs):
        q = clamp(q, K)
        left[i][:, q:] = np.nan
        right[i][q:] = np.nan
        mid[i][q:] = np.nan
        mid[i][:, q:] = np.nan
        s[i][q:] = np.nan
    u, s_out, vt, ranks = recompress_tall(left, right, k, 0.0, mid, s, qs)
    for i, q in enumerate(qs):
        q = clamp(q, K)
        print(f"  q={q} {np.dtype(dtype).name}")
        assert ranks[i] == min(k, q)
        a, sigma = dense(*blocks[i], q)
        check_block(a, sigma, u[i], s_out[i], vt[i], int(ranks[i]), q, k, dtype)
        if q == 0:
            assert not np.any(u[i]) and not np.any(vt[i]) and not np.any(s_out[i])
            continue
        tl, tr, tm, ts = blocks[i]  # the truncated factors as a call of their own (inner width q): the same bits
        tu, tsv, tvt, trk = recompress_tall(tl[None, :, :q], tr[None, :q], k, 0.0, tm[None, :q, :q], ts[None, :q])
        r = int(ranks[i])
        assert trk[0] == r
        assert np.array_equal(tsv[0], s_out[i][:q]) and np.array_equal(tu[0][:, :r], u[i][:, :r]) and np.array_equal(tvt[0][:r], vt[i][:r])


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_stage_count_differs_across_inner_ranks_of_one_batch(dtype):
    """m = 1534 = 512 + 2 * 511: q = 1 fills exactly three stages (1 + 1022 / 511), q = 64 and q = 100 need a fourth
    (1 + ceil(1022 / 448), 1 + ceil(1022 / 412)); one row more and q = 1 needs four as well."""
    rng = np.random.default_rng(32)
    m, n, K = 1534, 110, 100
    qs = np.array([1, 64, 100], dtype=np.int64)
    assert [stages(m, int(q)) for q in qs] == [3, 4, 4] and stages(m + 1, 1) == 4
    blocks = [factors(rng, "gauss", m, n, K, "s", dtype) for _ in qs]
    left, right, mid, s = stack(blocks)
    u, s_out, vt, ranks = recompress_tall(left, right, K, 0.0, mid, s, qs)
    for i, q in enumerate(qs):
        q = int(q)
        a, sigma = dense(*blocks[i], q)
        assert ranks[i] == q
        check_block(a, sigma, u[i], s_out[i], vt[i], q, q, K, dtype)


# ---------------------------------------------------------------- 5. exact zeros
@pytest.mark.parametrize("dtype", DTYPES)
def test_zero_columns_of_left_give_exactly_zero_singular_values(dtype):
    rng = np.random.default_rng(42)
    m, n, K = 1500, 60, 12
    for mode in MODES:
        zl, zr, zm, zs = factors(rng, "gauss", m, n, K, mode, dtype)
        zl[:, [3, 7]] = 0                      # zero in every stage
        pl, pr, pm, ps = factors(rng, "gauss", m, n, K, mode, dtype)
        pl[H:, 5] = 0                          # zero only below the first stage: not a zero column
        blocks = [(zl, zr, zm, zs), (pl, pr, pm, ps)]
        left, right, mid, s = stack(blocks)
        u, s_out, vt, ranks = recompress_tall(left, right, K, 0.0, mid, s)
        assert np.all(s_out[0][:10] > 0) and not np.any(s_out[0][10:]), (mode, s_out[0])
        assert np.all(s_out[1] > 0), (mode, s_out[1])
        assert list(ranks) == [10, 12]
        for i in range(2):
            a, sigma = dense(*blocks[i], K)
            check_block(a, sigma, u[i], s_out[i], vt[i], int(ranks[i]), K, K, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_svd_add_of_a_block_with_itself(dtype):
    """x + x through the rank-deficient left factor [U U]: the singular values are 2 s, the other ones are rounding of sigma, and where the
    inputs' columns were zero (ranks below k, as the batched SVD writes them) the trailing values are exactly 0."""
    rng = np.random.default_rng(43)
    cnt, m, n, k = 3, 1500, 64, 20
    rd = real_of(dtype)
    t = TOL[rd]
    live = [k, k - 4, k - 7]  # nonzero columns per block
    u0 = np.stack([orthonormal(rng, m, k) for _ in range(cnt)]).astype(dtype)
    vt0 = np.stack([orthonormal(rng, n, k).conj().T for _ in range(cnt)]).astype(dtype)
    s0 = np.stack([np.sort(rng.uniform(0.5, 2.0, k))[::-1] for _ in range(cnt)]).astype(rd)
    for i, r in enumerate(live):
        u0[i][:, r:] = 0
        vt0[i][r:] = 0
        s0[i][r:] = 0
    u, s_out, vt, ranks = (npy(x) for x in rc.svd_add_tall_batched_complex(cuda(u0), cuda(s0), cuda(vt0), cuda(u0), cuda(s0), cuda(vt0), 2 * k, 0.0))
    torch.cuda.synchronize()
    assert s_out.shape == (cnt, 2 * k) and s_out.dtype == rd
    for i, r0 in enumerate(live):
        left, right = np.concatenate([u0[i]] * 2, axis=1), np.concatenate([vt0[i]] * 2, axis=0)
        a, sigma = dense(left, right, None, np.concatenate([s0[i]] * 2), 2 * k)
        err = np.abs(s_out[i][:k].astype(np.float64) - 2.0 * s0[i].astype(np.float64)).max()
        rest = np.abs(s_out[i][k:]).max()
        print(f"  block {i} {np.dtype(dtype).name}: |s - 2 s0| {err:.3e}, rest {rest:.3e}, bound {4 * t['sval'] * sigma:.3e}")
        assert err <= 4 * t["sval"] * sigma and rest <= 4 * t["sval"] * sigma
        assert not np.any(s_out[i][2 * r0:]), "zero columns of the summands must give exactly zero singular values"
        r = int(ranks[i])
        assert r0 <= r <= 2 * r0
        ur = u[i][:, :r].astype(C64)
        assert np.abs(ur.conj().T @ ur - np.eye(r)).max() <= 4 * t["orth"]
        check_block(a, sigma, u[i][:, :r0], s_out[i], vt[i][:r0], r0, 2 * k, r0, dtype)  # the leading triplets as a rank-r0 truncation


# ---------------------------------------------------------------- 6. the phase rule runs over every chunk of rows
@pytest.mark.parametrize("dtype", DTYPES)
def test_phase_rule_over_chunks(dtype):
    """K = 3, m = 1100: chunks of rows [0, 512), [512, 1021), [1021, 1100).  u's first column is, up to a phase, the first column of left,
    which carries one dominant entry of modulus 1 and a chosen phase in a chosen chunk."""
    rng = np.random.default_rng(51)
    m, n, K = 1100, 30, 3
    rd = real_of(dtype)
    blocks, rows = [], []
    for row in (1090, 5, 700, 1021, 511):
        for theta in (0.0, np.pi / 2, np.pi, 2.1):
            spike = 0.01 * gaussian(rng, m, 1)[:, 0]
            spike[row] = np.exp(1j * theta)
            q1 = np.linalg.qr(np.column_stack([spike, gaussian(rng, m, K - 1)]))[0]
            blocks.append((q1.astype(dtype), orthonormal(rng, n, K).conj().T.astype(dtype), None, np.array([4.0, 2.0, 1.0], dtype=rd)))
            rows.append(row)
    left, right, mid, s = stack(blocks)
    u, s_out, vt, ranks = recompress_tall(left, right, K, 0.0, mid, s)
    for i, row in enumerate(rows):
        assert ranks[i] == K
        assert int(np.argmax(np.abs(u[i][:, 0]))) == row, (i, row)
        assert u[i][row, 0].imag == 0 and u[i][row, 0].real > 0, (i, row, u[i][row, 0])
        check_phases(u[i], K)
        a, sigma = dense(*blocks[i], K)
        check_block(a, sigma, u[i], s_out[i], vt[i], K, K, K, dtype)  # the reconstruction holds vt to the conjugate phase


@pytest.mark.parametrize("dtype", DTYPES)
def test_phase_rule_on_entries_of_equal_modulus_in_different_chunks(dtype):
    """Left factors of one column built from exact entries in {1, -1, i, -i} in two or three chunks (K = 1, m = 1100: chunks [0, 512),
    [512, 1023), [1023, 1100)): u's column has entries of the same modulus up to rounding in different chunks, and where they come out
    equal to the last bit the earlier row decides.  Either way the first largest entry must be real positive and the others follow it.
    The product by the phase moves the other entries' moduli by up to an ulp, so where numpy's first largest modulus of the output is not
    the real positive entry, that entry must be an earlier or later row of the same modulus to 2 eps."""
    m, n = 1100, 4
    cases = [{3: -1j, 800: 1.0}, {3: 1.0, 800: -1j}, {600: -1.0, 1050: 1j}, {0: -1j, 512: 1.0, 1023: 1j}, {511: 1j, 1099: -1.0}, {3: 1j, 800: 1j}]
    left = np.zeros((len(cases), m, 1), dtype=dtype)
    for i, c in enumerate(cases):
        for row, v in c.items():
            left[i, row, 0] = v
    right = np.zeros((len(cases), 1, n), dtype=dtype)
    right[:, 0, 1] = 1.0
    u, s_out, vt, ranks = recompress_tall(left, right, 1, 0.0)
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


# ---------------------------------------------------------------- 7. symmetries
@pytest.mark.parametrize("dtype", DTYPES)
def test_conjugated_inputs_give_conjugated_outputs_bit_for_bit(dtype):
    rng = np.random.default_rng(65)
    m, n, K, k = 1100, 140, 33, 20
    left, right, mid, s = stack([factors(rng, kind, m, n, K, "both", dtype) for kind in ("gauss", "spectrum", "scaled", "gauss")])
    qs = np.array([K, K, K, 17], dtype=np.int64)
    u, s_out, vt, ranks = recompress_tall(left, right, k, 1e-6, mid, s, qs)
    cu, cs, cvt, cranks = recompress_tall(left.conj(), right.conj(), k, 1e-6, mid.conj(), s, qs)
    assert np.array_equal(cs, s_out) and np.array_equal(cranks, ranks)
    assert np.array_equal(cu, u.conj()) and np.array_equal(cvt, vt.conj())
    # a lazily conjugated tensor is materialised by the Python call
    lazy = cuda(left.conj()).conj()
    assert lazy.is_conj()
    lz = rc.lowrank_recompress_tall_batched_complex(lazy, cuda(right), k, 1e-6, mid=cuda(mid), s=cuda(s), ranks=cuda(qs))
    for v, w in zip((u, s_out, vt, ranks), lz):
        assert np.array_equal(v, npy(w))


@pytest.mark.parametrize("dtype", DTYPES)
def test_zero_imaginary_parts_stay_zero_and_match_the_real_tall_call(dtype):
    rng = np.random.default_rng(66)
    cnt, m, n, K, k = 3, 1100, 90, 20, 20
    rd = real_of(dtype)
    t = TOL[rd]
    blocks = []
    for kind in KINDS:
        lf, rt, md, s = factors(rng, kind, m, n, K, "both", dtype)
        blocks.append((lf.real.astype(dtype), rt.real.astype(dtype), md.real.astype(dtype), s))
    left, right, mid, s = stack(blocks)
    u, s_out, vt, ranks = recompress_tall(left, right, k, 0.0, mid, s)
    assert not np.any(u.imag) and not np.any(vt.imag), "real inputs must give exactly real singular vectors"
    ru, rs, rvt, rranks = (npy(x) for x in rc.lowrank_recompress_tall_batched(cuda(left.real.astype(rd)), cuda(right.real.astype(rd)), k, 0.0,
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


# ---------------------------------------------------------------- 8. the batch contract
def _view(t):
    if t is None:
        return _lib.mat(None), ctypes.c_int64(0)
    return _lib.rc_matrix(t.data_ptr(), t.shape[1], t.shape[2], t.stride(1), t.stride(2)), ctypes.c_int64(t.stride(0))


def _raw(left, mid, s, right, in_ranks, cnt, k, tol, u, ubs, s_out, vt, vbs, ranks, ctx=None, dtype=torch.complex128):
    ctx = ctx or _lib.default_context()
    fn = getattr(_lib.lib(), f"rc_lowrank_recompress_tall_complex_batched_{_lib.suffix(dtype)}")
    tol_arg = ctypes.c_double(tol) if dtype == torch.complex128 else ctypes.c_float(tol)  # tol has the real type of the data
    return fn(ctx._h, *_view(left), *_view(mid), ctypes.c_void_p(s.data_ptr() if s is not None else None),
              ctypes.c_int64(s.stride(0) if s is not None else 0), *_view(right), _lib.i64p(in_ranks), ctypes.c_int32(cnt), ctypes.c_int64(k),
              tol_arg, u, ctypes.c_int64(ubs), ctypes.c_void_p(s_out.data_ptr() if s_out is not None else None), vt, ctypes.c_int64(vbs),
              _lib.i64p(ranks))


def test_bits_independent_of_count_position_and_neighbours():
    rng = np.random.default_rng(61)
    m, n, K, k, tol = 600, 20, 8, 6, 1e-9
    protos = [factors(rng, kind, m, n, K, "both", C64) for kind in ("gauss", "spectrum", "scaled", "gauss", "gauss", "scaled", "gauss")]
    qs = [K, K, 5, 0, 1, K + 2, 3]
    alone = []
    labels = None
    for b, q in zip(protos, qs):
        out, labels = batched_launch(lambda: recompress_tall(b[0][None], b[1][None], k, tol, b[2][None], b[3][None], np.array([q], dtype=np.int64)))
        alone.append(out)
    assert labels["op"] == "batched_recompress_tall<complex>"
    assert (labels["m"], labels["n"], labels["k"], labels["count"], labels["grid"]) == (m, n, K, 1, 1)
    cnt = labels["slots"] + 3  # the last three blocks are some workgroup's second
    pick = [(5 * i + i // 7) % 7 for i in range(cnt)]
    left, right, mid, s = stack([protos[p] for p in pick])
    got, lab = batched_launch(lambda: recompress_tall(left, right, k, tol, mid, s, np.array([qs[p] for p in pick], dtype=np.int64)))
    assert lab["count"] == cnt and lab["grid"] == lab["slots"] and lab["plan"] == labels["plan"]
    for i, p in enumerate(pick):
        for v, w in zip(alone[p], got):
            assert np.array_equal(v[0], w[i]), (i, p)


@pytest.mark.parametrize("dtype", DTYPES)
def test_input_views_give_the_same_bits(dtype):
    rng = np.random.default_rng(62)
    cnt, m, n, K, k = 4, 1100, 50, 12, 9
    left, right, mid, s = (cuda(x) for x in stack([factors(rng, "gauss", m, n, K, "both", dtype) for _ in range(cnt)]))
    ref = tuple(npy(x) for x in rc.lowrank_recompress_tall_batched_complex(left, right, k, 1e-6, mid=mid, s=s))

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
        got = rc.lowrank_recompress_tall_batched_complex(f(left), f(right), k, 1e-6, mid=f(mid), s=spad)
        for v, w in zip(ref, got):
            assert np.array_equal(v, npy(w)), f.__name__
    shared = right[2:3].expand(cnt, K, n)  # right_batch_stride = 0
    assert shared.stride(0) == 0
    got = rc.lowrank_recompress_tall_batched_complex(left, shared, k, 1e-6, mid=mid, s=s)
    one = rc.lowrank_recompress_tall_batched_complex(left[2:3], right[2:3], k, 1e-6, mid=mid[2:3], s=s[2:3])
    for v, w, x in zip(ref, got, one):
        assert np.array_equal(v[2], npy(w)[2]) and np.array_equal(v[2], npy(x)[0])


def test_strided_outputs_leave_the_gaps_untouched():
    rng = np.random.default_rng(63)
    cnt, m, n, K, k = 4, 1100, 40, 14, 10
    left, right, mid, s = (cuda(x) for x in stack([factors(rng, "gauss", m, n, K, "mid", C64) for _ in range(cnt)]))
    # ranks below k in two blocks, so that zero columns are written through the strided views too
    in_ranks = cuda(np.array([K, 4, K, 7], dtype=np.int64))
    ref = tuple(npy(x) for x in rc.lowrank_recompress_tall_batched_complex(left, right, k, 1e-3, mid=mid, ranks=in_ranks))
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
    # u row-major with a padded row: the chunks of a column are written and re-read for the phase through the row stride
    up = torch.full((cnt, m, k + 3), 7.0, dtype=left.dtype, device=left.device)
    vt = torch.zeros((cnt, k, n), dtype=left.dtype, device=left.device)
    assert _raw(left, mid, None, right, in_ranks, cnt, k, 1e-3, _lib.rc_matrix(up.data_ptr(), m, k, k + 3, 1), m * (k + 3), s_out, _lib.mat(vt[0]), k * n,
                ranks) == 0
    torch.cuda.synchronize()
    assert np.array_equal(npy(up)[:, :, :k], ref[0]) and np.all(npy(up)[:, :, k:] == 7.0) and np.array_equal(npy(vt), ref[2])


def test_graph_capture_replays_the_eager_bits():
    rng = np.random.default_rng(64)
    cnt, m, n, K, k = 6, 600, 128, 24, 16
    lib = _lib.lib()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        left, right, mid, s = (cuda(x) for x in stack([factors(rng, "gauss", m, n, K, "both", C64) for _ in range(cnt)]))
        in_ranks = cuda(rng.integers(0, K + 1, cnt).astype(np.int64))
        eager = tuple(npy(x) for x in rc.lowrank_recompress_tall_batched_complex(left, right, k, 1e-9, mid=mid, s=s, ranks=in_ranks))
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
    u, s, vt, r = rc.lowrank_recompress_tall_batched_complex(e(0, 600, 8), e(0, 8, 20), 5)
    assert u.shape == (0, 600, 5) and s.shape == (0, 8) and vt.shape == (0, 5, 20) and r.shape == (0,)
    assert u.dtype == torch.complex64 and s.dtype == torch.float32


@pytest.mark.parametrize("dtype", DTYPES)
def test_nan_stays_in_its_block(dtype):
    rng = np.random.default_rng(71)
    cnt, m, n, K, k = 6, 600, 70, 30, 20
    left, right, mid, s = stack([factors(rng, "gauss", m, n, K, "both", dtype) for _ in range(cnt)])
    ref = recompress_tall(left, right, k, 1e-5, mid, s)
    left, right, mid, s = left.copy(), right.copy(), mid.copy(), s.copy()
    left[4, 590, 3] = np.nan  # in the second stage's rows
    right[1, 5, :] = np.inf
    mid[2, 1, 1] = complex(0.0, np.nan)
    got = recompress_tall(left, right, k, 1e-5, mid, s)
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
    m, n, K = 1100, 130, 128
    rd = real_of(dtype)
    blocks = [factors(rng, kind, m, n, K, "both", dtype) for kind in KINDS]
    clustered = np.concatenate([np.ones(10), 0.5 * np.ones(40), 1e-3 * (1 + 1e-9 * np.arange(78))])
    blocks.append((orthonormal(rng, m, K).astype(dtype), orthonormal(rng, n, K).conj().T.astype(dtype), np.eye(K, dtype=dtype), clustered.astype(rd)))
    left, right, mid, s = stack(blocks)
    u, s_out, vt, ranks = recompress_tall(left, right, 64, 0.0, mid, s)
    ctx.synchronize()
    assert ctx.get_health() == 0
    for i, b in enumerate(blocks):
        a, sigma = dense(*b, K)
        assert ranks[i] == 64
        check_block(a, sigma, u[i], s_out[i], vt[i], 64, K, 64, dtype)


# ---------------------------------------------------------------- 9. a wide pair is the plain transpose
@pytest.mark.parametrize("dtype", DTYPES)
def test_wide_pairs_through_transposed_views(dtype):
    """A = left mid diag(s) right with a tall right factor (n = 1100): A^T = right^T (mid diag(s))^T left^T, so the call takes right^T, the
    transposed core and left^T as strided views.  With A = U S V^H and nothing conjugated in the product, A^T = conj(V) S U^T: the call's u
    is conj(V) = vt(A)^T and its vt is U^T, plain transposes with no conjugation anywhere.  diag(s) moves to the other side of mid under
    the transposition, so the scales are folded into mid here."""
    rng = np.random.default_rng(91)
    m, n, K, k = 40, 1100, 16, 12
    blocks = [factors(rng, kind, m, n, K, "both", dtype) for kind in KINDS]
    left, right, mid, s = (cuda(x) for x in stack(blocks))
    core = mid * s[:, None, :]
    out = rc.lowrank_recompress_tall_batched_complex(right.mT, left.mT, k, 0.0, mid=core.mT)
    v, s_out, ut, ranks = (npy(x) for x in out)
    torch.cuda.synchronize()
    for i in range(3):
        a, sigma = dense(*blocks[i], K)
        assert ranks[i] == k
        check_block(a.T, sigma, v[i], s_out[i], ut[i], k, K, k, dtype)  # the oracle on A^T (the plain transpose): the phase rule holds on its u
        # and read back as factors of A itself: U = ut^T, Vt = v^T
        rec = (ut[i].T.astype(C64) * s_out[i][:k].astype(np.float64)) @ v[i].T.astype(C64)
        tail = np.linalg.svd(a, compute_uv=False)[k]
        assert np.linalg.norm(a - rec, 2) <= 4 * TOL[real_of(dtype)]["recon"] * sigma + tail


# ---------------------------------------------------------------- 10. the wrappers
@pytest.mark.parametrize("dtype", DTYPES)
def test_sketched_ids_convert_to_svds_and_the_chain_is_the_two_calls(dtype):
    rng = np.random.default_rng(101)
    cnt, m, n, k, r0 = 3, 1100, 96, 16, 9
    tol = 1e-8 if dtype == C64 else 1e-4
    exact = np.stack([gaussian(rng, m, r0) @ gaussian(rng, r0, n) for _ in range(cnt)]).astype(dtype)
    decay = np.stack([(gaussian(rng, m, 40) * 2.0 ** -np.arange(40)) @ gaussian(rng, 40, n) for _ in range(cnt)]).astype(dtype)
    for a_np, run_tol in ((exact, tol), (decay, 0.0)):
        a = cuda(a_np)
        c, z, _, ranks = rc.sketch_column_id_rank_batched_complex(a, k, run_tol, oversampling=8, seed=7)  # l = 24 rows of omega
        u, s_out, vt, rk = rc.column_id_to_svd_tall_batched_complex(c, z, ranks, k, run_tol)
        chain = rc.sketch_svd_rank_batched_complex(a, k, run_tol, oversampling=8, seed=7)
        for v, w in zip((u, s_out, vt, rk), chain):
            assert torch.equal(v, w)
        torch.cuda.synchronize()
        for i in range(cnt):
            q = int(ranks[i])
            print(f"  block {i} q={q} {np.dtype(dtype).name}")
            prod, sigma = dense(npy(c)[i], npy(z)[i], None, None, q)
            check_block(prod, sigma, npy(u)[i], npy(s_out)[i], npy(vt)[i], int(rk[i]), q, k, dtype)
        if a_np is exact:
            assert list(npy(ranks)) == [r0] * cnt and list(npy(rk)) == [r0] * cnt


# ---------------------------------------------------------------- 11. the label, the arguments
@pytest.mark.parametrize("m,n,K", [(513, 40, 8), (1100, 130, 128), (2100, 64, 64), (300, 64, 16)])
def test_label_shows_the_stages(m, n, K):
    rng = np.random.default_rng(m)
    blocks = [factors(rng, "gauss", m, n, K, "s", C32) for _ in range(3)]
    left, right, mid, s = stack(blocks)
    _, lab = batched_launch(lambda: recompress_tall(left, right, K, 0.0, mid, s))
    assert lab["op"] == "batched_recompress_tall<complex>" and (lab["m"], lab["n"], lab["k"], lab["count"], lab["grid"]) == (m, n, K, 3, 3)
    fields = lab["plan"].split(",")
    assert fields[0] == f"stages={stages(m, K)}", lab["plan"]
    assert fields[1] == ("L:ws" if m > H else fields[1]) and fields[-1] == "s" and f"kk={K}" in fields
    assert [f[:2] for f in fields[1:5]] == ["L:", "R:", "V:", "G:"]
    # the 2 GiB bound on the workspace does not bind at these sizes: the family's grid rule stands
    sg, slot, grid = (ctypes.c_int64(0) for _ in range(3))
    assert _lib.lib().rc_lowrank_recompress_tall_complex_batched_plan(ctypes.c_int64(m), ctypes.c_int64(n), ctypes.c_int64(K), ctypes.c_int32(4),
                                                                    ctypes.c_int64(lab["slots"]), ctypes.byref(sg), ctypes.byref(slot),
                                                                    ctypes.byref(grid)) == 0
    assert sg.value == stages(m, K) and grid.value == lab["slots"]
    if m <= H:  # one stage: the existing call's plan
        _, old = batched_launch(lambda: tuple(npy(x) for x in rc.lowrank_recompress_batched_complex(cuda(left), cuda(right), K, 0.0, s=cuda(s))))
        assert lab["plan"] == "stages=1," + old["plan"]


def test_argument_checks():
    e = lambda c, r, q: torch.zeros((c, r, q), dtype=torch.complex128, device="cuda")  # noqa: E731
    sbuf = torch.zeros((2, 600), dtype=torch.float64, device="cuda")
    ranks = torch.zeros(2, dtype=torch.int64, device="cuda")

    def call(left, right, k, tol, u, ubs, vt, vbs, mid=None, cnt=2, s_out=sbuf, rk=ranks):
        return _raw(left, mid, None, right, None, cnt, k, tol, _lib.mat(u[0]) if u is not None else _lib.mat(None), ubs, s_out,
                    _lib.mat(vt[0]) if vt is not None else _lib.mat(None), vbs, rk)

    def message():
        return _lib.lib().rc_last_error_message(_lib.default_context()._h).decode()

    lf, rt, u, vt = e(2, 700, 16), e(2, 16, 100), e(2, 700, 8), e(2, 8, 100)
    assert call(lf, rt, 8, 0.0, u, 5600, vt, 800) == 0                                             # the valid call the rest departs from
    assert call(e(2, 513, 16), rt, 8, 0.0, e(2, 513, 8), 4104, vt, 800) == 0                       # m = 513: the first row past the existing call
    big = torch.zeros((1, 65537, 16), dtype=torch.complex128, device="cuda")
    ubig = torch.zeros((1, 65537, 8), dtype=torch.complex128, device="cuda")
    assert call(big[:, :65536], rt[:1], 8, 0.0, ubig[:, :65536], 65536 * 8, vt[:1], 800, cnt=1) == 0        # m = 65536
    assert call(big, rt[:1], 8, 0.0, ubig, 65537 * 8, vt[:1], 800, cnt=1) == INVALID               # m = 65537
    assert message().startswith("lowrank_recompress_tall_complex_batched") and "65536" in message()
    assert call(lf, e(2, 16, 513), 8, 0.0, u, 5600, e(2, 8, 513), 4104) == INVALID                # n = 513
    assert message().startswith("lowrank_recompress_tall_complex_batched")
    assert call(e(2, 700, 129), e(2, 129, 200), 8, 0.0, u, 5600, e(2, 8, 200), 1600) == INVALID   # K = 129
    assert message().startswith("lowrank_recompress_tall_complex_batched")
    assert call(lf, e(2, 16, 12), 8, 0.0, u, 5600, e(2, 8, 12), 96) == INVALID                     # K > min(m, n)
    assert message().startswith("lowrank_recompress_tall_complex_batched") and "rc_svd_rank_batched" in message()
    assert call(lf, e(2, 15, 100), 8, 0.0, u, 5600, vt, 800) == INVALID                           # left.cols != right.rows
    assert call(lf, rt, 8, 0.0, u, 5600, vt, 800, mid=e(2, 16, 15)) == INVALID                    # mid not K x K
    assert call(lf, rt, 0, 0.0, e(2, 700, 1), 700, e(2, 1, 100), 100) == INVALID                  # k < 1
    assert call(lf, rt, 8, 1.0, u, 5600, vt, 800) == INVALID                                      # tol = 1, as the existing complex call
    assert call(lf, rt, 8, -1e-3, u, 5600, vt, 800) == INVALID                                    # tol < 0
    assert call(lf, rt, 8, 0.0, u, 5599, vt, 800) == INVALID                                      # a short batch stride of u
    assert call(lf, rt, 8, 0.0, u, 5600, vt, 799) == INVALID                                      # and of vt
    assert call(lf, rt, 8, 0.0, e(2, 700, 7), 4900, vt, 800) == INVALID                           # u not m x kk
    assert message().startswith("lowrank_recompress_tall_complex_batched")
    assert call(lf, rt, 8, 0.0, e(2, 699, 8), 5592, vt, 800) == INVALID
    assert call(lf, rt, 8, 0.0, u, 5600, e(2, 8, 99), 792) == INVALID                             # vt not kk x n
    assert call(lf, rt, 8, 0.0, u, 5600, vt, 800, cnt=-1) == INVALID                              # count < 0
    assert call(lf, rt, 8, 0.0, u, 5600, vt, 800, s_out=None) == INVALID                          # null outputs
    assert message().startswith("lowrank_recompress_tall_complex_batched")
    assert call(lf, rt, 8, 0.0, u, 5600, vt, 800, rk=None) == INVALID
    assert call(lf, rt, 8, 0.0, None, 5600, vt, 800) == INVALID
    assert call(lf, rt, 8, 0.0, u, 5600, None, 800) == INVALID
    assert call(lf, rt, 8, 0.0, u, 5600, vt, 800, cnt=0) == 0                                     # count = 0: nothing to do
    # the c32 entry point takes its tol as a float
    c32 = lambda c, r, q: torch.zeros((c, r, q), dtype=torch.complex64, device="cuda")  # noqa: E731
    s32 = torch.zeros((2, 16), dtype=torch.float32, device="cuda")
    args32 = (c32(2, 700, 16), None, None, c32(2, 16, 100), None, 2, 8)
    outs32 = (_lib.mat(c32(2, 700, 8)[0]), 5600, s32, _lib.mat(c32(2, 8, 100)[0]), 800, ranks)
    assert _raw(*args32, 0.5, *outs32, dtype=torch.complex64) == 0
    assert _raw(*args32, 1.0, *outs32, dtype=torch.complex64) == INVALID
    torch.cuda.synchronize()
    # the real tall name keeps refusing complex data; the complex names refuse real data and mixed dtypes
    for bad in (torch.complex128, torch.complex64):
        z = lambda *shape: torch.zeros(shape, dtype=bad, device="cuda")  # noqa: E731
        with pytest.raises(TypeError):
            rc.lowrank_recompress_tall_batched(z(1, 600, 4), z(1, 4, 8), 2)
        with pytest.raises(TypeError):
            rc.sketch_svd_rank_batched(z(1, 600, 8), 2)
    for bad in (torch.float64, torch.float32):
        z = lambda *shape: torch.zeros(shape, dtype=bad, device="cuda")  # noqa: E731
        with pytest.raises(TypeError):
            rc.lowrank_recompress_tall_batched_complex(z(1, 600, 4), z(1, 4, 8), 2)
        with pytest.raises(TypeError):
            rc.column_id_to_svd_tall_batched_complex(z(1, 600, 4), z(1, 4, 8), None, 2)
        with pytest.raises(TypeError):
            rc.svd_add_tall_batched_complex(*[z(1, 600, 2), z(1, 2), z(1, 2, 8)] * 2, 2)
        with pytest.raises(TypeError):
            rc.sketch_svd_rank_batched_complex(z(1, 600, 8), 2)
    with pytest.raises(TypeError):
        rc.lowrank_recompress_tall_batched_complex(e(1, 600, 4), e(1, 4, 8).to(torch.complex64), 2)                   # mixed complex dtypes
    with pytest.raises(TypeError):
        rc.lowrank_recompress_tall_batched_complex(e(1, 600, 4), e(1, 4, 8), 2, s=torch.zeros((1, 4), dtype=torch.complex128, device="cuda"))
    with pytest.raises(AssertionError, match="lowrank_recompress_tall_complex_batched"):  # RC_INVALID_ARGUMENT: the reference asserts
        rc.lowrank_recompress_tall_batched_complex(e(1, 600, 16), e(1, 16, 12), 4)
