"""GPU parity tests (run with -m gpu on an MI355X): every call goes through the
C ABI (librusty_compression_amd.so) and is compared with

  * the committed golden vectors (tests/golden/, SciPy-LAPACK oracle),
  * the oracle run live on the same seeded inputs,
  * the reference's own property tests, restated (file:line cited per test).

Tolerances (tests/helpers.py TOL): f64 factors <= 1e-10 relative Frobenius,
singular values <= 1e-12 relative; f32 1e-4 / 1e-5.  Permutation indices are
compared bit-exactly on the prefix that is determined by the data (helpers.stable_prefix).
"""
import ctypes

import numpy as np
import pytest
import torch

import rusty_compression_amd as rc
from oracle import ref_lapack as o
from tests.dense_scale_cases import check_pivoted_qr_real, check_truncated_qr_real
from tests.gemm_cases import GEMM_DISPATCH, gemm_operand, last_gemm_kernel
from tests.helpers import TOL, agreed_pivot_prefix, golden, greedy_pivot_slack, is_permutation, npy, rel, sign_normalise, stable_prefix

pytestmark = pytest.mark.gpu

QRCP_FILES = [f"qrcp_{t}_{s}_{g}.npz" for t in ("f64", "f32") for s in ("thin", "thick") for g in ("s5", "s10")]
CT = rc.CompressionType


def test_native_library_is_the_one_loaded():
    from rusty_compression_amd import _lib

    assert torch.cuda.is_available()
    assert _lib.lib().rc_abi_version() == 1
    with open("/proc/self/maps") as f:
        assert "librusty_compression_amd.so" in f.read()


# ---------------------------------------------------------------- GEMM (a2, a3, N9)
@pytest.mark.parametrize("dtype,tol", [(np.float64, 1e-13), (np.float32, 2e-6)])
def test_gemm_all_layouts_and_ragged_shapes(dtype, tol):
    rng = np.random.default_rng(0)
    for (m, k, n) in ((100, 50, 37), (256, 512, 133), (128, 1000, 300), (33, 7, 5), (300, 260, 69), (1, 64, 1), (513, 129, 257), (5, 1, 9), (160, 2100, 128)):
        a = rng.standard_normal((m, k)).astype(dtype)
        b = rng.standard_normal((k, n)).astype(dtype)
        ref = a.astype(np.float64) @ b.astype(np.float64)
        for la in ("C", "F"):
            for lb in ("C", "F"):
                ta = torch.from_numpy(a).cuda() if la == "C" else torch.from_numpy(np.ascontiguousarray(a.T)).cuda().t()
                tb = torch.from_numpy(b).cuda() if lb == "C" else torch.from_numpy(np.ascontiguousarray(b.T)).cuda().t()
                assert rel(npy(rc.dot(ta, tb)), ref) <= tol, (m, k, n, la, lb)
    # strided sub-views (neither operand starts at an aligned address, odd leading dimension)
    big = rng.standard_normal((70, 91)).astype(dtype)
    tb = torch.from_numpy(big).cuda()
    assert rel(npy(rc.dot(tb[3:45, 5:60], tb[1:56, 7:40])), big[3:45, 5:60].astype(np.float64) @ big[1:56, 7:40].astype(np.float64)) <= tol
    # matrix . vector (Apply on Ix1, col_interp_decomp.rs:134-143)
    v = rng.standard_normal(91).astype(dtype)
    assert rel(npy(rc.dot(tb, v)), big.astype(np.float64) @ v.astype(np.float64)) <= tol
    # matmat / conj_matmat (types.rs:58-101)
    x = rng.standard_normal((91, 12)).astype(dtype)
    y = rng.standard_normal((70, 12)).astype(dtype)
    assert rel(npy(rc.matmat(big, x)), big.astype(np.float64) @ x) <= tol
    assert rel(npy(rc.conj_matmat(big, y)), big.T.astype(np.float64) @ y) <= tol


def test_gemm_dispatch_launches_the_expected_instantiation():
    rng = np.random.default_rng(4)
    wrong = []
    for dt, la, lb, m, n, k, want in GEMM_DISPATCH:
        dtype, tol = (np.float64, 1e-13) if dt == "f64" else (np.float32, 2e-6)
        a = rng.standard_normal((m, k)).astype(dtype)
        b = rng.standard_normal((k, n)).astype(dtype)
        out = rc.dot(gemm_operand(a, la), gemm_operand(b, lb))
        got = last_gemm_kernel()
        if got != want:
            wrong.append((dt, la, lb, m, n, k, got, want))
        assert rel(npy(out), a.astype(np.float64) @ b.astype(np.float64)) <= tol, (dt, la, lb, m, n, k)
    assert not wrong, "\n".join(map(str, wrong))


def test_f64_gemm_hand_ordered_loops_on_their_shapes():
    """k_gemm_f64r (three-stage LDS ring, copies inside the MFMA stream, hand-ordered main loop, direct-to-LDS copies, masked
    tail copy) on the shapes that reach it -- 129..136 rows over a K-contiguous wide operand (the sketch as the transposed
    problem) and <= 128 rows over an N-contiguous one (the projection) -- around its preconditions: row counts that clamp, one
    K tile, K tiles that split, wide / narrow N, plus neighbours that must fall back to k_gemm_f64p / k_gemm_f64q (K not a
    multiple of 16, N not a multiple of the tile, shallow K over a wide N)."""
    rng = np.random.default_rng(5)
    sketch_ring = "k_gemm_f64r<1,0,136,256,2,4,true,0>"
    projection_ring = "k_gemm_f64r<0,1,128,256,1,8,false,0>"
    for m in (129, 133, 136, 128, 97, 130):
        for n in (256, 512, 768, 2048, 300):
            for k in (16, 48, 1024, 2080, 40):
                a = rng.standard_normal((m, k))
                b = rng.standard_normal((k, n))
                ref = a @ b
                # the ring kernel takes whole 16-deep K tiles; shallow products over a wide N get 128-column tiles instead
                ring = k % 16 == 0 and not (k <= 160 and n >= 2048)
                # sketch layout: A stored (k x m) with even leading dimension (M-contiguous), B stored (n x k) (K-contiguous)
                ta = torch.zeros((k, m + (m & 1)), dtype=torch.float64, device="cuda")[:, :m]
                ta.copy_(torch.from_numpy(np.ascontiguousarray(a.T)))
                tb = torch.from_numpy(np.ascontiguousarray(b.T)).cuda()
                assert rel(npy(rc.dot(ta.t(), tb.t())), ref) <= 1e-13, ("sketch layout", m, n, k)
                got = last_gemm_kernel()
                if ring and m > 128 and n % 256 == 0:
                    assert got == sketch_ring, ("sketch layout", m, n, k, got)
                else:
                    assert got.startswith(("k_gemm_f64p<", "k_gemm_f64q<")), ("sketch layout", m, n, k, got)
                # projection layout: A M-contiguous as above, B stored (k x n) (N-contiguous)
                tb2 = torch.from_numpy(b).cuda()
                assert rel(npy(rc.dot(ta.t(), tb2)), ref) <= 1e-13, ("projection layout", m, n, k)
                got = last_gemm_kernel()
                if ring and m <= 128:
                    assert got == projection_ring, ("projection layout", m, n, k, got)
                else:
                    assert got.startswith(("k_gemm_f64p<", "k_gemm_f64q<")), ("projection layout", m, n, k, got)


def test_gemm_is_deterministic_under_split_k():
    a = rc.random_gaussian((512, 8192), rc.Rng(1))
    b = rc.random_gaussian((8192, 69), rc.Rng(2))
    c1 = rc.dot(a, b)
    c2 = rc.dot(a, b)
    assert torch.equal(c1, c2)
    assert rel(npy(c1), npy(a) @ npy(b)) <= 1e-13


# ---------------------------------------------------------------- permutation (a17)
def test_permutation_known_answers_of_the_reference():
    g = golden("perm_known.npz")  # values of src/permutation.rs:192-239
    for mode in ("COL", "COLINV", "ROW", "ROWINV"):
        assert np.array_equal(npy(rc.apply_permutation(g["mat"], g["perm"], rc.MatrixPermutationMode[mode])), g[mode])
        assert np.array_equal(npy(rc.apply_permutation(g["mat"].astype(np.float32), g["perm"], rc.MatrixPermutationMode[mode])), g[mode])
    assert np.array_equal(npy(rc.apply_permutation(g["vec"], g["perm"], rc.VectorPermutationMode.NOINV)), g["NOINV"])
    assert np.array_equal(npy(rc.apply_permutation(g["vec"], g["perm"], rc.VectorPermutationMode.INV)), g["INV"])
    assert npy(rc.invert_permutation_vector(g["perm"])).tolist() == [1, 2, 0]


def test_permutation_random_and_length_asserts():
    rng = np.random.default_rng(3)
    a = rng.standard_normal((37, 53))
    pc, pr = rng.permutation(53), rng.permutation(37)
    for mode, p in (("COL", pc), ("COLINV", pc), ("ROW", pr), ("ROWINV", pr)):
        assert np.array_equal(npy(rc.apply_permutation(a, p, rc.MatrixPermutationMode[mode])), o.apply_permutation_matrix(a, p, mode))
    with pytest.raises(AssertionError):  # src/permutation.rs:96-99
        rc.apply_permutation(a, pr, rc.MatrixPermutationMode.COL)
    with pytest.raises(AssertionError):
        rc.apply_permutation(a[:, 0].copy(), pc, rc.VectorPermutationMode.INV)


# ---------------------------------------------------------------- Gaussian fill (a1)
def test_gaussian_stream_matches_the_philox_oracle_bit_for_bit():
    """k_fill_gaussian against oracle/philox.py (pinned to Random123's known answers on the CPU side) and the committed
    golden: uint32 words bit-exact, normals within 4 ulp of the correctly rounded Box-Muller value, f32 = cast of f64."""
    from oracle import philox as ph

    g = golden("philox_stream.npz")
    for i, (seed, off) in enumerate(g["pairs"]):
        seed, off = int(seed), int(off)
        w = npy(rc.random_bits_u32(4096, seed, off)).astype(np.uint32)
        assert np.array_equal(w, g[f"words_{i}"]), "Philox4x32-10 word stream differs from the golden"
        z = npy(rc.random_gaussian((64, 64), rc.Rng(seed, off)))
        ref = g[f"normals_{i}"].reshape(64, 64)
        ulp = np.abs(z - ref) / np.spacing(np.abs(ref))
        assert ulp.max() <= 4.0, f"normals differ by {ulp.max()} ulp"
        z32 = npy(rc.random_gaussian((64, 64), rc.Rng(seed, off), torch.float32))
        assert np.array_equal(z32, z.astype(np.float32))  # drawn in f64 then cast (random_matrix.rs:123)
    # live oracle at a ragged shape, odd offset, words across a block boundary
    for (seed, off, shape) in ((3, 1, (37, 53)), (2 ** 63 + 5, 2 ** 33 + 7, (5, 1)), (9, 0, (1, 1))):
        z = npy(rc.random_gaussian(shape, rc.Rng(seed, off)))
        ref = ph.random_gaussian(shape, seed, off)
        assert (np.abs(z - ref) <= 4.0 * np.spacing(np.abs(ref))).all()
    assert np.array_equal(npy(rc.random_bits_u32(11, 5, 2 ** 34 + 3)).astype(np.uint32), ph.words(5, 2 ** 34 + 3, 11))
    assert np.array_equal(npy(rc.random_bits_u32(3, 0, 0)).astype(np.uint32), g["kat_out"][0][:3])  # Random123 KAT (zero key, zero counter)


def test_gaussian_stream_is_counter_based_and_normal():
    from scipy import stats

    g = npy(rc.random_gaussian((4096, 133), rc.Rng(7)))
    assert stats.kstest(g.reshape(-1), "norm").pvalue > 1e-3
    edges = stats.norm.ppf(np.linspace(0, 1, 65)[1:-1])
    cnt = np.bincount(np.searchsorted(edges, g.reshape(-1)), minlength=64)
    assert stats.chisquare(cnt).pvalue > 1e-3
    r1 = rc.Rng(7)
    a, b = npy(rc.random_gaussian((10, 7), r1)), npy(rc.random_gaussian((5, 7), r1))
    assert np.array_equal(np.vstack([a, b]), npy(rc.random_gaussian((15, 7), rc.Rng(7))))  # consumption order = row-major
    assert not np.array_equal(a, npy(rc.random_gaussian((10, 7), rc.Rng(8))))


# ---------------------------------------------------------------- pivoted QR / LQ (a5, a6)
@pytest.mark.parametrize("name", QRCP_FILES)
def test_pivoted_qr_and_lq_match_golden(name):
    g = golden(name)
    a = g["a"]
    tol = TOL[a.dtype]
    q, r, ind = (npy(t) for t in rc.pivoted_qr(a))
    ns = agreed_pivot_prefix(ind, r, g["ind"], g["r"], a.dtype)
    assert is_permutation(ind, a.shape[1]) and ns >= 15
    if a.dtype == np.float64:
        assert ns == stable_prefix(g["r"], a.dtype)  # f64: bit-exact permutation on everything the data determines
    assert rel(r[:ns, :ns], g["r"][:ns, :ns]) <= tol["factor"]
    assert rel(o.apply_permutation_matrix(r[:ns], ind, "COLINV"), o.apply_permutation_matrix(g["r"][:ns], g["ind"], "COLINV")) <= tol["factor"]
    if name.endswith("s5.npz") and ns == stable_prefix(g["r"], a.dtype):  # cond ~1e5: Q is determined to ~cond * eps
        assert rel(q, g["q"]) <= (1e-9 if a.dtype == np.float64 else 5e-2)
    # the reference's own assertions (src/pivoted_qr.rs:225-242): orthogonality and column match, 1e-6
    assert np.abs(q.T @ q - np.eye(q.shape[1])).max() < 1e-6
    prod = q @ r
    for j in range(a.shape[1]):
        assert np.linalg.norm(prod[:, j] - a[:, ind[j]]) < 1e-6 * max(np.linalg.norm(a[:, ind[j]]), 1e-30) or np.linalg.norm(a[:, ind[j]]) < 1e-5
    l, ql, indl = (npy(t) for t in rc.pivoted_lq(a))
    nsl = agreed_pivot_prefix(indl, l, g["indl"], g["l"], a.dtype)
    assert is_permutation(indl, a.shape[0]) and nsl >= 15
    if a.dtype == np.float64:
        assert nsl == stable_prefix(g["l"], a.dtype)
    assert rel(l[:nsl, :nsl], g["l"][:nsl, :nsl]) <= tol["factor"]
    assert np.abs(ql @ ql.T - np.eye(ql.shape[0])).max() < 1e-6  # src/pivoted_qr.rs:273-281
    prod = l @ ql
    for i in range(a.shape[0]):
        assert np.linalg.norm(prod[i] - a[indl[i]]) < 1e-6 * max(np.linalg.norm(a[indl[i]]), 1e-30) or np.linalg.norm(a[indl[i]]) < 1e-5


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("shape", [(512, 69), (64, 512), (300, 300), (2100, 40), (17, 1), (1, 17), (9000, 6)])
def test_pivoted_qr_shapes_against_live_oracle(dtype, shape):
    rng = np.random.default_rng(shape[0] * 7 + shape[1])
    a = o.random_approximate_low_rank_matrix(shape, 1.0, 1e-5, rng, dtype) if min(shape) > 1 else rng.standard_normal(shape).astype(dtype)
    gq, gr, gi = (npy(t) for t in rc.pivoted_qr(a))
    check_pivoted_qr_real(a, gq, gr, gi, o.pivoted_qr(a))


@pytest.mark.parametrize("n", [8, 33, 64, 65, 100, 133, 160, 161, 224])
def test_tall_pivoted_qr_across_the_register_tile_variants(n):
    """4096 x n Gaussian, f64: the tall-skinny path (CholeskyQR2 + small QRCP + sign fix) switches register tilings at
    n = 64 / 144 / 160 (k_chol_inv, k_qrcp_small) and leaves the fast path above its limits; pivots identical to
    ?geqp3, Q, R with LAPACK's signs to 1e-12, Q orthonormal to 1e-13 at every size."""
    rng = np.random.default_rng(1000 + n)
    a = rng.standard_normal((4096, n))
    q, r, ind = o.pivoted_qr(a)
    gq, gr, gi = (npy(t) for t in rc.pivoted_qr(a))
    assert np.array_equal(gi, ind)
    assert rel(gr, r) <= 1e-12 and rel(gq, q) <= 1e-12
    assert np.abs(gq.T @ gq - np.eye(n)).max() <= 1e-13


def test_pivoted_qr_accepts_any_layout_and_leaves_input_untouched():
    rng = np.random.default_rng(9)
    a = o.random_approximate_low_rank_matrix((120, 80), 1.0, 1e-5, rng)
    ref = o.pivoted_qr(a)
    t_c = torch.from_numpy(a).cuda()
    t_f = torch.from_numpy(np.ascontiguousarray(a.T)).cuda().t()
    big = torch.zeros((130, 95), dtype=torch.float64, device="cuda")
    big[5:125, 10:90] = t_c
    for t in (t_c, t_f, big[5:125, 10:90]):
        before = t.clone()
        q, r, ind = rc.pivoted_qr(t)
        assert torch.equal(t, before)
        assert np.array_equal(npy(ind), ref[2]) and rel(npy(r), ref[1]) <= 1e-10


def test_truncated_pivoted_qr_equals_the_leading_part_of_the_full_one():
    rng = np.random.default_rng(12)
    for dtype in (np.float64, np.float32):
        a = o.random_approximate_low_rank_matrix((200, 120), 1.0, 1e-5, rng, dtype)
        gq, gr, gi = (npy(t) for t in rc.pivoted_qr(a, rank=30))
        check_truncated_qr_real(a, gq, gr, gi, 30, o.pivoted_qr(a))


def test_pivot_ties_take_the_first_maximum_like_idamax():
    # duplicate and zero columns: exact ties in the partial norms
    rng = np.random.default_rng(4)
    base = rng.standard_normal((40, 6))
    a = np.concatenate([base, base, np.zeros((40, 3)), base[:, :2]], axis=1)
    q, r, ind = o.pivoted_qr(a)
    gq, gr, gi = (npy(t) for t in rc.pivoted_qr(a))
    assert np.array_equal(gi[:6], ind[:6])
    assert rel(gq @ gr, a[:, gi]) <= 1e-13
    z = np.zeros((8, 5))
    gq, gr, gi = (npy(t) for t in rc.pivoted_qr(z))
    assert gi.tolist() == [0, 1, 2, 3, 4] and np.all(gr == 0) and np.array_equal(gq, np.eye(8, 5))


# ---------------------------------------------------------------- SVD (a11, a12)
@pytest.mark.parametrize("name", QRCP_FILES)
def test_compute_svd_matches_golden(name):
    g = golden(name)
    a = g["a"]
    tol = TOL[a.dtype]
    u, s, vt = (npy(t) for t in rc.compute_svd(a))
    assert np.abs(s - g["s"]).max() / g["s"][0] <= tol["sval"]
    assert np.all(np.diff(s) <= 0)
    assert rel(u @ np.diag(s) @ vt, a) <= tol["recon"]
    assert np.abs(u.T @ u - np.eye(len(s))).max() <= (1e-12 if a.dtype == np.float64 else 1e-4)
    assert np.abs(vt @ vt.T - np.eye(len(s))).max() <= (1e-12 if a.dtype == np.float64 else 1e-4)
    # singular vectors of well separated, well conditioned singular values, after fixing the pair signs
    un, vtn = sign_normalise(u, vt)
    lead = 10
    assert rel(un[:, :lead], g["u"][:, :lead]) <= (1e-9 if a.dtype == np.float64 else 1e-3)
    assert rel(vtn[:lead], g["vt"][:lead]) <= (1e-9 if a.dtype == np.float64 else 1e-3)


@pytest.mark.parametrize("dtype,shape,tol", [(np.float64, (100, 50), 1e-12), (np.float32, (100, 50), 1e-5), (np.float64, (50, 100), 1e-12), (np.float32, (50, 100), 1e-5)])
def test_svd_reference_properties(dtype, shape, tol):
    """src/svd.rs:214-223 (SVD -> QR -> matrix), :246-253 (RANK(20)), :277-281 (ADAPTIVE)."""
    rng = np.random.default_rng(21)
    a = o.random_approximate_low_rank_matrix(shape, 1.0, 1e-10, rng, dtype)
    svd = rc.SVD.compute_from(a)
    assert rc.rel_diff_fro(svd.to_qr().to_mat(), a) < tol
    c = svd.compress(CT.RANK(20))
    assert c.u.shape[1] == 20 and c.vt.shape[0] == 20
    assert rc.rel_diff_fro(c.to_mat(), a) < 1e-4
    ad = svd.compress(CT.ADAPTIVE(1e-4))
    assert rc.rel_diff_fro(ad.to_mat(), a) < 1e-4
    assert ad.rank() == o.SVD.compute_from(a).compress("ADAPTIVE", 1e-4).rank()


@pytest.mark.parametrize("dtype,shape", [(np.float64, (1000, 777)), (np.float32, (300, 900)), (np.float64, (1300, 1100)), (np.float64, (200, 199))])
def test_svd_cores_beyond_the_lds_limit(dtype, shape):
    """Cores that do not fit one CU's LDS run the round-per-launch Jacobi in global memory (any size):
    singular values against ?gesdd, orthonormal factors, reconstruction; a random spectrum and a decaying one."""
    f64 = dtype == np.float64
    rng = np.random.default_rng(shape[0])
    for a in (rng.standard_normal(shape).astype(dtype), o.random_approximate_low_rank_matrix(shape, 1.0, 1e-8 if f64 else 1e-4, rng, dtype)):
        u, s, vt = (npy(t) for t in rc.compute_svd(a))
        so = o.compute_svd(a)[1]
        r = min(shape)
        assert u.shape == (shape[0], r) and vt.shape == (r, shape[1])
        assert np.all(s[:-1] >= s[1:])
        assert np.abs(s - so).max() <= (1e-12 if f64 else 2e-5) * so[0]
        assert rel((u * s) @ vt, a) <= (1e-12 if f64 else 5e-5)
        # (vectors of tiny singular values are not unique enough to COMPARE; orthonormal they are all the same)
        assert np.abs(u.T @ u - np.eye(r)).max() <= (1e-11 if f64 else 1e-4)
        assert np.abs(vt @ vt.T - np.eye(r)).max() <= (1e-11 if f64 else 1e-4)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("shape", [(50, 30), (30, 50), (128, 128), (8, 8)])
def test_svd_with_exactly_zero_singular_values_keeps_u_orthonormal(dtype, shape):
    """?gesdd returns an orthonormal U for rank-deficient input (compute_svd.rs:18-27 -> svddc); the Jacobi core completes the
    left vectors of zero singular values (k_complete_left_basis).  Zero columns / rows make singular values EXACTLY zero."""
    f64 = dtype == np.float64
    rng = np.random.default_rng(shape[0] + 3 * shape[1])
    m, n = shape
    r = min(m, n)
    a = rng.standard_normal(shape).astype(dtype)
    a[:, n // 3:] = 0  # only n // 3 nonzero columns
    a[m // 2:, :] = 0  # and m // 2 nonzero rows
    u, s, vt = (npy(t) for t in rc.compute_svd(a))
    rank = min(n // 3, m // 2)
    assert np.all(s[rank:] == 0) and np.all(s[:rank] > 0)
    tol = 1e-12 if f64 else 2e-5
    assert np.abs(u.T @ u - np.eye(r)).max() <= tol, "left vectors of zero singular values complete the basis"
    assert np.abs(vt @ vt.T - np.eye(r)).max() <= tol
    assert rel((u * s) @ vt, a) <= (1e-13 if f64 else 1e-5)
    z = np.zeros(shape, dtype=dtype)
    u, s, vt = (npy(t) for t in rc.compute_svd(z))
    assert np.all(s == 0) and np.abs(u.T @ u - np.eye(r)).max() <= tol and np.abs(vt @ vt.T - np.eye(r)).max() <= tol


@pytest.mark.parametrize("shape", [(128, 128), (100, 50), (50, 100), (133, 133), (300, 40)])
def test_svd_of_clustered_and_repeated_singular_values(shape):
    """Clustered / (near-)equal singular values: a rotation between two such columns has an O(1) angle however small the
    columns' cosine is, so the 'last sweep' shortcut of the Jacobi kernel must not fire on it.  ?gesdd delivers
    orthonormal factors to ~1e-15 here and the reference's f64 tests assume 1e-12 (src/svd.rs:214-223)."""
    from rusty_compression_amd import _lib

    m, n = shape
    r = min(m, n)
    rng = np.random.default_rng(m * 1000 + n)
    qa = np.linalg.qr(rng.standard_normal((m, r)))[0]
    qb = np.linalg.qr(rng.standard_normal((n, r)))[0]
    cases = {
        "1 + 1e-9 r": (qa * (1.0 + 1e-9 * rng.standard_normal(r))) @ qb.T,
        "all equal": qa @ qb.T,
        "two clusters": (qa * np.where(np.arange(r) % 2 == 0, 1.0, 0.5 + 1e-12 * np.arange(r))) @ qb.T,
    }
    if m == n:
        cases["I + 1e-9 E"] = np.eye(n) + 1e-9 * rng.standard_normal((n, n))
    for name, a in cases.items():
        u, s, vt = (npy(t) for t in rc.compute_svd(a))
        so = o.compute_svd(a)[1]
        assert np.abs(s - so).max() <= 1e-12 * so[0], name
        assert np.abs(u.T @ u - np.eye(r)).max() <= 1e-12, (name, np.abs(u.T @ u - np.eye(r)).max())
        assert np.abs(vt @ vt.T - np.eye(r)).max() <= 1e-12, (name, np.abs(vt @ vt.T - np.eye(r)).max())
        assert rel((u * s) @ vt, a) <= 1e-12, name
    assert _lib.default_context().get_health() == 0  # no sweep budget was exhausted


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_degenerate_shapes_and_zero_matrices(dtype):
    """1 x 1, single rows / columns, all-zero inputs (every reflector is the identity: tau = 0) and rank-1 inputs
    through pivoted QR / LQ, SVD and the IDs, against the oracle."""
    f64 = dtype == np.float64
    tol = 1e-13 if f64 else 1e-5
    rng = np.random.default_rng(3)
    for shape in [(1, 1), (1, 5), (5, 1), (2, 2), (3, 7), (7, 3)]:
        a = rng.standard_normal(shape).astype(dtype)
        q, r, ind = (npy(t) for t in rc.pivoted_qr(a))
        oq, orr, oind = o.pivoted_qr(a)
        assert np.array_equal(ind, oind), shape
        assert rel(q, oq) <= 10 * tol and rel(r, orr) <= 10 * tol, shape
        l, ql, indl = (npy(t) for t in rc.pivoted_lq(a))
        assert rel(l @ ql, a[indl, :]) <= 10 * tol, shape
        u, s, vt = (npy(t) for t in rc.compute_svd(a))
        assert np.abs(s - o.compute_svd(a)[1]).max() <= 10 * tol * max(1.0, float(np.abs(a).max())), shape
        assert rel((u * s) @ vt, a) <= 10 * tol, shape
        qr = rc.QR.compute_from(a)
        assert rc.rel_diff_fro(qr.column_id().to_mat(), a) <= 100 * tol
        assert rc.rel_diff_fro(rc.LQ.compute_from(a).row_id().to_mat(), a) <= 100 * tol
    # all-zero matrix: LAPACK leaves the identity permutation, Q = [I; 0], R = 0
    z = np.zeros((6, 4), dtype=dtype)
    q, r, ind = (npy(t) for t in rc.pivoted_qr(z))
    oq, orr, oind = o.pivoted_qr(z)
    assert np.array_equal(ind, oind) and np.array_equal(r, orr) and np.array_equal(q, oq)
    u, s, vt = (npy(t) for t in rc.compute_svd(z))
    assert np.all(s == 0) and np.all(np.isfinite(u)) and np.all(np.isfinite(vt))
    # rank one: one non-zero singular value, the pivot is the column of largest norm
    x = np.outer(rng.standard_normal(40), rng.standard_normal(30)).astype(dtype)
    q, r, ind = (npy(t) for t in rc.pivoted_qr(x))
    assert ind[0] == int(np.argmax(np.linalg.norm(x, axis=0)))
    assert rel(q @ r, x[:, ind]) <= 100 * tol
    s = npy(rc.compute_svd(x)[1])
    assert abs(s[0] - np.linalg.norm(x)) <= 100 * tol * np.linalg.norm(x) and s[1] <= 1e3 * tol * s[0]


# ---------------------------------------------------------------- compress / to_mat / IDs (a7-a10, a13-a16)
@pytest.mark.parametrize("dtype,shape", [(np.float64, (100, 50)), (np.float32, (100, 50)), (np.float64, (50, 100)), (np.float32, (50, 100))])
def test_qr_compression_and_ids_reference_properties(dtype, shape):
    """src/qr.rs:432-450, :466-483, :497-524, :538-564; src/col_interp_decomp.rs:180-223; src/row_interp_decomp.rs:180-217."""
    rng = np.random.default_rng(33)
    a = o.random_approximate_low_rank_matrix(shape, 1.0, 1e-10, rng, dtype)
    tol = 1e-4
    qr = rc.QR.compute_from(a)
    c = qr.compress(CT.RANK(30))
    assert c.q.shape[1] == 30 and c.r.shape[0] == 30 and c.ind.shape[0] == shape[1]
    assert rc.rel_diff_fro(c.to_mat(), a) < tol
    t = qr.compress(CT.ADAPTIVE(tol))
    oq = o.QR.compute_from(a).compress("ADAPTIVE", tol)
    assert t.rank() == oq.rank() and t.rank() < min(shape)
    assert rc.rel_diff_fro(t.to_mat(), a) < 5 * tol
    cid = t.column_id()
    assert rc.rel_diff_fro(cid.to_mat(), a) < 5 * tol
    ap = npy(rc.apply_permutation(a, cid.get_col_ind(), rc.MatrixPermutationMode.COL))
    for i in range(t.rank()):
        assert rc.rel_diff_l2(ap[:, i].copy(), cid.get_c()[:, i].contiguous()) < tol
    lq = rc.LQ.compute_from(a).compress(CT.ADAPTIVE(tol))
    assert lq.rank() == o.LQ.compute_from(a).compress("ADAPTIVE", tol).rank()
    assert rc.rel_diff_fro(lq.to_mat(), a) < 5 * tol
    rid = lq.row_id()
    assert rc.rel_diff_fro(rid.to_mat(), a) < 5 * tol
    apr = npy(rc.apply_permutation(a, rid.get_row_ind(), rc.MatrixPermutationMode.ROW))
    for i in range(lq.rank()):
        assert rc.rel_diff_l2(apr[i].copy(), rid.get_r()[i].contiguous()) < tol
    for ts, k in ((cid.two_sided_id(), t.rank()), (rid.two_sided_id(), lq.rank())):
        assert rc.rel_diff_fro(ts.to_mat(), a) < 5 * tol
        assert tuple(ts.x.shape) == (k, k)
        mp = o.apply_permutation_matrix(o.apply_permutation_matrix(a, npy(ts.row_ind), "ROW"), npy(ts.col_ind), "COL")
        assert np.all(np.abs(npy(ts.x) - mp[:k, :k]) < 10 * tol * np.abs(mp[:k, :k]))
    # Apply (types.rs:25-29) on a matrix and on a vector
    rhs = rng.standard_normal((shape[1], 3)).astype(dtype)
    for dec in (cid, rid, cid.two_sided_id()):
        full = npy(dec.to_mat()).astype(np.float64)
        assert rel(npy(dec.dot(rhs)), full @ rhs) <= (1e-10 if dtype == np.float64 else 1e-4)
        assert rel(npy(dec.dot(rhs[:, 0].copy())), full @ rhs[:, 0]) <= (1e-10 if dtype == np.float64 else 1e-4)


def test_ids_match_golden_factor_by_factor():
    g = golden("cfg1_id.npz")
    a = golden("cfg1_sketch_rsvd.npz")["a"]
    full = rc.QR.compute_from(a)
    full_lq = rc.LQ.compute_from(a)
    for ct, tag in ((CT.RANK(32), "rank32"), (CT.ADAPTIVE(1e-4), "tol1e4")):
        qrc = full.compress(ct)
        k = int(g[f"{tag}_rank"])
        assert qrc.rank() == k
        assert np.array_equal(npy(qrc.ind)[:k], g[f"{tag}_ind"][:k])
        cid = qrc.column_id()
        assert rel(npy(cid.c), g[f"{tag}_c"]) <= 1e-10
        # Z solves R11 Z12 = R12 with cond(R11) ~ 1/tol: compare through the action on A's columns
        assert rel(npy(cid.c) @ npy(cid.z), g[f"{tag}_c"] @ g[f"{tag}_z"]) <= 1e-10
        assert rel(npy(cid.z)[:, npy(cid.col_ind)[:k]], np.eye(k)) <= 1e-12
        ts = cid.two_sided_id()
        assert np.array_equal(npy(ts.row_ind)[:k], g[f"{tag}_ts_row_ind"][:k])
        assert rel(npy(ts.x), g[f"{tag}_ts_x"]) <= 1e-10
        assert rel(npy(ts.to_mat()), g[f"{tag}_ts_c"] @ g[f"{tag}_ts_x"] @ g[f"{tag}_ts_r"]) <= 1e-9
        lqc = full_lq.compress(ct)
        kl = int(g[f"{tag}_lq_rank"])
        assert lqc.rank() == kl
        assert np.array_equal(npy(lqc.ind)[:kl], g[f"{tag}_lq_ind"][:kl])
        rid = lqc.row_id()
        assert rel(npy(rid.r), g[f"{tag}_rid_r"]) <= 1e-10
        assert rel(npy(rid.to_mat()), g[f"{tag}_rid_x"] @ g[f"{tag}_rid_r"]) <= 1e-10
        ts2 = rid.two_sided_id()
        assert np.array_equal(npy(ts2.col_ind)[:kl], g[f"{tag}_ts2_col_ind"][:kl])
        assert rel(npy(ts2.x), g[f"{tag}_ts2_x"]) <= 1e-10


def test_full_rank_shortcuts_and_error_behaviour():
    rng = np.random.default_rng(8)
    a = rng.standard_normal((40, 12))
    qr = rc.QR.compute_from(a)           # rank == ncols: src/qr.rs:274-281
    cid = qr.column_id()
    assert rel(npy(cid.to_mat()), a) <= 1e-13
    ocid = o.QR.compute_from(a).column_id()
    assert rel(npy(cid.c), ocid.c) <= 1e-12 and np.array_equal(npy(cid.z), ocid.z)
    lq = rc.LQ.compute_from(a.T.copy())  # rank == nrows: src/qr.rs:367-374
    rid = lq.row_id()
    assert rel(npy(rid.to_mat()), a.T) <= 1e-13
    with pytest.raises(rc.CompressionError):  # src/qr.rs:196-199
        rc.QR.compute_from(np.eye(6)).compress(CT.ADAPTIVE(1e-3))
    with pytest.raises(rc.CompressionError):  # src/svd.rs:97-100
        rc.SVD.compute_from(np.eye(6)).compress(CT.ADAPTIVE(1e-3))
    with pytest.raises(AssertionError):       # src/qr.rs:188
        qr.compress(CT.ADAPTIVE(1.5))
    big = qr.compress(CT.RANK(1000))          # rank is clipped: src/qr.rs:172-174
    assert big.rank() == 12


# ---------------------------------------------------------------- sampling (a4, a9, a12, a19, a20)
def test_sketch_rsvd_and_range_qr_match_golden():
    g = golden("cfg1_sketch_rsvd.npz")
    a, omega, k, p = g["a"], g["omega"], int(g["k"]), int(g["p"])
    q = rc.sample_range_by_rank(a, k, p, omega)
    assert rel(npy(q), g["q_sample"]) <= 1e-10
    qp = rc.sample_range_power_iteration(a, k, p, 2, omega)
    assert rel(npy(qp), g["q_power"]) <= 1e-10
    assert rel(npy(rc.sample_range_power_iteration(a, k, p, 1, omega)), g["q_power"]) <= 1e-10  # the shadowing quirk
    assert rel(npy(rc.sample_range_power_iteration(a, k, p, 0, omega)), g["q_sample"]) <= 1e-10
    svd = rc.SVD.compute_from_range_estimate(q, a)
    assert np.abs(npy(svd.s) - g["s"]).max() / g["s"][0] <= 1e-12
    u, vt = sign_normalise(npy(svd.u), npy(svd.vt))
    assert rel(u, g["u"]) <= 1e-8 and rel(vt, g["vt"]) <= 1e-8
    assert rel(npy(svd.to_mat()), g["u"] @ np.diag(g["s"]) @ g["vt"]) <= 1e-10
    qr = rc.QR.compute_from_range_estimate(q, a)
    assert np.array_equal(npy(qr.ind), g["qr_ind"])
    assert rel(npy(qr.r), g["qr_r"]) <= 1e-10 and rel(npy(qr.q), g["qr_q"]) <= 1e-10
    cid = qr.column_id()
    assert rel(npy(cid.c), g["id_c"]) <= 1e-10 and rel(npy(cid.z), g["id_z"]) <= 1e-9


def test_fused_pipeline_with_forked_branches_is_bit_identical():
    """RC_OPT_FORK_BRANCHES: the SVD and the ID branch of rc_rsvd_id on two streams (fork / join), eager and replayed
    from a hipGraph, give exactly the results of the single-stream order."""
    import ctypes

    from rusty_compression_amd import _lib

    lib = _lib.lib()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        ctx = _lib.Context(torch.cuda.current_device(), st.cuda_stream)
        g = torch.Generator(device="cpu").manual_seed(9)
        m, n, k, p = 1536, 1280, 48, 5
        a = torch.randn(m, n, dtype=torch.float64, generator=g).cuda()
        om = torch.randn(n, k + p, dtype=torch.float64, generator=g).cuda()
        mk = lambda r, c: torch.zeros((r, c), dtype=torch.float64, device="cuda")  # noqa: E731

        def outputs():
            b = dict(range_q=mk(m, k), u=mk(m, k), s=torch.zeros(k, dtype=torch.float64, device="cuda"), vt=mk(k, n), qr_q=mk(m, k), qr_r=mk(k, n),
                     qr_ind=torch.zeros(n, dtype=torch.int64, device="cuda"), id_c=mk(m, k), id_z=mk(k, n))
            o_ = _lib.rc_rsvd_id_out(_lib.mat(b["range_q"]), _lib.mat(b["u"]), ctypes.c_void_p(b["s"].data_ptr()), _lib.mat(b["vt"]), _lib.mat(b["qr_q"]),
                                     _lib.mat(b["qr_r"]), ctypes.c_void_p(b["qr_ind"].data_ptr()), _lib.mat(b["id_c"]), _lib.mat(b["id_z"]))
            return b, o_

        def run(o_):
            ctx.call("rc_rsvd_id_f64", _lib.mat(a), ctypes.c_int64(k), ctypes.c_int64(p), _lib.mat(om), ctypes.c_uint64(0), ctypes.byref(o_))

        ref, oref = outputs()
        run(oref)
        ctx.synchronize()
        ctx.set_option(_lib.RC_OPT_FORK_BRANCHES, 1)
        got, ogot = outputs()
        run(ogot)
        ctx.synchronize()
        for key in ref:
            assert torch.equal(ref[key], got[key]), key
        graph = ctypes.c_void_p(None)
        rep, orep = outputs()
        run(orep)  # sizes the side arena for this output set
        ctx.synchronize()
        ctx.check(lib.rc_graph_begin_capture(ctx._h))
        run(orep)
        ctx.check(lib.rc_graph_end_capture(ctx._h, ctypes.byref(graph)))
        for t in rep.values():
            t.zero_()
        for _ in range(3):
            ctx.check(lib.rc_graph_launch(ctx._h, graph))
        ctx.synchronize()
        for key in ref:
            assert torch.equal(ref[key], rep[key]), key
        assert ctx.get_health() == 0
        ctx.check(lib.rc_graph_destroy(ctx._h, graph))
        ctx.close()


def test_power_iteration_fixed_mode_is_opt_in_and_matches_the_documented_algorithm():
    """RC_OPT_POWER_ITERATION_FIXED: it_count real power steps; the default keeps
    the reference's shadowing quirk (one step).  Oracle: oracle/ref_lapack.sample_range_power_iteration(fixed=True)."""
    from rusty_compression_amd import _lib

    g = golden("cfg1_sketch_rsvd.npz")
    a, omega, k, p = g["a"], g["omega"], int(g["k"]), int(g["p"])
    ctx = _lib.default_context()
    want = o.sample_range_power_iteration(a, k, p, 2, lambda shape: omega, fixed=True)
    ctx.set_option(_lib.RC_OPT_POWER_ITERATION_FIXED, 1)
    try:
        got2 = npy(rc.sample_range_power_iteration(a, k, p, 2, omega))
        got1 = npy(rc.sample_range_power_iteration(a, k, p, 1, omega))
    finally:
        ctx.set_option(_lib.RC_OPT_POWER_ITERATION_FIXED, 0)
    assert rel(got2, want) <= 1e-9
    assert rel(got1, g["q_power"]) <= 1e-10                     # one step: identical to the quirk
    assert rel(got2, g["q_power"]) > 1e-6                       # two real steps are a different basis
    # more power steps = a better range for a matrix with a decaying spectrum
    err = lambda q: np.linalg.norm(a - q @ (q.T @ a)) / np.linalg.norm(a)
    assert err(got2) <= err(g["q_power"]) * (1 + 1e-9)
    assert rel(npy(rc.sample_range_power_iteration(a, k, p, 2, omega)), g["q_power"]) <= 1e-10  # option off again


def test_fused_rsvd_id_equals_the_separate_calls():
    import ctypes

    from rusty_compression_amd import _lib

    g = golden("cfg1_sketch_rsvd.npz")
    a = torch.from_numpy(g["a"]).cuda()
    omega = torch.from_numpy(g["omega"]).cuda()
    m, n = a.shape
    k, p = int(g["k"]), int(g["p"])
    mk = lambda r, c: torch.empty((r, c), dtype=torch.float64, device="cuda")  # noqa: E731
    rq, u, vt, qq, qr_, cc, zz = mk(m, k), mk(m, k), mk(k, n), mk(m, k), mk(k, n), mk(m, k), mk(k, n)
    s = torch.empty(k, dtype=torch.float64, device="cuda")
    ind = torch.empty(n, dtype=torch.int64, device="cuda")
    out = _lib.rc_rsvd_id_out(_lib.mat(rq), _lib.mat(u), ctypes.c_void_p(s.data_ptr()), _lib.mat(vt), _lib.mat(qq), _lib.mat(qr_),
                              ctypes.c_void_p(ind.data_ptr()), _lib.mat(cc), _lib.mat(zz))
    _lib.default_context().call("rc_rsvd_id_f64", _lib.mat(a), ctypes.c_int64(k), ctypes.c_int64(p), _lib.mat(omega), ctypes.c_uint64(0), ctypes.byref(out))
    assert rel(npy(rq), g["q_sample"]) <= 1e-10
    assert np.abs(npy(s) - g["s"]).max() / g["s"][0] <= 1e-12
    un, vtn = sign_normalise(npy(u), npy(vt))
    assert rel(un, g["u"]) <= 1e-8 and rel(vtn, g["vt"]) <= 1e-8
    assert np.array_equal(npy(ind), g["qr_ind"])
    assert rel(npy(qr_), g["qr_r"]) <= 1e-10 and rel(npy(qq), g["qr_q"]) <= 1e-10
    assert rel(npy(cc), g["id_c"]) <= 1e-10 and rel(npy(zz), g["id_z"]) <= 1e-9


def test_adaptive_sampling_matches_golden_history():
    """examples/adaptive_sampling.rs call sequence; src/random_sampling.rs:223-274."""
    g = golden("adaptive_500x200.npz")
    a = g["a"]
    q, res = rc.sample_range_adaptive(a, 1e-5, 5, g["omegas"])
    assert [r for r, _ in res] == g["hist_rank"].tolist()
    assert np.allclose([e for _, e in res], g["hist_res"], rtol=1e-6)
    assert rel(npy(q), g["q"]) <= 1e-8
    qr = rc.QR.compute_from_range_estimate(q, a)
    err = rc.rel_diff_fro(qr.to_mat(), a)
    assert abs(err - float(g["rel_err"])) <= 1e-9 and err < 1e-4
    # device-generated Omega: same statistical behaviour, different samples
    q2, res2 = rc.sample_range_adaptive(a, 1e-5, 5, rc.Rng(5))
    assert q2.shape[1] % 5 == 0 and abs(q2.shape[1] - q.shape[1]) <= 25
    assert rc.rel_diff_fro(rc.QR.compute_from_range_estimate(q2, a).to_mat(), a) < 1e-4
    assert np.abs(npy(q2).T @ npy(q2) - np.eye(q2.shape[1])).max() < 1e-10
    with pytest.raises(rc.CompressionError):  # capacity exhausted before the tolerance
        rc.sample_range_adaptive(a, 1e-9, 5, rc.Rng(5), max_rank=20)


def test_max_col_norm_and_rel_diff():
    rng = np.random.default_rng(2)
    for dtype in (np.float64, np.float32):
        y = rng.standard_normal((300, 17)).astype(dtype)
        assert abs(rc.max_col_norm(y) - float(o.max_col_norm(y))) <= (1e-12 if dtype == np.float64 else 1e-4)
        z = y + (1e-3 * rng.standard_normal(y.shape)).astype(dtype)
        assert abs(rc.rel_diff_fro(z, y) - o.rel_diff_fro(z, y)) <= (1e-12 if dtype == np.float64 else 1e-6)
        assert abs(rc.rel_diff_l2(z[:, 0].copy(), y[:, 0].copy()) - o.rel_diff_l2(z[:, 0], y[:, 0])) <= (1e-12 if dtype == np.float64 else 1e-6)


def test_random_test_matrix_generators():
    a = rc.random_approximate_low_rank_matrix((120, 70), 1.0, 1e-6, rc.Rng(1))
    s = np.linalg.svd(npy(a), compute_uv=False)
    assert rel(s, np.geomspace(1e-6, 1.0, 70)[::-1]) <= 1e-9  # src/random_matrix.rs:84-92
    u = npy(rc.random_orthogonal_matrix((90, 30), rc.Rng(2)))
    assert np.abs(u.T @ u - np.eye(30)).max() <= 1e-12
    w = npy(rc.random_orthogonal_matrix((30, 90), rc.Rng(2)))
    assert np.abs(w @ w.T - np.eye(30)).max() <= 1e-12


# ---------------------------------------------------------------- tall-skinny fast path (CholeskyQR2 + LDS QRCP + sign fix)
def _with_fast_path(on, fn):
    from rusty_compression_amd import _lib

    ctx = _lib.default_context()
    ctx.set_option(_lib.RC_OPT_TALL_SKINNY_FAST_PATH, 1 if on else 0)
    try:
        return fn()
    finally:
        ctx.set_option(_lib.RC_OPT_TALL_SKINNY_FAST_PATH, 1)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("shape,smin", [((4096, 69), 1e-3), ((8192, 133), 1e-2), ((2048, 33), 1e-3), ((1500, 17), 1e-1)])
def test_fast_path_reproduces_lapack_pivots_signs_and_factors(dtype, shape, smin):
    rng = np.random.default_rng(shape[1])
    if dtype == np.float32:
        smin = max(smin, 3e-2)  # keep cond^2 * eps_f32 << 1 so the certificate holds and the fast path is what is tested
    a = o.random_approximate_low_rank_matrix(shape, 1.0, smin, rng, dtype)
    q, r, ind = o.pivoted_qr(a)
    f64 = dtype == np.float64
    for fast in (True, False):
        gq, gr, gi = _with_fast_path(fast, lambda: tuple(npy(t) for t in rc.pivoted_qr(a)))
        ns = agreed_pivot_prefix(gi, gr, ind, r, dtype)
        assert is_permutation(gi, shape[1])
        if f64:
            assert ns == shape[1], (fast, ns)
            assert rel(gr, r) <= 1e-10, (fast, rel(gr, r))          # same signs as ?geqp3
            assert rel(gq, q) <= 1e-9, (fast, rel(gq, q))            # same signs as ?orgqr
        else:
            assert rel(gr[:ns, :ns], r[:ns, :ns]) <= 1e-4
        assert rel(gq @ gr, a[:, gi]) <= (1e-13 if f64 else 5e-6)
        assert np.abs(gq.T @ gq - np.eye(shape[1])).max() <= (1e-13 if f64 else 1e-5)
    # truncated + LQ orientation through the same path
    gq, gr, gi = (npy(t) for t in rc.pivoted_qr(a, rank=shape[1] // 2))
    kk = shape[1] // 2
    if f64:
        assert np.array_equal(gi[:kk], ind[:kk]) and rel(gq, q[:, :kk]) <= 1e-9
    l, ql, indl = (npy(t) for t in rc.pivoted_lq(a.T.copy()))
    if f64:
        assert np.array_equal(indl, ind) and rel(l, r.T) <= 1e-10 and rel(ql, q.T) <= 1e-9


def test_fast_path_falls_back_when_its_certificate_fails():
    rng = np.random.default_rng(77)
    # cond 1e10: cond^2 eps >> 1, CholeskyQR2 cannot work; the call must still return LAPACK-quality factors
    a = o.random_approximate_low_rank_matrix((3000, 40), 1.0, 1e-10, rng)
    q, r, ind = o.pivoted_qr(a)
    gq, gr, gi = (npy(t) for t in rc.pivoted_qr(a))
    assert np.array_equal(gi, ind) and rel(gr, r) <= 1e-10
    assert np.abs(gq.T @ gq - np.eye(40)).max() <= 1e-13 and rel(gq @ gr, a[:, gi]) <= 1e-13
    u, s, vt = (npy(t) for t in rc.compute_svd(a))
    assert np.abs(s - o.compute_svd(a)[1]).max() / s[0] <= 1e-12
    assert np.abs(u.T @ u - np.eye(40)).max() <= 1e-12
    # rank-deficient sketch: exactly singular Gram matrix
    b = rng.standard_normal((2048, 10)) @ rng.standard_normal((10, 24))
    gq, gr, gi = (npy(t) for t in rc.pivoted_qr(b))
    assert rel(gq @ gr, b[:, gi]) <= 1e-12 and np.abs(gq.T @ gq - np.eye(24)).max() <= 1e-12


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_svd_of_tall_and_wide_matrices_through_both_paths(dtype):
    rng = np.random.default_rng(5)
    tol = TOL[np.dtype(dtype)]
    for shape in ((4096, 96), (128, 8192), (2048, 128)):
        a = o.random_approximate_low_rank_matrix(shape, 1.0, 1e-2, rng, dtype)
        s_ref = o.compute_svd(a)[1]
        for fast in (True, False):
            u, s, vt = _with_fast_path(fast, lambda: tuple(npy(t) for t in rc.compute_svd(a)))
            assert np.abs(s - s_ref).max() / s_ref[0] <= tol["sval"] * 4
            assert rel(u @ np.diag(s) @ vt, a) <= tol["recon"] * 4
            r_ = min(shape)
            assert np.abs(u.T @ u - np.eye(r_)).max() <= (1e-12 if dtype == np.float64 else 1e-4)
            assert np.abs(vt @ vt.T - np.eye(r_)).max() <= (1e-12 if dtype == np.float64 else 1e-4)


def test_headline_size_sketch_matches_the_oracle():
    """cfg2 / cfg3 shapes with device-generated inputs; oracle in GEMM form on the same bits.  Every factor of the chain is
    held to the oracle: range basis, S, U S V^T, the FULL permutation (a k x n ?geqp3 performs exactly k steps, so the tail
    ind[k:] is the deterministic swap order), R, Q, and the column ID built from them."""
    for (n, k) in ((4096, 64), (8192, 128)):
        a = rc.random_gaussian((n, n), rc.Rng(n))
        om = rc.random_gaussian((n, k + 5), rc.Rng(1))
        q = rc.sample_range_by_rank(a, k, 5, om)
        an, omn = npy(a), npy(om)
        oq = o.sample_range_by_rank(an, k, 5, lambda s: omn)
        assert rel(npy(q), oq) <= 1e-10
        svd = rc.SVD.compute_from_range_estimate(q, a)
        osv = o.SVD.compute_from_range_estimate(oq, an)
        assert np.abs(npy(svd.s) - osv.s).max() / osv.s[0] <= 1e-12
        assert rel(npy(svd.to_mat()), osv.to_mat()) <= 1e-10
        qr = rc.QR.compute_from_range_estimate(q, a)
        oqr = o.QR.compute_from_range_estimate(oq, an)
        assert np.array_equal(npy(qr.ind), oqr.ind)
        assert rel(npy(qr.r), oqr.r) <= 1e-10
        assert rel(npy(qr.q), oqr.q) <= 1e-10
        cid, ocid = qr.column_id(), oqr.column_id()
        assert rel(npy(cid.c), ocid.c) <= 1e-10 and rel(npy(cid.z), ocid.z) <= 1e-9
        assert np.array_equal(npy(cid.col_ind), ocid.col_ind)


def _rsvd_id_buffers(m, n, k):
    import ctypes

    from rusty_compression_amd import _lib

    mk = lambda r, c: torch.zeros((r, c), dtype=torch.float64, device="cuda")  # noqa: E731
    b = dict(range_q=mk(m, k), u=mk(m, k), s=torch.zeros(k, dtype=torch.float64, device="cuda"), vt=mk(k, n), qr_q=mk(m, k), qr_r=mk(k, n),
             qr_ind=torch.zeros(n, dtype=torch.int64, device="cuda"), id_c=mk(m, k), id_z=mk(k, n))
    o_ = _lib.rc_rsvd_id_out(_lib.mat(b["range_q"]), _lib.mat(b["u"]), ctypes.c_void_p(b["s"].data_ptr()), _lib.mat(b["vt"]), _lib.mat(b["qr_q"]),
                             _lib.mat(b["qr_r"]), ctypes.c_void_p(b["qr_ind"].data_ptr()), _lib.mat(b["id_c"]), _lib.mat(b["id_z"]))
    return b, o_


def test_cfg3_accuracy_bearing_input_through_the_fused_call_eager_and_graph_replayed():
    """the second cfg3 input, A = U diag(geomspace(1e-10, 1, 8192)) V^T (reference recipe), so that the
    <= 1e-10 factor-error target means something; through rc_rsvd_id_f64 eagerly and replayed from a hipGraph."""
    import ctypes

    from rusty_compression_amd import _lib

    n, k, p = 8192, 128, 5
    lib = _lib.lib()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        ctx = _lib.Context(torch.cuda.current_device(), st.cuda_stream)
        a = _decaying_matrix(n, 1e-10, torch.float64, 3)
        om = rc.random_gaussian((n, k + p), rc.Rng(33))
        st.synchronize()
        eager, oe = _rsvd_id_buffers(n, n, k)

        def run(o_):
            ctx.call("rc_rsvd_id_f64", _lib.mat(a), ctypes.c_int64(k), ctypes.c_int64(p), _lib.mat(om), ctypes.c_uint64(0), ctypes.byref(o_))

        run(oe)
        ctx.synchronize()
        rep, orep = _rsvd_id_buffers(n, n, k)
        run(orep)
        ctx.synchronize()
        graph = ctypes.c_void_p(None)
        ctx.check(lib.rc_graph_begin_capture(ctx._h))
        run(orep)
        ctx.check(lib.rc_graph_end_capture(ctx._h, ctypes.byref(graph)))
        for t in rep.values():
            t.zero_()
        ctx.check(lib.rc_graph_launch(ctx._h, graph))
        ctx.synchronize()
        assert ctx.get_health() == 0
        for key in eager:
            assert torch.equal(eager[key], rep[key]), key
        ctx.check(lib.rc_graph_destroy(ctx._h, graph))
        an, omn = npy(a), npy(om)
        oq = o.sample_range_by_rank(an, k, p, lambda s_: omn)
        osv = o.SVD.compute_from_range_estimate(oq, an)
        oqr = o.QR.compute_from_range_estimate(oq, an)
        ocid = oqr.column_id()
        g = {kk: npy(v) for kk, v in eager.items()}
        assert rel(g["range_q"], oq) <= 1e-10
        assert np.abs(g["s"] - osv.s).max() / osv.s[0] <= 1e-12
        assert rel((g["u"] * g["s"]) @ g["vt"], osv.to_mat()) <= 1e-10
        assert np.array_equal(g["qr_ind"], oqr.ind)
        assert rel(g["qr_r"], oqr.r) <= 1e-10 and rel(g["qr_q"], oqr.q) <= 1e-10
        assert rel(g["id_c"], ocid.c) <= 1e-10 and rel(g["id_z"], ocid.z) <= 1e-9
        # factor error vs the CPU reference path (north_star: <= 1e-10) and the approximation error itself
        err = np.linalg.norm(an - (g["u"] * g["s"]) @ g["vt"]) / np.linalg.norm(an)
        oerr = np.linalg.norm(an - osv.to_mat()) / np.linalg.norm(an)
        assert abs(err - oerr) <= 1e-10
        ctx.close()


def test_graph_mode_reports_an_ill_conditioned_sketch_and_eager_mode_falls_back():
    """Negative test of the captured fast paths: a sketch Y = A Omega with cond(Y)^2 eps >> 1 cannot go through
    CholeskyQR2.  Inside a hipGraph no fallback is possible -- the replay must raise health bits 1 / 2; the eager call on
    the same input must fall back to the Householder chain and match the oracle."""
    import ctypes

    from rusty_compression_amd import _lib

    m = n = 2048
    k, p = 32, 5
    lib = _lib.lib()
    rng = np.random.default_rng(77)
    u = np.linalg.qr(rng.standard_normal((m, 64)))[0]
    v = np.linalg.qr(rng.standard_normal((n, 64)))[0]
    sig = np.concatenate([np.geomspace(1.0, 1e-11, k + p), np.full(64 - k - p, 1e-12)])   # cond(Y) ~ 1e11: cond^2 eps ~ 1e6
    an = (u * sig) @ v.T
    omn = rng.standard_normal((n, k + p))
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        ctx = _lib.Context(torch.cuda.current_device(), st.cuda_stream)
        a, om = torch.from_numpy(an).cuda(), torch.from_numpy(omn).cuda()
        eager, oe = _rsvd_id_buffers(m, n, k)

        def run(o_):
            ctx.call("rc_rsvd_id_f64", _lib.mat(a), ctypes.c_int64(k), ctypes.c_int64(p), _lib.mat(om), ctypes.c_uint64(0), ctypes.byref(o_))

        run(oe)   # eager: the certificate fails, the call falls back
        ctx.synchronize()
        assert ctx.get_health() == 0
        oq = o.sample_range_by_rank(an, k, p, lambda s_: omn)
        osv = o.SVD.compute_from_range_estimate(oq, an)
        g = {kk: npy(t) for kk, t in eager.items()}
        assert np.abs(g["range_q"].T @ g["range_q"] - np.eye(k)).max() <= 1e-12
        assert rel(g["range_q"][:, :8], oq[:, :8]) <= 1e-9          # later columns are ill-determined (sigma_j / sigma_1 down to 1e-10)
        assert np.abs(g["s"] - osv.s).max() / osv.s[0] <= 1e-12
        assert rel((g["u"] * g["s"]) @ g["vt"], osv.to_mat()) <= 1e-10
        rep, orep = _rsvd_id_buffers(m, n, k)
        graph = ctypes.c_void_p(None)
        ctx.check(lib.rc_graph_begin_capture(ctx._h))
        run(orep)
        ctx.check(lib.rc_graph_end_capture(ctx._h, ctypes.byref(graph)))
        ctx.check(lib.rc_graph_launch(ctx._h, graph))
        ctx.synchronize()
        h = ctx.get_health()
        assert h & 3, f"health word {h}: an ill-conditioned captured CholeskyQR2 must raise bit 0 (value 1) or bit 1 (value 2)"
        assert ctx.get_health() == 0   # read-and-clear
        ctx.check(lib.rc_graph_destroy(ctx._h, graph))
        ctx.close()


# ---------------------------------------------------------------- BASELINE.json full sizes: size-independent properties
def test_cfg2_sketch_and_pivoted_qr_4096():
    """configs[1]: 4096 x 4096 f64, fixed-rank-64 sketch + pivoted QR."""
    n, k, p = 4096, 64, 5
    a = rc.random_gaussian((n, n), rc.Rng(2))
    om = rc.random_gaussian((n, k + p), rc.Rng(22))
    y = rc.matmat(a, om)
    q, r, ind = rc.pivoted_qr(y)
    qn, rn, indn = npy(q), npy(r), npy(ind)
    oq, orr, oind = o.pivoted_qr(npy(y))
    assert np.array_equal(indn, oind) and rel(rn, orr) <= 1e-10 and rel(qn, oq) <= 1e-10
    assert np.abs(qn.T @ qn - np.eye(k + p)).max() <= 1e-13
    basis = rc.sample_range_by_rank(a, k, p, om)
    assert rel(npy(basis), oq[:, :k]) <= 1e-10


def test_cfg4_adaptive_two_sided_id_16384x4096():
    """configs[3]: 16384 x 4096 f64, adaptive range finder to 1e-6 + two-sided ID (call sequence of
    examples/adaptive_sampling.rs followed by column_id / two_sided_id)."""
    m, n, r = 16384, 4096, 384
    g1 = rc.random_gaussian((m, r), rc.Rng(41))
    g2 = rc.random_gaussian((r, n), rc.Rng(42))
    sig = torch.logspace(0, -10, r, dtype=torch.float64, device="cuda")
    a = rc.dot(g1, sig[:, None] * g2) * (1.0 / np.sqrt(m * n))
    q, res = rc.sample_range_adaptive(a, 1e-6, 64, rc.Rng(4), max_rank=1024)
    rank = q.shape[1]
    assert rank % 64 == 0 and 64 <= rank <= 640 and res[-1][0] == rank and res[-1][1] < 1e-6
    assert all(res[i][1] >= res[i + 1][1] * 0.1 for i in range(len(res) - 1))  # the estimate decays
    qn = npy(q)
    assert np.abs(qn.T @ qn - np.eye(rank)).max() <= 1e-10
    qr = rc.QR.compute_from_range_estimate(q, a)
    err = rc.rel_diff_fro(qr.to_mat(), a)
    assert err < 1e-5, err   # the probabilistic bound is 1e-6 on the spectral estimate; Frobenius error is of that order
    cid = qr.column_id()
    assert rc.rel_diff_fro(cid.to_mat(), a) < 1e-5
    ts = cid.two_sided_id()
    assert rc.rel_diff_fro(ts.to_mat(), a) < 1e-4
    k = rank
    rows, cols = npy(ts.row_ind)[:k], npy(ts.col_ind)[:k]
    sub = npy(a)[np.ix_(rows, cols)]
    # X reproduces the selected entries to the accuracy of the rank-k approximation (col_interp_decomp.rs:208-223)
    assert np.linalg.norm(npy(ts.x) - sub) <= 1e-5 * np.linalg.norm(npy(a))


def test_cfg4_survey_recipe_rank_2816_against_the_oracle():
    """configs[3] at the SURVEY 8(d) recipe: 16384 x 4096 f64 = U diag(logspace(0, -10)) V^T, adaptive range finder to 1e-6 with
    sample size 64 (rank 2816 = 44 rounds), then QR::compute_from_range_estimate -- a 2816 x 4096 ?geqp3 that the blocked QRCP with
    cooperative panels factors in ~0.08 s -- compared with ?geqp3 (SciPy) of the SAME projected matrix: pivots on the prefix the data
    determines, R there, and the ID / two-sided ID errors."""
    m, n = 16384, 4096
    g = torch.Generator(device="cuda").manual_seed(4)
    u = torch.linalg.qr(torch.randn(m, n, dtype=torch.float64, device="cuda", generator=g)).Q
    v = torch.linalg.qr(torch.randn(n, n, dtype=torch.float64, device="cuda", generator=g)).Q
    sig = torch.logspace(0, -10, n, dtype=torch.float64, device="cuda")
    a = ((u * sig) @ v.T).contiguous()
    del u, v
    q, res = rc.sample_range_adaptive(a, 1e-6, 64, rc.Rng(11))
    rank = q.shape[1]
    assert rank % 64 == 0 and 2304 <= rank <= 3072 and res[-1][0] == rank and res[-1][1] < 1e-6, (rank, res[-1])
    assert len(res) == rank // 64 and all(res[i][1] >= res[i + 1][1] * 0.1 for i in range(len(res) - 1))
    qr = rc.QR.compute_from_range_estimate(q, a)
    err = rc.rel_diff_fro(qr.to_mat(), a)
    assert err < 1e-5, err
    # oracle: ?geqp3 of B = Q^H A on the host
    b = npy(rc.dot(q.t(), a))
    oq, orr, oind = o.pivoted_qr(b)
    r_dev, ind_dev = npy(qr.r), npy(qr.ind)
    assert is_permutation(ind_dev, n)
    ns = agreed_pivot_prefix(ind_dev[:rank], r_dev, oind[:rank], orr[:rank], np.float64)
    want = min(rank, stable_prefix(orr, np.float64))
    assert ns >= want and want >= 1024, f"{ns} of {want} pivots agree with ?geqp3 (rank {rank})"
    assert rel(np.abs(np.diag(r_dev))[:ns], np.abs(np.diag(orr))[:ns]) <= 1e-10
    assert rel(r_dev[:ns][:, ind_dev.argsort()], orr[:ns][:, oind.argsort()]) <= 1e-9
    qn = npy(qr.q)
    assert np.abs(qn[:, :256].T @ qn - np.eye(256, rank)).max() <= 1e-12
    cid = qr.column_id()
    assert rc.rel_diff_fro(cid.to_mat(), a) < 1e-5
    ts = cid.two_sided_id()
    assert rc.rel_diff_fro(ts.to_mat(), a) < 1e-4


def _with_blocked(on, fn):
    from rusty_compression_amd import _lib

    ctx = _lib.default_context()
    ctx.set_option(_lib.RC_OPT_BLOCKED_QRCP, 1 if on else 0)
    try:
        return fn()
    finally:
        ctx.set_option(_lib.RC_OPT_BLOCKED_QRCP, 1)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("shape,smin,rank", [((300, 300), 1e-6, None), ((1000, 777), 1e-8, None), ((700, 1500), 1e-5, None), ((2048, 2048), 1e-6, 96),
                                              ((1500, 1100), 1e-3, 70), ((640, 4000), 1e-4, 33), ((513, 259), 1e-9, None)])
def test_blocked_qrcp_matches_lapack_and_the_per_step_chain(dtype, shape, smin, rank):
    """General shapes through the blocked ?laqps path (kernels_qrblk.hip: candidate-set panels, GEMM block update) against
    ?geqp3 + ?orgqr (pivots bit-exact on the prefix the data determines, near-tie rule at a first disagreement, factors to
    tolerance) and against the library's own per-step chain (RC_OPT_BLOCKED_QRCP = 0), full and truncated."""
    f64 = dtype == np.float64
    tol = TOL[np.dtype(dtype)]
    rng = np.random.default_rng(shape[0] + shape[1])
    a = o.random_approximate_low_rank_matrix(shape, 1.0, smin if f64 else max(smin, 1e-4), rng, dtype)
    k = rank or min(shape)
    oq, orr, oind = o.pivoted_qr(a)
    res = {}
    for blocked in (True, False):
        q, r, ind = _with_blocked(blocked, lambda: tuple(npy(t) for t in rc.pivoted_qr(a, rank=k)))
        assert is_permutation(ind, shape[1])
        ns = agreed_pivot_prefix(ind[:k], r, oind[:k], orr[:k], dtype)
        want = min(k, stable_prefix(orr, dtype))
        # f64: every pivot the data determines; f32: a first disagreement may be a proven near tie (agreed_pivot_prefix asserts it)
        assert (ns == want) if f64 else (ns >= want // 4), f"blocked={blocked}: {ns} of {want} pivots agree with ?geqp3"
        assert np.abs(q.T @ q - np.eye(k)).max() <= (1e-12 if f64 else 2e-5)
        assert rel(q @ r, a[:, ind]) <= (tol["recon"] * 10 if rank is None else 1.0)  # truncated: not a full factorization
        ia = ind.argsort()
        assert rel(r[:ns][:, ia], orr[:ns][:, oind.argsort()]) <= tol["factor"] * (1 if f64 else 3)
        # columns of Q that belong to tiny |r_jj| are ill-determined (sensitivity ~ eps |r_00| / |r_jj|): compare the leading ones
        lead = min(ns, int((np.abs(np.diag(orr)) > np.abs(orr[0, 0]) * (1e-4 if f64 else 1e-2)).sum()))
        assert rel(q[:, :lead], oq[:, :lead]) <= tol["factor"] * (10 if f64 else 3)
        res[blocked] = (q, r, ind)
    nsb = agreed_pivot_prefix(res[True][2][:k], res[True][1], res[False][2][:k], res[False][1], dtype)
    assert nsb >= (min(k, stable_prefix(orr, dtype)) if f64 else 1)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_blocked_qrcp_degenerate_inputs(dtype):
    """All-equal norms (every column a candidate: plain ?laqps), exact ties (first position wins), zero and rank-deficient
    matrices, a panel that must end early because a norm loses its accuracy."""
    f64 = dtype == np.float64
    n = 256
    # identity-like: all norms tie -> LAPACK takes positions in order
    e = np.eye(n, dtype=dtype)
    q, r, ind = (npy(t) for t in rc.pivoted_qr(e))
    oq, orr, oind = o.pivoted_qr(e)
    assert np.array_equal(ind, oind) and rel(r, orr) <= 1e-6
    # duplicated columns: the first of each tie is taken
    rng = np.random.default_rng(12)
    b = rng.standard_normal((300, 160)).astype(dtype)
    b[:, 80:] = b[:, :80]
    q, r, ind = (npy(t) for t in rc.pivoted_qr(b))
    oq, orr, oind = o.pivoted_qr(b)
    ns = stable_prefix(orr, dtype)
    # a column and its copy tie exactly here, while the BLAS kernels behind LAPACK may round the two differently (their
    # position inside a SIMD group differs): the pivots are compared as "a column or its copy"
    assert ns <= 90 and np.array_equal(ind[:ns] % 80, oind[:ns] % 80)
    assert rel(q @ r, b[:, ind]) <= (1e-12 if f64 else 1e-5)
    # zero matrix
    z = np.zeros((200, 300), dtype=dtype)
    q, r, ind = (npy(t) for t in rc.pivoted_qr(z))
    assert np.array_equal(ind, np.arange(300)) and np.all(r == 0) and np.array_equal(q, np.eye(200, dtype=dtype))
    # exact rank 40 inside 400 x 400: after 40 steps every norm collapses (tol3z recomputations galore)
    x = (rng.standard_normal((400, 40)) @ rng.standard_normal((40, 400))).astype(dtype)
    q, r, ind = (npy(t) for t in rc.pivoted_qr(x))
    oq, orr, oind = o.pivoted_qr(x)
    ns = stable_prefix(orr, dtype)
    assert 38 <= ns <= 42 and np.array_equal(ind[:ns], oind[:ns])
    assert rel(q @ r, x[:, ind]) <= (1e-12 if f64 else 2e-5) and np.abs(q.T @ q - np.eye(400)).max() <= (1e-12 if f64 else 2e-5)


def _with_coop_panel(on, fn):
    from rusty_compression_amd import _lib

    ctx = _lib.default_context()
    ctx.set_option(_lib.RC_OPT_COOP_PANEL, 1 if on else 0)
    try:
        return fn()
    finally:
        ctx.set_option(_lib.RC_OPT_COOP_PANEL, 1)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("shape", [(157, 520), (301, 700), (300, 400), (1021, 1300), (333, 2000), (4400, 640), (3200, 600)])
def test_cooperative_panels_match_the_step_kernels_and_lapack(dtype, shape):
    """The cooperative register-resident panel (k_qrb_coop) against the step kernels (RC_OPT_COOP_PANEL = 0) and ?geqp3: odd
    row counts (the last 16-byte vector of a column is partly beyond the matrix), more columns than one launch has waves
    (non-candidates take the Y = V^T A / T-factor route), fewer (every column a candidate), panels ended by the tau test, and
    tall matrices whose first panels have more rows than a wave's registers hold (4096 in f32, 3072 in f64): those run on the
    step kernels and the factorization switches to cooperative panels once the active rows fit."""
    f64 = dtype == np.float64
    rng = np.random.default_rng(shape[0] * 7 + shape[1])
    a = o.random_approximate_low_rank_matrix(shape, 1.0, 1e-6 if f64 else 1e-3, rng, dtype)
    k = min(shape)
    oq, orr, oind = o.pivoted_qr(a)
    want = stable_prefix(orr, dtype)
    res = {}
    for coop in (True, False):
        q, r, ind = _with_coop_panel(coop, lambda: tuple(npy(t) for t in rc.pivoted_qr(a)))
        assert is_permutation(ind, shape[1])
        ns = agreed_pivot_prefix(ind[:k], r, oind[:k], orr[:k], dtype)
        assert (ns == want) if f64 else (ns >= want // 4), f"coop={coop}: {ns} of {want} pivots agree with ?geqp3"
        assert np.abs(q.T @ q - np.eye(k)).max() <= (1e-12 if f64 else 2e-5)
        assert rel(q @ r, a[:, ind]) <= (1e-13 if f64 else 1e-5)
        res[coop] = (q, r, ind)
    nsb = agreed_pivot_prefix(res[True][2][:k], res[True][1], res[False][2][:k], res[False][1], dtype)
    assert nsb >= (want if f64 else 1)
    assert rel(np.abs(np.diag(res[True][1]))[:nsb], np.abs(np.diag(res[False][1]))[:nsb]) <= (1e-10 if f64 else 1e-3)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_cooperative_panel_gives_way_when_the_candidates_do_not_fit(dtype):
    """600 columns of identical norm: every column ties at the candidate threshold, more than the cooperative launch has waves;
    it leaves the panel untouched and the step kernels factor it (positions in order, as ?geqp3 does)."""
    n = 600
    e = np.eye(n, dtype=dtype)
    q, r, ind = (npy(t) for t in rc.pivoted_qr(e))
    assert np.array_equal(ind, np.arange(n)) and np.abs(np.abs(r) - e).max() <= 1e-6
    rng = np.random.default_rng(3)
    u = np.linalg.qr(rng.standard_normal((700, n)))[0].astype(dtype)  # orthonormal columns: all norms 1 up to rounding
    q, r, ind = (npy(t) for t in rc.pivoted_qr(u))
    assert is_permutation(ind, n) and rel(q @ r, u[:, ind]) <= (1e-13 if dtype == np.float64 else 1e-5)


def test_batch_of_eight_gaussian_matrices_repeats_exactly_under_concurrency():
    """Eight cooperative panels of different matrices in flight (six admitted by the budget, two waiting at the gate): every
    permutation stays a permutation and every factor equals the one-matrix call's, round after round.  (A workgroup that had
    finished its last step used to write its part of the permutation while workgroup 0 was still reading the old occupant of
    that position: one duplicated column, only under this kind of load.  And with the lanes pipelined -- panels of some matrices
    beside the streaming kernels of others -- a header used to overtake its column under memory load, because the workgroup
    barrier does not wait for another wave's global stores: about one matrix in a thousand came out with a wrong T factor, right
    pivots, wrong C and Z.  tools/batch_repeat_diag.py is the long version of this test.)"""
    from rusty_compression_amd import batch

    mats = [rc.random_gaussian((4096, 4096), rc.Rng(500 + i), torch.float32) for i in range(8)]
    want = [batch.column_id_rank(a, 64) for a in mats]
    for _ in range(60):
        out = batch.batch_column_id(mats, 64)
        for (c, z, ind), (c1, z1, i1) in zip(out, want):
            assert torch.equal(ind, i1), "permutation differs from the one-matrix call"
            assert torch.equal(c, c1) and torch.equal(z, z1)
    assert sorted(npy(want[0][2]).tolist()) == list(range(4096))
    from rusty_compression_amd import _lib
    assert _lib.default_context().get_health() == 0


def test_rccl_self_gather_of_the_packed_factors():
    """rc_comm_* on one GPU (world 1): the packed buffer of a small batch goes through the library's RCCL gather unchanged.
    (The multi-rank layout logic is covered on the CPU: tests/test_dist_cpu.py.)"""
    from rusty_compression_amd import batch

    mats = [rc.random_gaussian((512, 384), rc.Rng(900 + i), torch.float32) for i in range(3)]
    packed = batch.batch_column_id_packed(mats, 24, lanes=2)
    comm = batch.Comm(1, 0, batch.Comm.unique_id())
    try:
        got = comm.gather(packed, 0)
    finally:
        comm.close()
    assert got is not None and torch.equal(got, packed)
    for (c, z, ind), a in zip(batch.unpack_factors(got, 3, 512, 384, 24), mats):
        c1, z1, i1 = batch.column_id_rank(a, 24)
        assert torch.equal(ind, i1) and torch.equal(c, c1) and torch.equal(z, z1)


def _decaying_matrix(n, sigma_min, dtype, seed):
    """The reference's test-matrix recipe (src/random_matrix.rs:70-93) at full size: A = U diag(geomspace(sigma_min, 1)) V^T with
    U, V the orthogonal factors of seeded Gaussians.  Input generation only: the factors come from torch's QR."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    u = torch.linalg.qr(torch.randn(n, n, dtype=torch.float64, device="cuda", generator=g)).Q
    v = torch.linalg.qr(torch.randn(n, n, dtype=torch.float64, device="cuda", generator=g)).Q
    sig = torch.logspace(0, float(np.log10(sigma_min)), n, dtype=torch.float64, device="cuda")
    return ((u * sig) @ v.T).to(dtype).contiguous()


def test_cfg5_rank64_column_id_4096_f32_gaussian():
    """configs[4] unit of work: 4096 x 4096 f32 N(0,1), rank-64 column ID through the truncated factorization.  The column
    norms of a Gaussian matrix agree to ~1 %, far inside what sgeqp3's f32 norm down-dating resolves after a few steps, so
    the pivot ORDER legitimately depends on summation order here: the agreed prefix is reported, the factors are held to
    the properties and to the approximation quality of LAPACK's own pivots (the exact-pivot set is the next test)."""
    from rusty_compression_amd import batch

    n, k = 4096, 64
    a = rc.random_gaussian((n, n), rc.Rng(500), torch.float32)
    c, z, ind = batch.column_id_rank(a, k)
    an, cn, zn, indn = npy(a), npy(c), npy(z), npy(ind)
    assert is_permutation(indn, n)
    assert rel(cn, an[:, indn[:k]]) <= 1e-4                      # C = A[:, col_ind[:k]]
    assert rel(zn[:, indn[:k]], np.eye(k)) <= 1e-5               # Z restricted to the chosen columns is the identity
    oq, orr, oind = o.pivoted_qr(an)                             # full sgeqp3 + sorgqr, ~4 s
    gq, gr, gi = (npy(t) for t in rc.pivoted_qr(a, rank=k))
    ns = agreed_pivot_prefix(gi, gr, oind, orr, np.float32)      # asserts that the first disagreement is a near tie
    # ... and EVERY pivot, before and after that point, is the largest remaining partial norm to within the accuracy sgeqp3 keeps
    # its down-dated f32 norms to (helpers.greedy_pivot_slack, evaluated in f64 from the factorization itself); the same
    # statistic of LAPACK's own factorization is printed beside it.  Bound: the down-dated norms are trusted until
    # (vn1 / vn2)^2 <= tol3z = sqrt(eps), i.e. they carry a relative error of up to ~eps / tol3z = sqrt(eps_f32) = 3.5e-4
    slack = greedy_pivot_slack(an, gr, gi, k)
    oslack = greedy_pivot_slack(an, orr[:k], oind, k)
    tie = 1e-3
    worst, oworst = max(slack), max(oslack)
    msg = (f"cfg5 Gaussian: agreed pivot prefix {ns} of {k}; worst pivot slack ours {worst:.2e} (step {int(np.argmax(slack))}), "
           f"sgeqp3 {oworst:.2e} (step {int(np.argmax(oslack))}); tie tolerance {tie}")
    print(msg)
    assert ns >= 1 and gi[0] == oind[0], msg
    assert worst <= tie, msg
    # position by position both factorizations report the same |r_jj| to the tie tolerance also after the pivots part ways
    dj = np.abs(np.abs(np.diag(gr)[:k]) - np.abs(np.diag(orr)[:k])) / np.abs(np.diag(orr)[:k])
    assert dj.max() <= 1e-2, msg + f"; |r_jj| ours vs sgeqp3 differ by {dj.max():.2e} at step {int(dj.argmax())}"
    ocid = o.QR(oq, orr, oind).compress("RANK", k).column_id()
    err_ours = np.linalg.norm(an - cn @ zn) / np.linalg.norm(an)
    err_ref = np.linalg.norm(an - ocid.c @ ocid.z) / np.linalg.norm(an)
    assert abs(err_ours - err_ref) <= 2e-3 * err_ref             # same approximation quality as LAPACK's pivots


def test_cfg5_decaying_spectrum_set_has_sgeqp3_pivots_exactly():
    """SURVEY.md 8(d), second cfg5 set: 4096 x 4096 f32 built by the decaying-spectrum recipe, so that the pivots are
    determined by the data: ALL 64 pivots equal sgeqp3's (a disagreement is accepted only where
    helpers.agreed_pivot_prefix proves a near tie), C = A[:, ind[:k]] and C, Z, C Z against the oracle's to 1e-4."""
    from rusty_compression_amd import batch

    n, k = 4096, 64
    a = _decaying_matrix(n, 1e-5, torch.float32, 5)
    an = npy(a)
    c, z, ind = batch.column_id_rank(a, k)
    cn, zn, indn = npy(c), npy(z), npy(ind)
    assert is_permutation(indn, n)
    oq, orr, oind = o.pivoted_qr(an)
    gq, gr, gi = (npy(t) for t in rc.pivoted_qr(a, rank=k))
    assert np.array_equal(gi, indn)                              # the ID reports the factorization's permutation
    ns = agreed_pivot_prefix(gi[:k], gr, oind[:k], orr[:k], np.float32)
    assert ns == k, f"only {ns} of {k} pivots agree with sgeqp3"
    assert rel(gr[:, indn.argsort()], orr[:k][:, oind.argsort()]) <= 1e-4   # R rows in original column order
    assert rel(gq, oq[:, :k]) <= 1e-4
    ocid = o.QR(oq, orr, oind).compress("RANK", k).column_id()
    assert rel(cn, an[:, oind[:k]]) <= 1e-5 and rel(cn, ocid.c) <= 1e-4
    assert rel(zn, ocid.z) <= 1e-4
    assert rel(cn @ zn, ocid.c @ ocid.z) <= 1e-4


def test_cfg5_batch_of_eight_on_one_gpu_packs_and_unpacks_exactly():
    """configs[4] per-GPU shard: 8 matrices through batch.batch_column_id on device tensors (rc_batch_column_id_f32 behind
    it), results identical to one-by-one calls, pack -> unpack round trip exact (the buffer the RCCL gather moves)."""
    from rusty_compression_amd import batch

    n, k = 4096, 64
    mats = [rc.random_gaussian((n, n), rc.Rng(500 + i), torch.float32) for i in range(8)]
    out = batch.batch_column_id(mats, k)
    assert len(out) == 8
    for i in (0, 3, 7):
        c1, z1, i1 = batch.column_id_rank(mats[i], k)
        assert torch.equal(out[i][2], i1) and torch.equal(out[i][0], c1) and torch.equal(out[i][1], z1)
    for (c, z, ind), a in zip(out, mats):
        indn = npy(ind)
        assert is_permutation(indn, n)
        assert rel(npy(c), npy(a[:, ind[:k]])) <= 1e-4              # C = Q R11 reproduces the selected columns
    packed = batch.pack_factors(out)
    assert packed.is_cuda and packed.numel() * packed.element_size() == 8 * batch.packed_bytes(n, n, k, 4)
    back = batch.unpack_factors(packed, 8, n, n, k)
    for (c, z, ind), (c2, z2, ind2) in zip(out, back):
        assert torch.equal(c, c2) and torch.equal(z, z2) and torch.equal(ind, ind2)


# ---------------------------------------------------------------- short-wide pivoted QR: cooperative / lazy / eager
WIDE_MODES = {"coop": (1, 1), "lazy": (0, 1), "eager": (0, 0)}  # (RC_OPT_WIDE_COOP_QRCP, RC_OPT_WIDE_LAZY_QRCP)


def _wide_mode(ctx, mode):
    from rusty_compression_amd import _lib

    coop, lazy = WIDE_MODES[mode]
    ctx.set_option(_lib.RC_OPT_WIDE_COOP_QRCP, coop)
    ctx.set_option(_lib.RC_OPT_WIDE_LAZY_QRCP, lazy)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("shape,smin", [((128, 8192), 1e-4), ((64, 512), 1e-5), ((33, 1000), 1e-3), ((200, 2048), 1e-6), ((128, 1031), 1e-5),
                                        ((256, 3000), 1e-5), ((2, 300), 1e-1)])
def test_wide_qrcp_paths_match_lapack_and_each_other(dtype, shape, smin):
    """The three implementations of the short-wide pivoted QR (one cooperative register-resident launch,
    the read-only lazy scheme, the eager Householder chain) against ?geqp3 + ?orgqr."""
    from rusty_compression_amd import _lib

    rng = np.random.default_rng(shape[0])
    a = o.random_approximate_low_rank_matrix(shape, 1.0, smin, rng, dtype)
    q, r, ind = o.pivoted_qr(a)
    ctx = _lib.default_context()
    f64 = dtype == np.float64
    results = {}
    for mode in WIDE_MODES:
        _wide_mode(ctx, mode)
        try:
            gq, gr, gi = (npy(t) for t in rc.pivoted_qr(a))
        finally:
            _wide_mode(ctx, "coop")
        assert ctx.get_health() == 0, mode
        results[mode] = (gq, gr, gi)
        ns = agreed_pivot_prefix(gi, gr, ind, r, dtype)
        assert is_permutation(gi, shape[1]), mode
        if f64:
            assert ns == stable_prefix(r, dtype), (mode, ns)
            assert rel(gr[:ns], r[:ns]) <= 1e-10, (mode, rel(gr[:ns], r[:ns]))
        assert rel(gq @ gr, a[:, gi]) <= (1e-13 if f64 else 5e-6), mode
        assert np.abs(gq.T @ gq - np.eye(shape[0])).max() <= (1e-13 if f64 else 1e-5), mode
    if f64:
        # the cooperative kernel performs the eager chain's arithmetic (same reflector applications): same pivots throughout
        ns = stable_prefix(r, dtype)
        assert np.array_equal(results["coop"][2][:ns], results["eager"][2][:ns])
        assert rel(results["coop"][1][:ns], results["eager"][1][:ns]) <= 1e-12
    # truncated factorization
    kk = max(shape[0] // 2, 1)
    gq, gr, gi = (npy(t) for t in rc.pivoted_qr(a, rank=kk))
    if f64:
        assert np.array_equal(gi[:kk], ind[:kk]) and rel(gq, q[:, :kk]) <= 1e-9
        assert rel(o.apply_permutation_matrix(gr, gi, "COLINV"), o.apply_permutation_matrix(r[:kk], ind, "COLINV")) <= 1e-10


_WQ_STAGES_SNIPPET = r"""
import hashlib, sys
import numpy as np, torch
import rusty_compression_amd as rc
out = []
for dt, shape, seed in ((torch.float64, (128, 8192), 1), (torch.float64, (100, 5000), 2), (torch.float32, (128, 4096), 3), (torch.float64, (200, 3000), 4),
                        (torch.float64, (64, 2048), 5), (torch.float64, (120, 8192), 6)):
    a = rc.random_gaussian(shape, rc.Rng(seed), dt)
    for rank in (None, shape[0] // 2 + 3):
        q, r, ind = rc.pivoted_qr(a) if rank is None else rc.pivoted_qr(a, rank=rank)
        h = hashlib.sha256()
        for t in (q, r, ind):
            h.update(t.contiguous().cpu().numpy().tobytes())
        out.append(h.hexdigest())
print("DIGESTS " + " ".join(out))
"""


def test_staged_wide_coop_qrcp_equals_the_single_launch_bit_for_bit():
    """Round 3: k_wq_coop runs in shrinking stages (steps 0..63 on 32 workgroups, 64..95 on 16, 96..127 on 16 half-CU workgroups for
    128 x 8192), the column state (positions, ?laqp2's two norm vectors) handed over through global memory.  Q, R and the permutation
    must be bit for bit those of the single launch (RC_WQ_STAGES=0, the round-2 kernel schedule), full and truncated, f64 and f32,
    also for row counts that are not a multiple of the stage granule -- and the staged result is the one the LAPACK comparisons of
    test_wide_qrcp_paths_match_lapack_and_each_other hold to ?geqp3."""
    import os
    import subprocess
    import sys

    def digests(env):
        res = subprocess.run([sys.executable, "-c", _WQ_STAGES_SNIPPET], env=dict(os.environ, **env), capture_output=True, text=True, timeout=600,
                             cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
        assert res.returncode == 0, res.stdout[-1500:] + res.stderr[-1500:]
        return [ln for ln in res.stdout.splitlines() if ln.startswith("DIGESTS ")][0].split()[1:]

    staged, single = digests({"RC_WQ_STAGES": "1"}), digests({"RC_WQ_STAGES": "0"})
    assert len(staged) == 12 and staged == single, [i for i, (x, y) in enumerate(zip(staged, single)) if x != y]


_QRCP_OPTIMISTIC_SNIPPET = r"""
import hashlib, os, sys
import numpy as np, torch
import rusty_compression_amd as rc
from rusty_compression_amd import batch
out = []
def dig(ts):
    h = hashlib.sha256()
    for t in ts:
        h.update(t.contiguous().cpu().numpy().tobytes())
    return h.hexdigest()
# (a) Gaussian: every panel makes its 32 steps (the optimistic check holds); (b) decaying spectrum: panels end early on the tau test
# (the check fails, the matrix is restored and redone panel by panel); (c) three panels, ragged shape, f64
g = rc.random_gaussian((4096, 4096), rc.Rng(11), torch.float32)
def decaying(n, smin, seed):   # the reference's recipe (src/random_matrix.rs:70-93) with torch's QR on the device: input generation only
    gen = torch.Generator(device="cuda").manual_seed(seed)
    u = torch.linalg.qr(torch.randn(n, n, dtype=torch.float64, device="cuda", generator=gen)).Q
    v = torch.linalg.qr(torch.randn(n, n, dtype=torch.float64, device="cuda", generator=gen)).Q
    return ((u * torch.logspace(0, float(np.log10(smin)), n, dtype=torch.float64, device="cuda")) @ v.T).to(torch.float32).contiguous()
d = decaying(4096, 1e-5, 5)
r = rc.random_gaussian((1500, 2100), rc.Rng(12), torch.float64)
for a, k in ((g, 64), (d, 64), (r, 80), (g, 40)):
    out.append(dig(batch.column_id_rank(a, k)))
mats = [rc.random_gaussian((2048, 2048), rc.Rng(20 + i), torch.float32) for i in range(5)] + [d[:2048, :2048].contiguous()]
for res in batch.batch_column_id(mats, 48, lanes=4):
    out.append(dig(res))
print("DIGESTS " + " ".join(out))
"""


def test_optimistic_blocked_qrcp_equals_the_panel_by_panel_schedule_bit_for_bit():
    """Round 3: the truncated blocked QRCP enqueues all its panels on their usual outcome and checks the panels' states once
    (kernels_qrblk.hip, qrb_issue_optimistic); a failed check restores the working matrix and runs panel by panel.  Both outcomes
    -- check holds (Gaussian), check fails (decaying spectrum: the tau test ends panels early) -- and the batch schedule built on it
    must give the bits of the per-panel schedule (RC_QRCP_OPTIMISTIC=0, RC_BATCH_OPTIMISTIC=0)."""
    import os
    import subprocess
    import sys

    def digests(env):
        res = subprocess.run([sys.executable, "-c", _QRCP_OPTIMISTIC_SNIPPET], env=dict(os.environ, **env), capture_output=True, text=True, timeout=600,
                             cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
        assert res.returncode == 0, res.stdout[-1500:] + res.stderr[-1500:]
        return [ln for ln in res.stdout.splitlines() if ln.startswith("DIGESTS ")][0].split()[1:]

    opt, plain = digests({"RC_QRCP_OPTIMISTIC": "1", "RC_BATCH_OPTIMISTIC": "1"}), digests({"RC_QRCP_OPTIMISTIC": "0", "RC_BATCH_OPTIMISTIC": "0"})
    assert len(opt) == 10 and opt == plain, [i for i, (x, y) in enumerate(zip(opt, plain)) if x != y]


_SCHEDULING_SNIPPET = r"""
import ctypes, hashlib
import torch
import rusty_compression_amd as rc
from rusty_compression_amd import _lib
CT = rc.CompressionType
out = []
def dig(ts):
    h = hashlib.sha256()
    for t in ts:
        h.update(t.contiguous().cpu().numpy().tobytes())
    return h.hexdigest()
# QRTraits::column_id / LQTraits::row_id through the Z kernel (rank-deficient branch), tall, wide and square inputs, f64 and f32
for dt, shape, k, seed in ((torch.float64, (300, 200), 50, 1), (torch.float64, (64, 2048), 40, 2), (torch.float32, (500, 700), 96, 3)):
    a = rc.random_gaussian(shape, rc.Rng(seed), dt)
    cid = rc.QR.compute_from(a).compress(CT.RANK(k)).column_id()
    rid = rc.LQ.compute_from(a).compress(CT.RANK(k)).row_id()
    out.append(dig((cid.c, cid.z, cid.col_ind, rid.x, rid.r, rid.row_ind)))
# the fused cfg3 call at a reduced size: B = Q^H A read in place by the cooperative QRCP, then overwritten by the SVD consumer
m = n = 2048; k, p = 64, 5
a = rc.random_gaussian((m, n), rc.Rng(9), torch.float64)
mk = lambda r, c: torch.empty((r, c), dtype=torch.float64, device="cuda")
b = dict(range_q=mk(m, k), u=mk(m, k), s=torch.empty(k, dtype=torch.float64, device="cuda"), vt=mk(k, n), qr_q=mk(m, k), qr_r=mk(k, n),
         qr_ind=torch.empty(n, dtype=torch.int64, device="cuda"), id_c=mk(m, k), id_z=mk(k, n))
o_ = _lib.rc_rsvd_id_out(_lib.mat(b["range_q"]), _lib.mat(b["u"]), ctypes.c_void_p(b["s"].data_ptr()), _lib.mat(b["vt"]), _lib.mat(b["qr_q"]), _lib.mat(b["qr_r"]),
                         ctypes.c_void_p(b["qr_ind"].data_ptr()), _lib.mat(b["id_c"]), _lib.mat(b["id_z"]))
_lib.default_context().call("rc_rsvd_id_f64", _lib.mat(a), ctypes.c_int64(k), ctypes.c_int64(p), _lib.mat(None), ctypes.c_uint64(3), ctypes.byref(o_))
torch.cuda.synchronize()
out.append(dig(b.values()))
print("DIGESTS " + " ".join(out))
"""


def test_scheduling_switches_give_identical_bits():
    """include/rusty_compression_amd.h, "Reproducibility": RC_ID_FUSED (Z of the ID in one launch instead of identity + copy + triangular
    solve + inverse permutation + gather) and RC_QRCP_KEEP_DIRECT (the cooperative QRCP reads B = Q^H A where it lies instead of a
    working copy) only change how the same arithmetic is issued: every output bit for bit."""
    import os
    import subprocess
    import sys

    def digests(env):
        res = subprocess.run([sys.executable, "-c", _SCHEDULING_SNIPPET], env=dict(os.environ, **env), capture_output=True, text=True, timeout=600,
                             cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
        assert res.returncode == 0, res.stdout[-1500:] + res.stderr[-1500:]
        return [ln for ln in res.stdout.splitlines() if ln.startswith("DIGESTS ")][0].split()[1:]

    new, old = digests({"RC_ID_FUSED": "1", "RC_QRCP_KEEP_DIRECT": "1"}), digests({"RC_ID_FUSED": "0", "RC_QRCP_KEEP_DIRECT": "0"})
    assert len(new) == 4 and new == old, [i for i, (x, y) in enumerate(zip(new, old)) if x != y]


def test_wide_coop_qrcp_ties_take_the_first_position():
    """Equal column norms everywhere: idamax semantics = lowest position first, across workgroup boundaries."""
    m, n = 16, 1024
    a = np.zeros((m, n))
    for c in range(n):
        a[c % m, c] = 1.0  # every column has norm exactly 1; columns c and c + 16 are identical
    q, r, ind = o.pivoted_qr(a)
    gq, gr, gi = (npy(t) for t in rc.pivoted_qr(a))
    assert np.array_equal(gi[:m], ind[:m])
    assert rel(gq @ gr, a[:, gi]) <= 1e-14


def test_wide_coop_qrcp_many_streams_in_flight():
    """Eight streams replay captured cooperative factorizations at once: the device-wide CU budget keeps the
    grid barriers live (health word stays 0) and every stream reproduces its eager result bit for bit."""
    import ctypes

    from rusty_compression_amd import _lib

    lib = _lib.lib()
    lanes = []
    for s in range(8):
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            ctx = _lib.Context(torch.cuda.current_device(), st.cuda_stream)
            g = torch.Generator(device="cpu").manual_seed(100 + s)
            a = torch.randn(128, 8192, dtype=torch.float64, generator=g).cuda()
            q = torch.empty(128, 128, dtype=torch.float64, device="cuda")
            r = torch.empty(128, 8192, dtype=torch.float64, device="cuda")
            ind = torch.empty(8192, dtype=torch.int64, device="cuda")
            args = (_lib.mat(a), _lib.mat(q), _lib.mat(r), ctypes.c_void_p(ind.data_ptr()))
            ctx.call("rc_pivoted_qr_f64", *args)
            ctx.synchronize()
            ref = (q.clone(), r.clone(), ind.clone())
            graph = ctypes.c_void_p(None)
            ctx.check(lib.rc_graph_begin_capture(ctx._h))
            ctx.call("rc_pivoted_qr_f64", *args)
            ctx.check(lib.rc_graph_end_capture(ctx._h, ctypes.byref(graph)))
            q.zero_(); r.zero_(); ind.zero_()
            lanes.append(dict(ctx=ctx, graph=graph, out=(q, r, ind), ref=ref, keep=(a, st)))
    for _ in range(6):
        for ln in lanes:
            ln["ctx"].check(lib.rc_graph_launch(ln["ctx"]._h, ln["graph"]))
    for ln in lanes:
        ln["ctx"].synchronize()
    for ln in lanes:
        assert ln["ctx"].get_health() == 0
        for got, want in zip(ln["out"], ln["ref"]):
            assert torch.equal(got, want)
        an, qn, rn, indn = npy(ln["keep"][0]), npy(ln["out"][0]), npy(ln["out"][1]), npy(ln["out"][2])
        assert rel(qn @ rn, an[:, indn]) <= 1e-13
        ln["ctx"].check(lib.rc_graph_destroy(ln["ctx"]._h, ln["graph"]))
        ln["ctx"].close()


def test_first_call_of_fresh_contexts_on_recycled_memory_matches_a_warm_context():
    """The first call of a context runs on workspace memory the allocator hands out fresh -- here the blocks the previous
    context (which worked on ANOTHER matrix) has just released, in the same roles.  The fused Jacobi's tagged words (sweep count,
    sorted positions: "(epoch << 8) | payload") used to be trusted uncleared, and every context's first epoch was 0: the previous
    context's words passed for this one's and V's columns went to the wrong places (one wrong `vt` among 16 contexts' first calls
    at cfg3 size, nothing flagged).  Every fresh context must reproduce the warm context's factors bit for bit.  (What the
    allocator hands out here is not under the test's control; the next test, with poisoned workspace, is the one that fails on the
    old behaviour.)"""
    import ctypes

    from rusty_compression_amd import _lib

    m, n, k, p = 4096, 4096, 128, 5
    mats = [rc.random_gaussian((m, n), rc.Rng(77 + j), torch.float64) for j in range(2)]

    def run(ctx, a):
        mk = lambda r, c: torch.zeros((r, c), dtype=torch.float64, device="cuda")  # noqa: E731
        b = dict(range_q=mk(m, k), u=mk(m, k), s=torch.zeros(k, dtype=torch.float64, device="cuda"), vt=mk(k, n), qr_q=mk(m, k), qr_r=mk(k, n),
                 qr_ind=torch.zeros(n, dtype=torch.int64, device="cuda"), id_c=mk(m, k), id_z=mk(k, n))
        out = _lib.rc_rsvd_id_out(_lib.mat(b["range_q"]), _lib.mat(b["u"]), ctypes.c_void_p(b["s"].data_ptr()), _lib.mat(b["vt"]), _lib.mat(b["qr_q"]),
                                  _lib.mat(b["qr_r"]), ctypes.c_void_p(b["qr_ind"].data_ptr()), _lib.mat(b["id_c"]), _lib.mat(b["id_z"]))
        ctx.call("rc_rsvd_id_f64", _lib.mat(a), ctypes.c_int64(k), ctypes.c_int64(p), _lib.mat(None), ctypes.c_uint64(7), ctypes.byref(out))
        ctx.synchronize()
        return b

    warm = _lib.Context(torch.cuda.current_device(), torch.cuda.current_stream().cuda_stream)
    run(warm, mats[0])
    want = [run(warm, a) for a in mats]
    for a, w in zip(mats, want):
        an, rq = npy(a), npy(w["range_q"])
        assert rel((npy(w["u"]) * npy(w["s"])) @ npy(w["vt"]), rq @ (rq.T @ an)) <= 1e-10
    for i in range(12):
        ctx = _lib.Context(torch.cuda.current_device(), torch.cuda.current_stream().cuda_stream)
        got = run(ctx, mats[i % 2])
        assert ctx.get_health() == 0
        for f in want[i % 2]:
            assert torch.equal(got[f], want[i % 2][f]), f"fresh context {i}: {f} differs from the warm context's"
        ctx.close()  # releases its workspace: the next context's first call gets these blocks
    warm.close()


def test_results_do_not_depend_on_what_fresh_workspace_memory_holds():
    """tests/poison_worker.py in two fresh processes, the second with RC_DEBUG_POISON_WORKSPACE=1 (workspace memory new to a context
    is filled with small integers before it is handed out): every output digest must be the same.  With the round-2 behaviour of
    the fused Jacobi (hand-over words not cleared before a launch, every context starting at epoch 0) the poisoned run differs in
    the SVD outputs."""
    import json
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

    def digests(extra):
        env = dict(os.environ, **extra)
        res = subprocess.run([sys.executable, os.path.join(root, "tests", "poison_worker.py")], env=env, capture_output=True, text=True, timeout=600)
        assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
        line = [ln for ln in res.stdout.splitlines() if ln.startswith("DIGESTS ")][-1]
        return json.loads(line[len("DIGESTS "):])

    plain, poisoned = digests({"RC_DEBUG_POISON_WORKSPACE": "0"}), digests({"RC_DEBUG_POISON_WORKSPACE": "1"})
    assert plain.keys() == poisoned.keys() and len(plain) >= 9
    assert plain == poisoned, {k: (plain[k], poisoned[k]) for k in plain if plain[k] != poisoned[k]}


def test_cpp_mirror_runs_the_reference_examples(tmp_path):
    """include/rusty_compression.hpp (compiled host side over the C ABI) running the reference's two
    example programs (examples/interpolative_decomposition.rs, examples/adaptive_sampling.rs)."""
    import subprocess

    from tests.test_abi_cpu import build_cpp_mirror_examples

    exe = build_cpp_mirror_examples(tmp_path)
    res = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(res.stdout)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "ALL OK" in res.stdout


def test_cpp_twin_of_the_rust_crate_passes_the_reference_unit_tests(tmp_path):
    """tests/cpp/reference_tests.cpp: the reference's own unit tests (src/pivoted_qr.rs:193-317, src/qr.rs:418-616,
    src/svd.rs:193-321, src/col_interp_decomp.rs:163-242, src/row_interp_decomp.rs:163-236, src/permutation.rs:187-240) for
    f32 / f64 / c32 / c64, thin / thick, against the C++ mirror -- the compiled twin of bindings/rust/tests/reference_tests.rs."""
    import subprocess

    from tests.test_abi_cpu import build_cpp_mirror_examples

    exe = build_cpp_mirror_examples(tmp_path, "reference_tests.cpp")
    res = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(res.stdout[-4000:])
    assert res.returncode == 0, res.stdout[-6000:] + res.stderr
    assert "95 tests, 0 failed" in res.stdout


@pytest.mark.parametrize("dtype,n", [(np.float64, 32), (np.float64, 64), (np.float64, 128), (np.float64, 100), (np.float64, 140),
                                     (np.float32, 150), (np.float32, 192)])
def test_jacobi_lds_instance_of_every_core_size(dtype, n):
    """The LDS Jacobi picks its instance from the size of the core: n = 32, 64, 128 the bound-free instance (n = 16 lanes x rows
    per lane) with the right vectors accumulated in the same launch; n = 100 the bounded instance, same launch; f64 n = 140 (70
    pair slots on 64 lane groups, column pitch n | 1 because the padded pitch needs 163 KB of LDS) and f32 n = 150 / 192 the
    pair-slot loop with a separate replay of V.  Singular values, U S V^T and the orthogonality of U and V against numpy:
    1e-12 in f64, the f32 bounds of the larger cores (test_svd_cores_beyond_the_lds_limit) in f32."""
    from rusty_compression_amd import _lib

    f64 = dtype == np.float64
    rng = np.random.default_rng(n)
    if f64:
        a = rng.standard_normal((n, n)) @ np.diag(np.geomspace(1.0, 1e-9, n)) @ rng.standard_normal((n, n))
    else:
        a = rng.standard_normal((n, n)).astype(np.float32)
    _lib.default_context().get_health()  # (read and cleared: only this test's bits count below)
    u, s, vt = (npy(t) for t in rc.compute_svd(torch.from_numpy(a).cuda()))
    sref = np.linalg.svd(a.astype(np.float64), compute_uv=False)
    err = {"s": np.abs(s - sref).max() / sref[0], "USV^T": np.abs((u * s) @ vt - a).max() / sref[0],
           "U^T U": np.abs(u.T @ u - np.eye(n)).max(), "V V^T": np.abs(vt @ vt.T - np.eye(n)).max()}
    bound = {"s": 1e-12, "USV^T": 1e-12, "U^T U": 1e-12, "V V^T": 1e-12} if f64 else {"s": 2e-5, "USV^T": 5e-5, "U^T U": 1e-4, "V V^T": 1e-4}
    assert all(err[k] <= bound[k] for k in err), err
    assert _lib.default_context().get_health() == 0


def test_fused_jacobi_of_graded_128_column_cores():
    """The 128-column core of the headline pipeline (bound-free instance, right vectors accumulated in the same launch) on three
    graded inputs: U and V orthonormal to 1e-12, reconstruction to 1e-13, the right vectors complete (health word clean)."""
    from rusty_compression_amd import _lib

    rng = np.random.default_rng(12)
    _lib.default_context().get_health()  # (read and cleared: only this test's bits count below)
    for trial in range(3):
        a = rng.standard_normal((128, 128)) * np.geomspace(1.0, 10.0 ** -(4 * trial), 128)
        u, s, vt = (npy(t) for t in rc.compute_svd(a))
        assert np.abs(u.T @ u - np.eye(128)).max() <= 1e-12, trial
        assert np.abs(vt @ vt.T - np.eye(128)).max() <= 1e-12, trial
        assert np.linalg.norm((u * s) @ vt - a) / np.linalg.norm(a) <= 1e-13, trial
    assert _lib.default_context().get_health() == 0


@pytest.mark.parametrize("dtype,shape", [(np.float64, (512, 512)), (np.float32, (640, 384)), (np.float64, (300, 700))])
def test_captured_pivoted_qr_of_a_blocked_eligible_shape_agrees_with_the_eager_one(dtype, shape):
    """for shapes that are neither tall-skinny nor short-wide the EAGER call runs the blocked ?laqps panels while a call
    under hipGraph capture runs the per-step chain (the blocked path reads one scalar back per panel): two routes to the same
    factorization.  They are not promised to agree bit for bit (bit-reproducibility holds per setting: eager vs captured, and per
    RC_OPT_CONCURRENCY_HINT -- include/rusty_compression_amd.h); what is promised and checked here: the same pivots on the prefix the
    data determine, R and Q to the parity tolerance, both against ?geqp3."""
    import ctypes

    from rusty_compression_amd import _lib

    lib = _lib.lib()
    rng = np.random.default_rng(shape[0] + shape[1])
    an = o.random_approximate_low_rank_matrix(shape, 1.0, 1e-6 if dtype == np.float64 else 1e-3, rng, dtype)
    oq, orr, oind = o.pivoted_qr(an)
    k = min(shape)
    tdt = torch.float64 if dtype == np.float64 else torch.float32
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        ctx = _lib.Context(torch.cuda.current_device(), st.cuda_stream)
        a = torch.from_numpy(an).cuda()
        q, r = torch.empty((shape[0], k), dtype=tdt, device="cuda"), torch.empty((k, shape[1]), dtype=tdt, device="cuda")
        ind = torch.empty(shape[1], dtype=torch.int64, device="cuda")
        args = (_lib.mat(a), _lib.mat(q), _lib.mat(r), ctypes.c_void_p(ind.data_ptr()))
        name = "rc_pivoted_qr_f64" if dtype == np.float64 else "rc_pivoted_qr_f32"
        ctx.call(name, *args)
        ctx.synchronize()
        eq, er, ei = npy(q).copy(), npy(r).copy(), npy(ind).copy()
        graph = ctypes.c_void_p(None)
        ctx.check(lib.rc_graph_begin_capture(ctx._h))
        ctx.call(name, *args)
        ctx.check(lib.rc_graph_end_capture(ctx._h, ctypes.byref(graph)))
        q.zero_(); r.zero_(); ind.zero_()
        ctx.check(lib.rc_graph_launch(ctx._h, graph))
        ctx.synchronize()
        assert ctx.get_health() == 0
        gq, gr, gi = npy(q), npy(r), npy(ind)
        lib.rc_graph_destroy(ctx._h, graph)
        ctx.close()
    tol = TOL[np.dtype(dtype)]["factor"]
    for tag, (fq, fr, fi) in {"eager": (eq, er, ei), "captured": (gq, gr, gi)}.items():
        assert is_permutation(fi, shape[1]), tag
        ns = agreed_pivot_prefix(fi, fr, oind, orr, dtype)
        assert ns >= min(stable_prefix(orr, dtype), k) - (0 if dtype == np.float64 else 2), (tag, ns)
        assert rel(fq @ fr, an[:, fi]) <= (1e-13 if dtype == np.float64 else 5e-6), tag
        assert rel(fr[:ns, :ns], orr[:ns, :ns]) <= 10 * tol, tag
    ns = agreed_pivot_prefix(gi, gr, ei, er, dtype)
    assert ns >= min(stable_prefix(er, dtype), k) - (0 if dtype == np.float64 else 2), f"eager and captured part ways at pivot {ns}"
    assert rel(gr[:ns, :ns], er[:ns, :ns]) <= 10 * tol and rel(gq[:, :ns], eq[:, :ns]) <= 100 * tol


def test_graph_replay_matches_eager_and_survives_workspace_growth():
    """hipGraph capture of the fused pipeline (rc_graph_*): the replay reproduces the eager result bit
    for bit, and an eager call that outgrows the workspace afterwards must not invalidate the graph
    (the superseded arena is retired, not freed, while a graph is alive)."""
    import ctypes

    from rusty_compression_amd import _lib

    lib = _lib.lib()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        ctx = _lib.Context(torch.cuda.current_device(), st.cuda_stream)
        g = torch.Generator(device="cpu").manual_seed(5)
        a = torch.randn(1024, 768, dtype=torch.float64, generator=g).cuda()
        om = torch.randn(768, 40, dtype=torch.float64, generator=g).cuda()
        q = torch.empty(1024, 32, dtype=torch.float64, device="cuda")
        args = (_lib.mat(a), ctypes.c_int64(32), ctypes.c_int64(8), _lib.mat(om), ctypes.c_uint64(0), _lib.mat(q))
        ctx.call("rc_sample_range_by_rank_f64", *args)
        ctx.synchronize()
        q_eager = q.clone()
        graph = ctypes.c_void_p(None)
        ctx.check(lib.rc_graph_begin_capture(ctx._h))
        ctx.call("rc_sample_range_by_rank_f64", *args)
        ctx.check(lib.rc_graph_end_capture(ctx._h, ctypes.byref(graph)))
        q.zero_()
        ctx.check(lib.rc_graph_launch(ctx._h, graph))
        ctx.synchronize()
        assert torch.equal(q, q_eager)
        # a much larger eager call on the same context: the arena is outgrown and rebuilt
        big = torch.randn(4096, 1024, dtype=torch.float64, generator=g).cuda()
        bq = torch.empty(4096, 1024, dtype=torch.float64, device="cuda")
        br = torch.empty(1024, 1024, dtype=torch.float64, device="cuda")
        bi = torch.empty(1024, dtype=torch.int64, device="cuda")
        for _ in range(2):  # the second call rebuilds the arena the first one outgrew
            ctx.call("rc_pivoted_qr_f64", _lib.mat(big), _lib.mat(bq), _lib.mat(br), ctypes.c_void_p(bi.data_ptr()))
        assert rel(npy(bq) @ npy(br), npy(big)[:, npy(bi)]) < 1e-13
        ctx.synchronize()
        q.zero_()
        ctx.check(lib.rc_graph_launch(ctx._h, graph))
        ctx.synchronize()
        assert torch.equal(q, q_eager)
        assert ctx.get_health() == 0
        ctx.check(lib.rc_graph_destroy(ctx._h, graph))
        ctx.close()
