"""Host model of the batched power iteration (rc_sketch_range_step_batched_* and the compositions of rusty_compression_amd.batch built on
it), in NumPy / SciPy f64 with the test matrix handed in: the pivoted QR of Y^T by scipy.linalg.qr, the orthonormalisation of P by
numpy.linalg.qr, and the ID rule of the batched column ID on the final sketch.  One block at a time; imported by
test_abi_batched_range_step_cpu.py (the conditions on the model itself) and test_gpu_batched_range_step.py (the device against it)."""
import numpy as np
import scipy.linalg

from oracle import ref_lapack as o

# (m, n, l, k) of the slowly decaying accuracy cases, and the tolerance example (spectrum 1 .. 1e-12, l = k = 40, tol = 1e-2)
DECAY_CASES = [(1030, 300, 40, 32), (2048, 96, 24, 16), (600, 130, 24, 16)]
TOL_CASE = (1030, 300, 40, 40)
TOL_SIGMA_MIN = 1e-12
TOL = 1e-2


def decaying(seed, m, n, sigma_min=1e-10):
    """The block of the sketch tests: singular values 1 .. sigma_min, geometric over min(m, n) values."""
    return o.random_approximate_low_rank_matrix((m, n), 1.0, sigma_min, np.random.default_rng(seed))


def gaussian(seed, l, m):
    return np.random.default_rng(seed).standard_normal((l, m))


def range_step(a, om):
    """Q (l x n, orthonormal rows spanning the rows of om a) and P = a Q^T."""
    a = np.asarray(a, dtype=np.float64)
    qt, _, _ = scipy.linalg.qr((np.asarray(om, dtype=np.float64) @ a).T, mode="economic", pivoting=True)
    return qt.T, a @ qt


def power_omega(a, om, iterations, orthonormalise_p=True):
    """The test matrix after `iterations` rounds; orthonormalise_p = False keeps P^T as it is (the variant the design rejects)."""
    om = np.asarray(om, dtype=np.float64)
    for _ in range(iterations):
        _, p = range_step(a, om)
        om = np.linalg.qr(p)[0].T if orthonormalise_p else p.T
    return om


def id_rule(rdiag, k, tol):
    """The rank rule of the batched IDs on the diagonal of R: the first j < kk with R_jj == 0 or |R_jj / R_00| < tol (tol > 0), else kk."""
    kk = min(k, len(rdiag))
    for j in range(kk):
        if rdiag[j] == 0 or (tol > 0 and abs(rdiag[j] / rdiag[0]) < tol):
            return j
    return kk


def column_id(a, om, k, tol=0.0):
    """The one-pass sketched column ID with test matrix om: (relative error of C Z, rank, |R_jj / R_00| of the steps taken)."""
    a = np.asarray(a, dtype=np.float64)
    _, rr, piv = scipy.linalg.qr(np.asarray(om, dtype=np.float64) @ a, mode="economic", pivoting=True)
    d = np.diag(rr)
    r = id_rule(d, k, tol)
    n = a.shape[1]
    z = np.zeros((r, n))
    z[:, piv[:r]] = np.eye(r)
    z[:, piv[r:]] = scipy.linalg.solve_triangular(rr[:r, :r], rr[:r, r:])
    ratios = np.abs(d[:min(k, len(d))] / d[0]) if d[0] != 0 else np.zeros(0)
    return np.linalg.norm(a - a[:, piv[:r]] @ z) / np.linalg.norm(a), r, ratios


def column_id_power(a, om, k, tol=0.0, iterations=1, orthonormalise_p=True):
    """sketch_column_id_rank_power_batched on one block."""
    return column_id(a, power_omega(a, om, iterations, orthonormalise_p), k, tol)


def svd_power(a, om, k, tol=0.0, iterations=1):
    """sketch_svd_rank_power_batched on one block: (relative error of U S Vt, rank), the SVD of P Q truncated by the SVD's rank rule."""
    a = np.asarray(a, dtype=np.float64)
    q, p = range_step(a, power_omega(a, om, iterations - 1))
    u, s, vt = np.linalg.svd(p @ q, full_matrices=False)
    kk = min(k, q.shape[0])
    r = kk
    for j in range(kk):
        if s[j] == 0 or (tol > 0 and s[j] / s[0] < tol):
            r = j
            break
    return np.linalg.norm(a - (u[:, :r] * s[:r]) @ vt[:r]) / np.linalg.norm(a), r


def best_rank(a, k):
    s = np.linalg.svd(np.asarray(a, dtype=np.float64), compute_uv=False)
    return np.sqrt(np.sum(s[k:] ** 2) / np.sum(s ** 2))
