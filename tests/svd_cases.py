"""Inputs and checks shared by the SVD route tests (host only: numpy, no GPU import).

Every input is built in f64 from a seeded default_rng and cast ONCE to the type under test; the f64 copy of the CAST input is what
the reference (numpy.linalg.svd, ?gesdd) factors, so the cast itself is never charged to the code under test.

Bounds (BOUNDS): the ones the existing tests of the same routes use -- f64 1e-12 throughout (test_jacobi_lds_instance_of_every_core_size,
test_svd_of_clustered_and_repeated_singular_values), f32 2e-5 / 1e-4 / 5e-5 (test_svd_cores_beyond_the_lds_limit) -- with ONE
difference: orthonormality is asked of ALL min(m, n) columns of U and V, the ones of tiny and zero singular values included."""
import numpy as np

BOUNDS = {
    np.dtype(np.float64): dict(sval=1e-12, orth=1e-12, recon=1e-12),
    np.dtype(np.float32): dict(sval=2e-5, orth=1e-4, recon=5e-5),
}
# Powers of four: the scaling is exact in f32.  The smallest keeps every squared column norm of a converged core above the smallest
# normal f32 (sigma_0 >~ 2^-16 * 10, noise >~ 2^-40 sigma_0: squares >~ 2^-105); smaller and larger scales: tests/dense_scale_cases.py.
SCALES = (1.0, 4.0 ** -5, 4.0 ** -8)


def _rng(*key):
    return np.random.default_rng([int(k) for k in key])


def gaussian(m, n, dtype, seed=0):
    return _rng(1, m, n, seed).standard_normal((m, n)).astype(dtype)


def low_rank_rho(m, n):
    return max(1, min(m, n) // 4)


def low_rank(m, n, scale, dtype, seed=0):
    """scale * X Y^T with rho = max(1, min(m, n) // 4) columns: numerically rank deficient after the cast."""
    rng = _rng(2, m, n, seed)
    rho = low_rank_rho(m, n)
    x, y = rng.standard_normal((m, rho)), rng.standard_normal((n, rho))
    return (scale * (x @ y.T)).astype(dtype)


def low_rank_complex(m, n, scale, dtype, seed=0):
    """scale * X Y^H with complex Gaussian factors of rho columns."""
    rng = _rng(3, m, n, seed)
    rho = low_rank_rho(m, n)
    x = rng.standard_normal((m, rho)) + 1j * rng.standard_normal((m, rho))
    y = rng.standard_normal((n, rho)) + 1j * rng.standard_normal((n, rho))
    return (scale * (x @ y.conj().T)).astype(dtype)


def gaussian_complex(m, n, dtype, seed=0):
    rng = _rng(4, m, n, seed)
    return (rng.standard_normal((m, n)) + 1j * rng.standard_normal((m, n))).astype(dtype)


def exact_zeros(m, n, dtype, seed=0):
    """Columns n // 3: and rows m // 2: zero: min(m, n) - min(n // 3, m // 2) singular values are EXACTLY zero."""
    a = _rng(5, m, n, seed).standard_normal((m, n)).astype(dtype)
    a[:, n // 3:] = 0
    a[m // 2:, :] = 0
    return a


def exact_zeros_rank(m, n):
    return min(n // 3, m // 2)


def clustered(m, n, dtype, seed=0):
    """Three families of clustered / repeated singular values, {name: matrix}.  In f32 the perturbations are 1e-4 / 1e-5 instead of
    1e-9 / 1e-12 so that they survive the cast."""
    f64 = np.dtype(dtype) == np.dtype(np.float64)
    r = min(m, n)
    rng = _rng(6, m, n, seed)
    qa = np.linalg.qr(rng.standard_normal((m, r)))[0]
    qb = np.linalg.qr(rng.standard_normal((n, r)))[0]
    p1, p2 = (1e-9, 1e-12) if f64 else (1e-4, 1e-5)
    return {
        "1 + %g r" % p1: ((qa * (1.0 + p1 * rng.standard_normal(r))) @ qb.T).astype(dtype),
        "all equal": (qa @ qb.T).astype(dtype),
        "two clusters": ((qa * np.where(np.arange(r) % 2 == 0, 1.0, 0.5 + p2 * np.arange(r))) @ qb.T).astype(dtype),
    }


def graded(n, dtype, seed=0):
    """G diag(2^-linspace(0, 30, n)): column norms graded over nine decades."""
    g = _rng(7, n, seed).standard_normal((n, n))
    return (g * 2.0 ** -np.linspace(0.0, 30.0, n)).astype(dtype)


def check_svd(a, u, s, vt, dtype, measured=None):
    """Asserts that (u, s, vt) is a thin SVD of `a` to BOUNDS[dtype] against numpy.linalg.svd of the f64 copy of `a`; returns the
    worst values {"sval", "orth_u", "orth_v", "recon"} (recon is 0.0 for the zero matrix, where it is not defined) and, before it
    asserts, copies them into the dict `measured` when one is given."""
    b = BOUNDS[np.dtype(dtype)]
    a64 = np.asarray(a, dtype=np.float64)
    m, n = a64.shape
    r = min(m, n)
    u, s, vt = (np.asarray(x, dtype=np.float64) for x in (u, s, vt))
    assert u.shape == (m, r) and s.shape == (r,) and vt.shape == (r, n), ("shape", u.shape, s.shape, vt.shape)
    assert np.all(np.isfinite(s)) and np.all(s >= 0), "s: not finite or negative"
    assert np.all(s[:-1] >= s[1:]), "s: not descending"
    assert np.all(np.isfinite(u)) and np.all(np.isfinite(vt)), "u / vt: not finite"
    s_ref = np.linalg.svd(a64, compute_uv=False)
    na = np.linalg.norm(a64)
    worst = {
        "sval": float(np.abs(s - s_ref).max() / s_ref[0]) if s_ref[0] > 0 else float(np.abs(s).max()),
        "orth_u": float(np.abs(u.T @ u - np.eye(r)).max()),
        "orth_v": float(np.abs(vt @ vt.T - np.eye(r)).max()),
        "recon": float(np.linalg.norm(a64 - (u * s) @ vt) / na) if na > 0 else 0.0,
    }
    if measured is not None:  # (the figures reach the caller also when an assertion below fails)
        measured.update(worst)
    assert worst["sval"] <= b["sval"], ("sval", worst)
    assert worst["orth_u"] <= b["orth"], ("orth U", worst)
    assert worst["orth_v"] <= b["orth"], ("orth V", worst)
    assert worst["recon"] <= b["recon"], ("recon", worst)
    return worst


# ---- the route table of rc_compute_svd, restated from jacobi_lds.hpp / kernels_svd.hip / kernels_tsqr.hip ----------------------
K_JACOBI_LDS_CAP = 160 * 1024 - 2048 - 64  # kJacobiLdsCap
K_LPP = 16                                 # lanes per column pair
K_LDS_MAX_ROWS_PER_LANE = 12               # the largest instance of launch_lds: n <= 16 * 12


def _size(dtype):
    return np.dtype(dtype).itemsize


def jacobi_lds_bytes(n, pitch, dtype):
    return (pitch * n + n) * _size(dtype) + n * 4 + 64


def jacobi_pitch(n, dtype):
    ld = ((n + 15) // 32) * 32 + 16
    return (n | 1) if jacobi_lds_bytes(n, ld, dtype) > K_JACOBI_LDS_CAP else ld


def core_is_lds(n, dtype):
    """jacobi_svd: the core runs in one CU's LDS unless it does not fit or has more than 16 * 12 columns."""
    return jacobi_lds_bytes(n, jacobi_pitch(n, dtype), dtype) <= K_JACOBI_LDS_CAP and n <= K_LPP * K_LDS_MAX_ROWS_PER_LANE


def last_lds_core(dtype):
    n = 1
    while core_is_lds(n + 1, dtype):
        n += 1
    return n


def core_is_fused(n):
    """launch_lds_impl: V is accumulated by a second workgroup of the same launch iff every pair slot has its own 16-lane group of
    the 1024 threads (n <= 128); larger LDS cores replay V from the rotation log in a second launch."""
    return ((n + 1) // 2) * K_LPP <= 1024


def tsqr_supported(m, r, dtype):
    """kernels_tsqr.hip: the CholeskyQR2 reduction takes the tall orientation m x r when this holds."""
    small_lds = (r * (r | 1) + 4 * r) * _size(dtype) + r * 4 + 256
    return r >= 2 and m >= 4 * r and m >= 1024 and small_lds <= 160 * 1024 - 2048


# ---- the cases of tests/test_gpu_svd_routes.py (tests/test_svd_cases_cpu.py sends the same inputs through LAPACK) ----------------
F64, F32 = np.dtype(np.float64), np.dtype(np.float32)
# the smallest core on each side of every decision of jacobi_svd, launch_lds and jacobi_pitch (r = min(m, n)):
#   f64 20 .. 128  bounded (20, 50, 100) and bound-free (32, 64, 128) instances, V accumulated in the same launch
#       129        first core with a separate replay of V, odd, 65 pair slots on 64 lane groups
#       141 / 142  last LDS core (pitch n | 1) / first core in global memory;  143: global, odd n with the dummy column
#   f32 32 .. 128  as above;  129 first replay core;  192 / 193 last LDS / first global core (odd);  194 global, even
CORE_SIZES = {F64: (20, 32, 50, 64, 100, 128, 129, 141, 142, 143), F32: (32, 64, 100, 128, 129, 192, 193, 194)}
# (only f32 is scaled: the threshold tests of the Jacobi kernels cannot underflow in f64 at these scales)
LOW_RANK_SCALES = {F64: (1.0,), F32: SCALES}


def reduction_sizes(dtype):
    return (64, 129, last_lds_core(dtype) + 1)


def reduction_shapes(r):
    """{name: shape} of the three non-square reductions to an r x r core."""
    tall = max(1024, 4 * r)
    return {"tall": (r + 37, r), "tall_chol": (tall, r), "wide_chol": (r, tall)}


def route_cases(dtype):
    """[(shape, generator name, scale)] of the dense route test."""
    dtype = np.dtype(dtype)
    out = []
    for r in CORE_SIZES[dtype]:
        out.append(((r, r), "gaussian", 1.0))
        out += [((r, r), "low_rank", sc) for sc in LOW_RANK_SCALES[dtype]]
        out.append(((r, r), "exact_zeros", 1.0))
    for r in reduction_sizes(dtype):
        for name, shape in reduction_shapes(r).items():
            out.append((shape, "gaussian", 1.0))
            out += [(shape, "low_rank", sc) for sc in LOW_RANK_SCALES[dtype]]
            if name == "tall_chol":
                out.append((shape, "exact_zeros", 1.0))
    return out


def make_case(shape, gen, scale, dtype):
    m, n = shape
    if gen == "gaussian":
        return gaussian(m, n, dtype)
    if gen == "low_rank":
        return low_rank(m, n, scale, dtype)
    if gen == "exact_zeros":
        return exact_zeros(m, n, dtype)
    raise KeyError(gen)


def case_id(case):
    (m, n), gen, scale = case
    return "%dx%d-%s%s" % (m, n, gen, "" if scale == 1.0 else "-4^%d" % round(np.log(scale) / np.log(4.0)))


GRADED_SIZES = {F64: (128, 141), F32: (64, 128)}
BATCHED_SHAPES = ((64, 64), (96, 40))


def batched_case(m, n, dtype, seed=0):
    """A batch of 5: matrices 1 and 3 are low_rank at scales 4^-5 and 4^-8, the others gaussian (complex: X Y^H, complex Gaussians)."""
    dtype = np.dtype(dtype)
    if dtype.kind == "c":
        mats = [gaussian_complex(m, n, dtype, seed + i) for i in range(5)]
        mats[1] = low_rank_complex(m, n, SCALES[1], dtype, seed)
        mats[3] = low_rank_complex(m, n, SCALES[2], dtype, seed)
    else:
        mats = [gaussian(m, n, dtype, seed + i) for i in range(5)]
        mats[1] = low_rank(m, n, SCALES[1], dtype, seed)
        mats[3] = low_rank(m, n, SCALES[2], dtype, seed)
    return np.stack(mats)
