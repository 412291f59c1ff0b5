"""Host model of the index-array contract of the C header (health bit 32), shared by the CPU and the GPU tests.

An index handed to a gather is either inside the source or rejected: the output column is then zero and the call raises bit 32.  An
inverse permutation starts at -1, so a position that no in-range entry names stays -1 and the gather that consumes it rejects it.
Everything a permutation-taking entry point returns is built from the two functions below plus plain f64 NumPy."""
import numpy as np

MODES = ("COL", "ROW", "COLINV", "ROWINV")  # RC_PERM_* = 0 .. 3
VMODES = ("INV", "NOINV")                   # RC_VPERM_* = 0, 1


def checked_gather(src, idx):
    """(out, rejected): out[:, j] = src[:, idx[j]] where 0 <= idx[j] < src.shape[1], else a zero column."""
    src = np.asarray(src)
    out = np.zeros((src.shape[0], len(idx)), dtype=src.dtype)
    rejected = False
    for j, s in enumerate(idx):
        s = int(s)
        if 0 <= s < src.shape[1]:
            out[:, j] = src[:, s]
        else:
            rejected = True
    return out, rejected


def checked_invert(perm, n):
    """inv[perm[i]] = i for the entries in range, starting from -1.  Returns a list of n tuples: the positions i that name each
    destination, in ascending order.  () is the -1 the device leaves; one member is a defined entry; where a value occurs twice the
    device's last writer is not defined and any member is admissible."""
    named = [[] for _ in range(n)]
    for i, e in enumerate(perm):
        e = int(e)
        if 0 <= e < n:
            named[e].append(i)
    return [tuple(v) for v in named]


def checked_invert_unique(perm, n):
    """checked_invert for an input without a duplicated in-range value, as an int64 array (-1 where unnamed): vectorised, for the
    sizes at which a Python loop would take seconds."""
    perm = np.asarray(perm, dtype=np.int64)
    ok = (perm >= 0) & (perm < n)
    assert np.unique(perm[ok]).size == int(ok.sum()), "a duplicated value has no unique inverse"
    inv = np.full(n, -1, dtype=np.int64)
    inv[perm[ok]] = np.nonzero(ok)[0]
    return inv


def any_inverse(adm):
    """One admissible inverse as an int64 array (-1 where unnamed, the first position where several name a destination)."""
    return np.array([v[0] if v else -1 for v in adm], dtype=np.int64)


def inverse_admissible(inv, adm):
    """True where the device's inverse entry is one the model admits."""
    return np.array([(int(e) in v) if v else int(e) == -1 for e, v in zip(inv, adm)], dtype=bool)


def gather_choices(src, adm):
    """The gather of `src` through every admissible inverse: a list, per destination column, of the admissible columns (each a 1-D
    array; a single zero column where the destination is unnamed), and whether the gather rejects an entry."""
    src = np.asarray(src)
    zero = np.zeros(src.shape[0], dtype=src.dtype)
    return [[src[:, p] for p in v] if v else [zero] for v in adm], any(not v for v in adm)


def admissible(out, choices):
    """True where column j of `out` is bit for bit one of choices[j]."""
    out = np.asarray(out)
    return np.array([any(np.array_equal(out[:, j], c) for c in cs) for j, cs in enumerate(choices)], dtype=bool)


def apply_matrix(mat, perm, mode):
    """rc_apply_permutation_matrix_*: (choices, rejected) with choices[j] the admissible values of column j of the output (COL, COLINV)
    or of row j (ROW, ROWINV)."""
    mat = np.asarray(mat)
    src = mat if mode.startswith("COL") else mat.T
    if mode.endswith("INV"):
        return gather_choices(src, checked_invert(perm, src.shape[1]))
    out, rejected = checked_gather(src, perm)
    return [[out[:, j]] for j in range(out.shape[1])], rejected


def apply_matrix_unique(mat, perm, mode):
    """The output of apply_matrix where it is unique (no destination named twice)."""
    choices, rejected = apply_matrix(mat, perm, mode)
    assert all(len(c) == 1 for c in choices)
    out = np.stack([c[0] for c in choices], axis=1)
    return (out if mode.startswith("COL") else out.T), rejected


def apply_vector(vec, perm, mode):
    """rc_apply_permutation_vector_*: the matrix modes ROWINV (INV) and ROW (NOINV) of the n x 1 matrix."""
    return apply_matrix(np.asarray(vec).reshape(-1, 1), perm, "ROWINV" if mode == "INV" else "ROW")


# --------------------------------------------------------------------------------------------------------------------------
# the column ID of given factors: Z = [I | R11^-1 R12] scattered by ind, C = Q R11
# --------------------------------------------------------------------------------------------------------------------------
def unit_roundoff(dtype):
    return float(np.finfo(np.dtype(dtype)).eps) / 2


def gamma(k, dtype):
    """gamma_k = k u / (1 - k u), the constant of the backward error of a k-term back substitution (Higham, Accuracy and Stability of
    Numerical Algorithms, 2nd ed., Theorem 8.5)."""
    u = unit_roundoff(dtype)
    return k * u / (1 - k * u)


def id_factors(rng, m, k, n, dtype):
    """(q, r): q random m x k; r k x n upper trapezoidal with |diagonal| in [1, 2] and random signs (unit-modulus phases for complex
    dtypes), the off-diagonal of R11 uniform in [-1, 1] / (2 k) -- R11 is strictly diagonally dominant by rows, its condition number
    small and independent of k -- and R12 standard normal."""
    dtype = np.dtype(dtype)
    cplx = dtype.kind == "c"

    def normal(*shape):
        return rng.standard_normal(shape) + (1j * rng.standard_normal(shape) if cplx else 0)

    r = np.zeros((k, n), dtype=np.complex128 if cplx else np.float64)
    off = rng.uniform(-1, 1, (k, k))
    if cplx:  # real and imaginary part uniform in [-1, 1] / sqrt 2: the modulus stays <= 1
        off = (off + 1j * rng.uniform(-1, 1, (k, k))) / np.sqrt(2)
    r[:, :k] = np.triu(off, 1) / (2 * k)
    mag = rng.uniform(1, 2, k)
    sign = np.exp(2j * np.pi * rng.uniform(0, 1, k)) if cplx else rng.choice([-1.0, 1.0], k)
    r[np.arange(k), np.arange(k)] = mag * sign
    r[:, k:] = normal(k, n - k)
    return normal(m, k).astype(dtype), r.astype(dtype)


def backward_error(r11, z12, r12, wide):
    """rho = ||R11 Z12 - R12||_F / || |R11| |Z12| ||_F evaluated in the type `wide`."""
    cw = np.clongdouble if np.dtype(wide) == np.longdouble else np.complex128
    w = cw if np.iscomplexobj(r11) else wide
    t, z, b = np.asarray(r11).astype(w), np.asarray(z12).astype(w), np.asarray(r12).astype(w)
    num = np.sqrt((np.abs(t @ z - b) ** 2).sum())
    den = np.sqrt(((np.abs(t) @ np.abs(z)) ** 2).sum())
    return float(num / den)


def wide_type(dtype):
    """The type rho is evaluated in: x86 extended for f64 and c64 data, f64 for f32 and c32."""
    return np.longdouble if np.dtype(dtype) in (np.dtype(np.float64), np.dtype(np.complex128)) else np.float64


def rho_factor():
    """2 gamma_k where np.longdouble is x86 extended; 3 gamma_k where it is no wider than 60 bits (then the evaluation of rho itself
    contributes an error of the size of the quantity it measures)."""
    return 2.0 if np.finfo(np.longdouble).nmant >= 60 else 3.0
