"""Host reference and error bounds of the batched residual norms (rc_lowrank_residual_batched_*), shared by the CPU and the GPU tests.

The bounds follow from the arithmetic the C header states and nothing else: an element of the rebuilt block is a dot product of r terms,
the factor it is taken against costs one rounding (diag(s) right) and r more (the mid product), and the subtraction one."""
import numpy as np

# the kernel's tiling (kernels_batched_residual.hip): rows of a per chunk, columns per tile, elements of a tile per thread
ROW_CHUNK = 32
COL_TILE = 64
PER_THREAD = 8


def chain_length(m, n):
    """L(m, n): the longest chain of additions one of the two sums of squares passes through: a thread's 8 elements of every
    (row chunk, column tile), then 6 butterfly steps over the lanes and 2 over the waves."""
    return PER_THREAD * -(-m // ROW_CHUNK) * -(-n // COL_TILE) + 8


def reference(a, left, right, mid, s, r):
    """(ah, e) in f64: ah = left[:, :r] mid[:r, :r] diag(s[:r]) right[:r, :] (absent factors omitted) and e = a - ah."""
    a64 = np.asarray(a, dtype=np.float64)
    w = np.asarray(right, dtype=np.float64)[:r]
    if s is not None:
        w = np.asarray(s, dtype=np.float64)[:r, None] * w
    if mid is not None:
        w = np.asarray(mid, dtype=np.float64)[:r, :r] @ w
    ah = np.asarray(left, dtype=np.float64)[:, :r] @ w
    return ah, a64 - ah


def bound(a, left, right, mid, s, r, dtype, L):
    """(B, err_bound, nrm_bound): |e - e_ref| <= B elementwise, |err - ||e_ref||_F| <= err_bound, |nrm - ||a||_F| <= nrm_bound.

    B = c g u (|a| + |left_r| |mid_r| diag|s_r| |right_r|) with u the unit roundoff of dtype, g = r + 2 without mid and s and 2 r + 4
    with either (the chain lengths of the rebuild, the pre-product and the subtraction), c = 1 in f32 and 2 in f64 (the f64 host reference
    carries an error of the same size).  The sums of squares run in f64 over chains of at most L additions and the root is rounded to
    dtype: (L + 16) 2^-53 + u relative."""
    u = float(np.finfo(dtype).eps) / 2
    c = 1.0 if np.dtype(dtype) == np.float32 else 2.0
    g = r + 2 if mid is None and s is None else 2 * r + 4
    w = np.abs(np.asarray(right, dtype=np.float64)[:r])
    if s is not None:
        w = np.abs(np.asarray(s, dtype=np.float64))[:r, None] * w
    if mid is not None:
        w = np.abs(np.asarray(mid, dtype=np.float64)[:r, :r]) @ w
    a64 = np.asarray(a, dtype=np.float64)
    B = c * g * u * (np.abs(a64) + np.abs(np.asarray(left, dtype=np.float64)[:, :r]) @ w)
    _, e_ref = reference(a, left, right, mid, s, r)
    rel = (L + 16) * 2.0 ** -53 + u
    return B, float(np.linalg.norm(B)) + rel * float(np.linalg.norm(e_ref)), rel * float(np.linalg.norm(a64))


def emulate(a, left, right, mid, s, r):
    """The contract's arithmetic in NumPy, in the dtype of a: products and sums rounded to that type in ascending inner index (not fused),
    diag(s) right rounded once, the residual one rounding, the squares accumulated in float64 and the root rounded to the type.
    Returns (err, nrm, e)."""
    dt = a.dtype
    w = right[:r].astype(dt)
    if s is not None:
        w = (s[:r, None].astype(dt) * w).astype(dt)
    if mid is not None:
        w2 = np.zeros_like(w)
        for p in range(r):
            w2 = (w2 + (mid[:r, p:p + 1].astype(dt) * w[p:p + 1]).astype(dt)).astype(dt)
        w = w2
    ah = np.zeros(a.shape, dtype=dt)
    for l in range(r):
        ah = (ah + (left[:, l:l + 1].astype(dt) * w[l:l + 1]).astype(dt)).astype(dt)
    e = (a - ah).astype(dt)
    e64, a64 = e.astype(np.float64), a.astype(np.float64)
    return dt.type(np.sqrt(np.sum(e64 * e64))), dt.type(np.sqrt(np.sum(a64 * a64))), e


def gaussian_factors(rng, m, n, K, dtype, mode, wide_core=False):
    """One block and factors of inner width K for mode in ("none", "mid", "s", "both"): Gaussian left and right, mid Gaussian / sqrt(K),
    s in [0.5, 1.5); with wide_core the core (s, else mid, else the columns of left) spans six orders of magnitude.  a is the product
    rounded to dtype plus noise of 1e-3 of its size, so the residual is small against a and the rebuild's rounding shows in it.
    Returns dict(a, left, right, mid, s) with None for the absent factors."""
    left = rng.standard_normal((m, K))
    right = rng.standard_normal((K, n))
    mid = rng.standard_normal((K, K)) / np.sqrt(K) if mode in ("mid", "both") else None
    s = rng.uniform(0.5, 1.5, K) if mode in ("s", "both") else None
    if wide_core:
        scale = np.logspace(3, -3, K)
        if s is not None:
            s = s * scale
        elif mid is not None:
            mid = mid * scale[None, :]
        else:
            left = left * scale[None, :]
    f = {"left": left, "right": right, "mid": mid, "s": s}
    f = {k: None if v is None else v.astype(dtype) for k, v in f.items()}
    ah, _ = reference(np.zeros((m, n)), f["left"], f["right"], f["mid"], f["s"], K)
    size = np.sqrt(np.mean(ah * ah)) if ah.size else 1.0
    f["a"] = (ah + 1e-3 * size * rng.standard_normal((m, n))).astype(dtype)
    return f
