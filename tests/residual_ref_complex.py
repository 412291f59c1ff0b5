"""Host reference and error bounds of the complex batched residual norms (rc_lowrank_residual_batched_c64 / _c32), shared by the CPU and
the GPU tests.

The bounds follow from the arithmetic the C header states and nothing else.  A component (Re or Im) of an element of the rebuilt block is
a real dot product of 2 r terms (r products of real parts and r of imaginary parts, or the two mixed kinds), each term bounded by
|left| |W| in moduli; the factor W it is taken against costs one rounding per component (diag(s) right) and a real dot product of 2 r more
terms (the mid product); the subtraction costs one.  So each component of e is within g u (|a| + |left_r| |mid_r| diag|s_r| |right_r|) of
the exact one, g = 2 r + 2 without mid and s and 4 r + 4 with either, and the modulus of the complex error is at most sqrt(2) times that."""
import numpy as np

# the kernel's tiling (kernels_batched_residual_c.hip): rows of a per chunk, columns per tile, complex elements of a tile per thread
ROW_CHUNK = 32
COL_TILE = 64
PER_THREAD = 8


def real_dtype(dtype):
    return np.dtype(np.float32) if np.dtype(dtype) in (np.dtype(np.complex64), np.dtype(np.float32)) else np.dtype(np.float64)


def chain_length(m, n):
    """L_c(m, n): the longest chain of additions one of the two sums of squares passes through: the two components of a thread's 8
    elements of every (row chunk, column tile), then 6 butterfly steps over the lanes and 2 over the waves."""
    return 2 * PER_THREAD * -(-m // ROW_CHUNK) * -(-n // COL_TILE) + 8


def reference(a, left, right, mid, s, r):
    """(ah, e) in complex128: ah = left[:, :r] mid[:r, :r] diag(s[:r]) right[:r, :] (absent factors omitted, nothing conjugated), e = a - ah."""
    a128 = np.asarray(a, dtype=np.complex128)
    w = np.asarray(right, dtype=np.complex128)[:r]
    if s is not None:
        w = np.asarray(s, dtype=np.float64)[:r, None] * w
    if mid is not None:
        w = np.asarray(mid, dtype=np.complex128)[:r, :r] @ w
    ah = np.asarray(left, dtype=np.complex128)[:, :r] @ w
    return ah, a128 - ah


def bound(a, left, right, mid, s, r, dtype, L):
    """(B, err_bound, nrm_bound): |e - e_ref| <= B elementwise (moduli), |err - ||e_ref||_F| <= err_bound, |nrm - ||a||_F| <= nrm_bound.

    B = c sqrt(2) g u (|a| + |left_r| |mid_r| diag|s_r| |right_r|), moduli throughout, with u the unit roundoff of the real type of dtype,
    g = 2 r + 2 without mid and s and 4 r + 4 with either, c = 1 for complex64 and 2 for complex128 (the complex128 host reference carries
    an error of the same size).  The sums of squares run in f64 over chains of at most L additions and the root is rounded to the real
    type: (L + 16) 2^-53 + u relative."""
    u = float(np.finfo(real_dtype(dtype)).eps) / 2
    c = 1.0 if real_dtype(dtype) == np.float32 else 2.0
    g = 2 * r + 2 if mid is None and s is None else 4 * r + 4
    w = np.abs(np.asarray(right, dtype=np.complex128)[:r])
    if s is not None:
        w = np.abs(np.asarray(s, dtype=np.float64))[:r, None] * w
    if mid is not None:
        w = np.abs(np.asarray(mid, dtype=np.complex128)[:r, :r]) @ w
    a128 = np.asarray(a, dtype=np.complex128)
    B = c * np.sqrt(2.0) * g * u * (np.abs(a128) + np.abs(np.asarray(left, dtype=np.complex128)[:, :r]) @ w)
    _, e_ref = reference(a, left, right, mid, s, r)
    rel = (L + 16) * 2.0 ** -53 + u
    return B, float(np.linalg.norm(B)) + rel * float(np.linalg.norm(e_ref)), rel * float(np.linalg.norm(a128))


def emulate(a, left, right, mid, s, r):
    """The contract's arithmetic in NumPy in the real type of a, component by component: every product and every sum rounded to that type
    (not fused); diag(s) right one rounding per component; the mid product over ascending p with the four real products of a term in the
    order re += mid_re w_re, re += (-mid_im) w_im, im += mid_re w_im, im += mid_im w_re; the rebuild in steps of four inner indices, Re
    taking the four left_re W_re then the four (-left_im) W_im, Im the four left_re W_im then the four left_im W_re; the residual one
    rounding per component, the squares accumulated in float64 and the root rounded to the real type.  Returns (err, nrm, e)."""
    rt = real_dtype(a.dtype)
    f = lambda x: np.ascontiguousarray(x, dtype=rt)  # noqa: E731
    w_re, w_im = f(right[:r].real), f(right[:r].imag)
    if s is not None:
        sr = f(s[:r])[:, None]
        w_re, w_im = (sr * w_re).astype(rt), (sr * w_im).astype(rt)
    if mid is not None:
        m_re, m_im = f(mid[:r, :r].real), f(mid[:r, :r].imag)
        re, im = np.zeros_like(w_re), np.zeros_like(w_im)
        for p in range(r):
            re = (re + (m_re[:, p:p + 1] * w_re[p:p + 1]).astype(rt)).astype(rt)
            re = (re + (-m_im[:, p:p + 1] * w_im[p:p + 1]).astype(rt)).astype(rt)
            im = (im + (m_re[:, p:p + 1] * w_im[p:p + 1]).astype(rt)).astype(rt)
            im = (im + (m_im[:, p:p + 1] * w_re[p:p + 1]).astype(rt)).astype(rt)
        w_re, w_im = re, im
    l_re, l_im = f(left[:, :r].real), f(left[:, :r].imag)
    re, im = np.zeros(a.shape, dtype=rt), np.zeros(a.shape, dtype=rt)
    for l0 in range(0, r, 4):
        step = range(l0, min(l0 + 4, r))
        for l in step:
            re = (re + (l_re[:, l:l + 1] * w_re[l:l + 1]).astype(rt)).astype(rt)
        for l in step:
            re = (re + (-l_im[:, l:l + 1] * w_im[l:l + 1]).astype(rt)).astype(rt)
        for l in step:
            im = (im + (l_re[:, l:l + 1] * w_im[l:l + 1]).astype(rt)).astype(rt)
        for l in step:
            im = (im + (l_im[:, l:l + 1] * w_re[l:l + 1]).astype(rt)).astype(rt)
    e_re, e_im = (f(a.real) - re).astype(rt), (f(a.imag) - im).astype(rt)
    e = np.empty(a.shape, dtype=a.dtype)
    e.real, e.imag = e_re, e_im
    sq = lambda x: float(np.sum(x.astype(np.float64) ** 2))  # noqa: E731
    return rt.type(np.sqrt(sq(e_re) + sq(e_im))), rt.type(np.sqrt(sq(f(a.real)) + sq(f(a.imag)))), e


def gaussian_factors(rng, m, n, K, dtype, mode, wide_core=False):
    """One complex block and factors of inner width K for mode in ("none", "mid", "s", "both"): complex Gaussian left and right, mid
    complex Gaussian / sqrt(K), s real in [0.5, 1.5); with wide_core the core (s, else mid, else the columns of left) spans six orders
    of magnitude.  a is the product rounded to dtype plus noise of 1e-3 of its size, so the residual is small against a and the
    rebuild's rounding shows in it.  Returns dict(a, left, right, mid, s) with None for the absent factors; s in the real type."""
    cg = lambda *shape: (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) / np.sqrt(2.0)  # noqa: E731
    left = cg(m, K)
    right = cg(K, n)
    mid = cg(K, K) / np.sqrt(K) if mode in ("mid", "both") else None
    s = rng.uniform(0.5, 1.5, K) if mode in ("s", "both") else None
    if wide_core:
        scale = np.logspace(3, -3, K)
        if s is not None:
            s = s * scale
        elif mid is not None:
            mid = mid * scale[None, :]
        else:
            left = left * scale[None, :]
    f = {"left": left, "right": right, "mid": mid}
    f = {k: None if v is None else v.astype(dtype) for k, v in f.items()}
    f["s"] = None if s is None else s.astype(real_dtype(dtype))
    ah, _ = reference(np.zeros((m, n)), f["left"], f["right"], f["mid"], f["s"], K)
    size = np.sqrt(np.mean(np.abs(ah) ** 2)) if ah.size else 1.0
    f["a"] = (ah + 1e-3 * size * cg(m, n)).astype(dtype)
    return f
