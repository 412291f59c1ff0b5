"""Every arm of the GEMM dispatch, bit for bit: exact data, general alpha / beta, every C view, both sides of every threshold.

gemm<T> (kernels_gemm.hip, kernels_gemm_pipe.hip) picks one of about three dozen instantiations by shape, layout and alignment;
each family (k_gemm_f64q, k_gemm_f64p, k_gemm_f64r, k_gemm_mfma<float>, then k_splitk_reduce / k_splitk_reduce_t) has its own
epilogue, ragged-tile guards and staging of out-of-range rows.  The calls here go through rc_gemm_* as the library's own callers
do, and are compared with a plain f64 host product.

Exact data.  A and B are integers in [-4, 4], C0 integers in [-64, 64], alpha in {1, -1, 2, 1/2}, beta in {0, 1, -2}, K <= 2100.
Every product a_ik b_kj is an integer of magnitude <= 16, so every partial sum over any subset of k, in any order -- a K tile, a
split-K slab, the slab sum -- is an integer of magnitude <= 16 * 2100 = 33 600, and alpha * sum + beta * c0 is a multiple of 1/2 of
magnitude <= 2 * 33 600 + 2 * 64 = 67 328.  Twice that is below 2^24, so every one of these numbers is representable in f32 (24
significand bits), a fortiori in f64: no operation of any correct kernel rounds, whatever its summation order, and the result
must EQUAL alpha * (A @ B) + beta * C0 (the host's f64 BLAS product of these integers is exact for the same reason).  The bound
is asserted below (test_magnitude_precondition_of_the_exact_data).  beta = 0 runs over a C full of NaN.

The operands of the sweeps are leading sub-views of ONE master matrix per layout and staging width, uploaded once: what lies
beyond a product's M, N or K in memory is other non-zero integers (or NaN, in the masking test), never zeros.
"""
import numpy as np
import pytest
import torch

from tests.gemm_cases import GEMM_DISPATCH, gemm, gemm_operand, gemm_traced, last_gemm_kernel, tdt, view
from tests.helpers import npy

pytestmark = pytest.mark.gpu

A_MAX, C_MAX, K_MAX = 4, 64, 2100
ALPHAS = (1.0, -1.0, 2.0, 0.5)
BETAS = (0.0, 1.0, -2.0)
PAIRS = [(al, be) for al in ALPHAS for be in BETAS]
CKINDS = ("C", "T", "P")          # row-major, transposed (column-major), padded odd-ld column-major inside a sentinel border
SENTINEL = 777.0

# Both sides of every threshold the dispatch reads (kernels_gemm.hip unless noted):
#   M  32|33    launch_shape_f64q :585, launch_shape :627 (32-row panel tiles)
#      80|81    :581 / :590, :624 / :633
#      128|129  :594, :597 (128-row tiles, ring / direct-to-LDS) ; 136|137 :591, :610 ; 144|145 :581, :611, :624, :634, gemm() :690
#   N  31|32    launch_split :516 (k_splitk_reduce_t needs N >= 32)
#      80|81    :581, :582, :624, :625 ; 128|129 :583 ; 144|145 :581, :584, :624, :626, gemm() :690
#      255|256|257  :601 (direct-to-LDS B: N % 256 == 0), kernels_gemm_pipe.hip launch_r :518 (the sketch ring: N % 256 == 0)
#      2047|2048    :591 (shallow K over a wide N: 128-column tiles)
#   K  15|16|17  kernels_gemm_pipe.hip gemm_f64p_launch :564 (whole 16-deep K tiles), kernels_gemm.hip :601
#      160|161   :591 ; 511|512 :585, :627 ; 2100: 132 K tiles, enough for launch_split :498 to split a one-tile product
#   the transposed problem of f64, gemm() :690: b.cols <= 144 && a.rows > 144 -- M = 145 / 300 against N = 144 / 145
M_SET = (1, 32, 33, 80, 81, 128, 129, 136, 137, 144, 145, 300)
N_SET = (31, 32, 80, 81, 128, 129, 144, 145, 255, 256, 257, 2047, 2048)
K_SET = (1, 15, 16, 17, 160, 161, 511, 512, 2100)
K_SHALLOW, K_SPLIT = 48, 2096     # both whole K tiles, so the pipelined and ring loops take their shapes un-split and split

# Instantiations the dispatch names that these sizes cannot reach (not in GEMM_DISPATCH, not asserted):
#   k_gemm_f64q<1,0,128,256,16,1,8,2,1,2>  direct-to-LDS A and B (GLDS = 2): M-contiguous A of exactly 128 rows, N % 256 == 0,
#                                          K % 16 == 0 -- gemm_f64p_launch (called first, launch_f64q :572) gives that shape to
#                                          k_gemm_f64r<0,1,128,256,...> unless an operand span reaches 2 GiB (launch_r :519-521)
#   k_gemm_f64q<1,0,128,256,16,1,8,2,1,1>  direct-to-LDS B under an M-contiguous A (GLDS = 1, ALAY = 1): the same
#   k_gemm_f64p<1,0,128,256,16,1,8,1>      the projection on the pipelined loop: only where the ring refuses, i.e. spans >= 2 GiB
DTYPES = {"f64": np.float64, "f32": np.float32}
M_MASTER = max(max(M_SET), max(e[3] for e in GEMM_DISPATCH))
N_MASTER = max(max(N_SET), max(e[4] for e in GEMM_DISPATCH))

_HOST, _DEV, _SWEPT = {}, {}, {}
# instantiation -> set of (beta != 0, C kind, splits > 1) it ran with; which of the two slab reductions ran
LAUNCHED, REDUCTIONS = {}, set()


def _magnitude_precondition():
    """The bound of the module docstring; every sweep draws its data through _host(), which asserts it."""
    bound = max(abs(a) for a in ALPHAS) * A_MAX * A_MAX * K_MAX + max(abs(b) for b in BETAS) * C_MAX
    # every result is a multiple of the smallest |alpha| (1/2); multiples of 1/2 below 2^23 are f32 numbers
    assert min(abs(a) for a in ALPHAS) == 0.5 and all(float(2 * x).is_integer() for x in ALPHAS + BETAS)
    assert 2 * bound < 2 ** 24, bound
    assert max(K_SET + (K_SHALLOW, K_SPLIT) + tuple(e[5] for e in GEMM_DISPATCH)) <= K_MAX
    return bound


def test_magnitude_precondition_of_the_exact_data():
    assert _magnitude_precondition() == 2 * 16 * 2100 + 128
    h = _host()
    assert np.abs(h["a"]).max() <= A_MAX and np.abs(h["b"]).max() <= A_MAX and np.abs(h["c"]).max() <= C_MAX
    assert np.array_equal(h["a"], np.rint(h["a"])) and np.array_equal(h["b"], np.rint(h["b"])) and np.array_equal(h["c"], np.rint(h["c"]))


def _host():
    if not _HOST:
        _magnitude_precondition()
        rng = np.random.default_rng(2100)
        _HOST["a"] = rng.integers(-A_MAX, A_MAX + 1, (M_MASTER, K_MAX)).astype(np.float64)
        _HOST["b"] = rng.integers(-A_MAX, A_MAX + 1, (K_MAX, N_MASTER)).astype(np.float64)
        _HOST["c"] = rng.integers(-C_MAX, C_MAX + 1, (M_MASTER, N_MASTER)).astype(np.float64)
    return _HOST


def _product(m, n, k):
    """A[:m, :k] @ B[:k, :n] of the master integers in f64, on the device (computed once per K on the host, rows beyond
    max(M_SET) once per shape)."""
    rows = max(M_SET)
    key = ("p", k) if m <= rows else ("p", k, m, n)
    if key not in _DEV:
        h = _host()
        p = h["a"][:rows, :k] @ h["b"][:k, :] if m <= rows else h["a"][:m, :k] @ h["b"][:k, :n]
        _DEV[key] = torch.from_numpy(p).cuda()
    return _DEV[key][:m, :n]


def _c0(m, n):
    if "c" not in _DEV:
        _DEV["c"] = torch.from_numpy(_host()["c"]).cuda()
    return _DEV["c"][:m, :n]


def _strided(x, layout, vec, dt, fill, margin=0):
    """x (host f64) on the device as `dt`: "C" row-major / "F" column-major; vec = 2: even leading dimension and 16-byte aligned
    base (2-element vector staging, launch_vec kernels_gemm.hip:643-649), vec = 1: odd leading dimension (scalar staging, as
    gemm_operand(..., "c")).  The matrix sits `margin` rows and columns inside a buffer otherwise full of `fill`."""
    src = x if layout == "C" else x.T
    r, c = src.shape
    off = margin + (1 if vec == 1 and margin else 0)
    ld = c + 2 * margin + 2
    ld += (ld % 2) != (vec == 1)
    buf = torch.full((r + 2 * margin, ld), fill, dtype=dt, device="cuda")
    v = buf[margin:margin + r, off:off + c]
    v.copy_(torch.from_numpy(np.ascontiguousarray(src)).cuda())
    assert (v.stride(0) % 2 == 0 and v.data_ptr() % (2 * v.element_size()) == 0) == (vec == 2)
    return v if layout == "C" else v.t()


def _master(which, layout, vec, dt):
    key = (which, layout, vec, dt)
    if key not in _DEV:
        _DEV[key] = _strided(_host()[which], layout, vec, dt, 9.0)
    return _DEV[key]


def _c_buffer(dt, m, n, kind):
    if kind == "C":
        buf = torch.empty((m, n), dtype=dt, device="cuda")
        return buf, (lambda t: t)
    if kind == "T":
        buf = torch.empty((n, m), dtype=dt, device="cuda")
        return buf, (lambda t: t.t())
    ld = m + 3 if (m + 3) % 2 else m + 4
    buf = torch.full((n + 2, ld), SENTINEL, dtype=dt, device="cuda")
    return buf, (lambda t: t[1:n + 1, 2:m + 2].t())


def _exact(dt, av, bv, m, n, k, alpha, beta, ckind, tag, bad, record=True):
    """One product on exact data: C (and, for the padded kind, its sentinel border) must equal the reference bit for bit."""
    buf, inner = _c_buffer(dt, m, n, ckind)
    cv = inner(buf)
    ref = alpha * _product(m, n, k)
    if beta == 0:
        cv.fill_(float("nan"))
    else:
        cv.copy_(_c0(m, n))
        ref = ref + beta * _c0(m, n)
    want = buf.clone()
    inner(want).copy_(ref)
    name, (dm, dn), splits = gemm_traced(alpha, av, bv, beta, cv)
    if record:
        LAUNCHED.setdefault(name, set()).add((beta != 0, ckind, splits > 1))
        if splits > 1:
            # launch_split (kernels_gemm.hip:516): k_splitk_reduce_t when the dispatched C has scm < scn and N >= 32
            scm, scn = cv.stride() if (dm, dn) == (m, n) else cv.stride()[::-1]
            REDUCTIONS.add("k_splitk_reduce_t" if scm < scn and dn >= 32 else "k_splitk_reduce")
    if not torch.equal(buf, want):
        got, exp = npy(cv).astype(np.float64), npy(inner(want)).astype(np.float64)
        wrong = ~(got == exp)
        what = "%d entries differ, first at %s: %r for %r" % (int(wrong.sum()), tuple(np.argwhere(wrong)[0]), got[wrong][0], exp[wrong][0]) if wrong.any() else "border written"
        bad.append((tag, m, n, k, alpha, beta, ckind, name, splits, what))


def _pairs():
    i = 0
    while True:
        yield PAIRS[i % len(PAIRS)]
        i += 1


def _sweep(which, dt_name, la, lb):
    """The products of one (dtype, layout of A, layout of B): `mn` = M_SET x N_SET at the shallow and the splitting K, `k` = K_SET
    at the (M, N) of every arm.  Each over both staging widths and the three C kinds, alpha / beta cycling through all twelve
    pairs (seven steps per shape against twelve pairs: every pair meets every staging width and C kind).  Run once per session."""
    key = (which, dt_name, la, lb)
    if key in _SWEPT:
        return _SWEPT[key]
    dt = tdt(DTYPES[dt_name])
    if which == "mn":
        shapes = [(m, n, k) for k in (K_SHALLOW, K_SPLIT) for m in M_SET for n in N_SET]
    else:
        mn = sorted({(e[3], e[4]) for e in GEMM_DISPATCH if e[0] == dt_name})
        shapes = [(m, n, k) for (m, n) in mn for k in K_SET]
    bad, pairs = [], _pairs()
    for (m, n, k) in shapes:
        for vec in (2, 1):
            av = _master("a", la, vec, dt)[:m, :k]
            bv = _master("b", lb, vec, dt)[:k, :n]
            for ckind in CKINDS:
                alpha, beta = next(pairs)
                _exact(dt, av, bv, m, n, k, alpha, beta, ckind, (dt_name, la, lb, vec), bad)
        next(pairs)
    _SWEPT[key] = bad
    return bad


LAYOUTS = [(dt, la, lb) for dt in ("f64", "f32") for la in "CF" for lb in "CF"]


@pytest.mark.parametrize("dt_name,la,lb", LAYOUTS)
def test_exact_on_both_sides_of_every_m_and_n_threshold(dt_name, la, lb):
    bad = _sweep("mn", dt_name, la, lb)
    assert not bad, "%d products differ from the exact result:\n%s" % (len(bad), "\n".join(map(str, bad[:20])))


@pytest.mark.parametrize("dt_name,la,lb", LAYOUTS)
def test_exact_on_both_sides_of_every_k_threshold_per_arm(dt_name, la, lb):
    bad = _sweep("k", dt_name, la, lb)
    assert not bad, "%d products differ from the exact result:\n%s" % (len(bad), "\n".join(map(str, bad[:20])))


def test_the_sweeps_reach_every_arm_with_beta_padded_c_and_split_k():
    """Every instantiation of GEMM_DISPATCH ran in the two sweeps above (run here if they have not yet) with beta != 0, with the
    padded C and with K split (every arm can split at these sizes: a one-tile product splits from 8 K tiles on, and the shallow-K
    arms of kernels_gemm.hip:591 take two slabs at K = 160), and both slab reductions ran."""
    for dt_name, la, lb in LAYOUTS:
        _sweep("mn", dt_name, la, lb)
        _sweep("k", dt_name, la, lb)
    names = sorted({e[6] for e in GEMM_DISPATCH})
    missing = []
    for nm in names:
        ran = LAUNCHED.get(nm, set())
        if not any(b for (b, _, _) in ran):
            missing.append((nm, "never with beta != 0"))
        if not any(c == "P" for (_, c, _) in ran):
            missing.append((nm, "never with the padded C"))
        if not any(s for (_, _, s) in ran):
            missing.append((nm, "never with splits > 1"))
        if not any(b and c == "P" for (b, c, _) in ran):
            missing.append((nm, "never with beta != 0 on the padded C"))
    assert not missing, "\n".join(map(str, missing))
    assert REDUCTIONS == {"k_splitk_reduce", "k_splitk_reduce_t"}, REDUCTIONS
    print("instantiations launched by the sweeps: %d (%d of them in GEMM_DISPATCH)" % (len(LAUNCHED), len(names)))


# ------------------------------------------------------------------------------------------------ operands of no unit stride
@pytest.mark.parametrize("dt_name", ["f64", "f32"])
def test_exact_when_neither_stride_of_an_operand_is_one(dt_name):
    """A, then B, as a [::2, ::3] view: gemm() packs it (kernels_gemm.hip:675-686) before the dispatch."""
    dt = tdt(DTYPES[dt_name])
    h = _host()
    bad = []
    pairs = _pairs()
    for (m, n, k) in ((37, 41, 29), (133, 300, 64)):
        for which in ("a", "b"):
            x = h[which][:m, :k] if which == "a" else h[which][:k, :n]
            big = torch.full((2 * x.shape[0], 3 * x.shape[1]), 9.0, dtype=dt, device="cuda")
            sv = big[::2, ::3]
            sv.copy_(torch.from_numpy(np.ascontiguousarray(x)).cuda())
            assert 1 not in sv.stride()
            av = sv if which == "a" else _master("a", "C", 2, dt)[:m, :k]
            bv = sv if which == "b" else _master("b", "C", 2, dt)[:k, :n]
            for ckind in CKINDS:
                alpha, beta = next(pairs)
                _exact(dt, av, bv, m, n, k, alpha, beta, ckind, (dt_name, "strided " + which), bad, record=False)
    assert not bad, "\n".join(map(str, bad))


# ------------------------------------------------------------------------------------------------ masking of out-of-range elements
MARGIN = 258    # >= one tile row / column (256) on every side, even: every out-of-range address stays inside the allocation


@pytest.mark.parametrize("dt_name", ["f64", "f32"])
def test_out_of_range_operand_elements_are_masked_not_multiplied_by_zero(dt_name):
    """A and B are interior views of buffers full of NaN.  Every arm at its own shape and layout (the instantiation is asserted),
    then a ragged neighbour of that shape under every layout and both staging widths: a tile element beyond M, N or K that was
    loaded and multiplied by zero, instead of being masked by a select, makes the result NaN (TileStager, the direct-to-LDS
    copies, the ring's masked tail copy; rows the pipelined loops re-read by clamping lie inside the matrix)."""
    dt = tdt(DTYPES[dt_name])
    h = _host()
    bad, wrong_arm, pairs = [], [], _pairs()

    def run(m, n, k, la, lb, vec, want=None):
        av = _strided(h["a"][:m, :k], la, vec, dt, float("nan"), MARGIN)
        bv = _strided(h["b"][:k, :n], lb, vec, dt, float("nan"), MARGIN)
        alpha, beta = next(pairs)
        _exact(dt, av, bv, m, n, k, alpha, beta, "C", (dt_name, la, lb, vec, "NaN margins"), bad, record=False)
        if want is not None and last_gemm_kernel() != want:
            wrong_arm.append((m, n, k, la, lb, last_gemm_kernel(), want))

    for (d, la, lb, m, n, k, want) in GEMM_DISPATCH:
        if d != dt_name:
            continue
        run(m, n, k, la.upper(), lb, 1 if la == "c" else 2, want)
        mr, nr, kr = (m - 3 if m > 8 else m), n - 5, (k - 7 if k > 8 else k)
        for la2 in "CF":
            for lb2 in "CF":
                for vec in (2, 1):
                    run(mr, nr, kr, la2, lb2, vec)
    assert not wrong_arm, "\n".join(map(str, wrong_arm))
    assert not bad, "%d products differ from the exact result:\n%s" % (len(bad), "\n".join(map(str, bad[:20])))


# ------------------------------------------------------------------------------------------------ rounding data, per element
def test_rounding_error_of_every_arm_is_within_the_any_order_bound_per_element():
    """Gaussian data, alpha = 0.3, beta = 1.1, one case per arm (the instantiation is asserted).  For every entry
        |got - ref| <= (K + 4) eps (|alpha| |A| |B| + |beta| |C0|):
    a sum of K products in any order, slabs included, is within gamma_K = K u / (1 - K u) of its exact value relative to
    |A| |B|, u = eps / 2 (Higham, Accuracy and Stability of Numerical Algorithms, 3.1 / 3.5); K eps is that bound doubled, and
    4 eps covers the two roundings of the epilogue (alpha * v, + beta * c).  ref is the f64 result of the inputs as the kernel
    receives them (f32: the f32-rounded A, B, C0, alpha and beta)."""
    rng = np.random.default_rng(5)
    over, wrong_arm = [], []
    for (d, la, lb, m, n, k, want) in GEMM_DISPATCH:
        dtype = DTYPES[d]
        a = rng.standard_normal((m, k)).astype(dtype)
        b = rng.standard_normal((k, n)).astype(dtype)
        c0 = rng.standard_normal((m, n)).astype(dtype)
        alpha, beta = float(dtype(0.3)), float(dtype(1.1))
        a64, b64, c64 = a.astype(np.float64), b.astype(np.float64), c0.astype(np.float64)
        ref = alpha * (a64 @ b64) + beta * c64
        bound = (k + 4) * float(np.finfo(dtype).eps) * (abs(alpha) * (np.abs(a64) @ np.abs(b64)) + abs(beta) * np.abs(c64))
        cv, _ = view(c0, "C")
        gemm(0, 0, alpha, gemm_operand(a, la), gemm_operand(b, lb), beta, cv)
        if last_gemm_kernel() != want:
            wrong_arm.append((d, la, lb, m, n, k, last_gemm_kernel(), want))
        err = np.abs(npy(cv).astype(np.float64) - ref)
        worst = float((err / bound).max())
        print("%s %s%s %dx%dx%d %s: max |got - ref| / bound = %.3g" % (d, la, lb, m, n, k, want, worst))
        if not (err <= bound).all():
            over.append((d, la, lb, m, n, k, want, int((err > bound).sum()), worst))
    assert not wrong_arm, "\n".join(map(str, wrong_arm))
    assert not over, "\n".join(map(str, over))


# ------------------------------------------------------------------------------------------------ complex: the 4M composition
@pytest.mark.parametrize("dtype", [np.complex128, np.complex64])
def test_complex_products_on_every_arm_shape_are_exact(dtype):
    """rc_gemm_c64 / _c32 (four real products with alpha / beta = 1 / 0, -+1 / 1, s / 0, s / 1 on the planes, rc_complex.hip:206-209)
    at the shape of every real arm, op none / none and conjugate transpose / conjugate transpose, alpha = 1 - i, beta in {0, 1},
    padded C.  Gaussian integers from the halved ranges ([-2, 2], C0 [-32, 32]): each plane of op(A) op(B) is a sum of 2 K
    integers of magnitude <= 4, <= 8 * 1024; times 1 - i and plus C0 stays below 2^15, so c32 is exact as well."""
    rng = np.random.default_rng(6)
    shapes = sorted({(e[3], e[4], e[5]) for e in GEMM_DISPATCH})
    assert 2 * (2 * 2 * (A_MAX // 2) ** 2 * max(s[2] for s in shapes)) + 2 * (C_MAX // 2) < 2 ** 24

    def gint(shape, mx):
        return (rng.integers(-mx, mx + 1, shape) + 1j * rng.integers(-mx, mx + 1, shape)).astype(dtype)

    bad = []
    alpha = complex(1.0, -1.0)
    for i, (m, n, k) in enumerate(shapes):
        for op in (0, 2):
            a = gint((m, k) if op == 0 else (k, m), A_MAX // 2)
            b = gint((k, n) if op == 0 else (n, k), A_MAX // 2)
            c0 = gint((m, n), C_MAX // 2)
            a128, b128 = a.astype(np.complex128), b.astype(np.complex128)
            prod = a128 @ b128 if op == 0 else a128.conj().T @ b128.conj().T
            da, db = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
            for beta in (0.0, 1.0):
                want = alpha * prod + beta * c0.astype(np.complex128)
                start = np.full((m, n), complex(np.nan, np.nan), dtype=dtype) if beta == 0 else c0
                cv, buf = view(start, "P", fill=complex(SENTINEL, -SENTINEL))
                before = buf.clone()
                gemm(op, op, alpha, da, db, complex(beta), cv)
                got = npy(cv)
                inner = torch.zeros(buf.shape, dtype=torch.bool, device="cuda")
                inner[1:n + 1, 2:m + 2] = True
                border_kept = bool(torch.all((buf == before) | inner))
                if not (np.array_equal(got.astype(np.complex128), want) and border_kept):
                    bad.append((np.dtype(dtype).name, m, n, k, op, beta, last_gemm_kernel(), int((got != want).sum()), border_kept))
    assert not bad, "\n".join(map(str, bad))
