"""Every call of the C ABI that takes a caller's index array, against the host model of tests/permutation_ref.py (health bit 32).

How the tests are built.  The library is called through the C ABI on hand-made views.  Every operand, input or output, is a view
inside a larger allocation filled with a finite sentinel, GUARD spare rows and columns on both sides along both dimensions; index
arrays have spare elements in front and behind.  After every call the guard bands must still hold the sentinel and the inputs
their values.  "Near" bad entries are -1, n and n + 1: with GUARD >= 2 even a kernel without a check stays inside the test's own
allocation, so a missing check shows as a changed sentinel or a column that is not zero.  "Far" entries (-2^63, 2^40, 2^62) come last
in the file: run it with -x, so that they only reach kernels whose near cases passed.  The health word is drained before each call, must
be 32 exactly where the model rejects an entry, and reads 0 the second time."""
import ctypes

import numpy as np
import pytest
import torch

import rusty_compression_amd as rc
from rusty_compression_amd import _lib
from tests import permutation_ref as pr
from tests.helpers import TOL, npy

pytestmark = pytest.mark.gpu

GUARD = 3
BAD_INDEX = 32
DTYPES = [np.float64, np.float32, np.complex128, np.complex64]
REAL_DTYPES = [np.float64, np.float32]
LAYOUTS = ["row", "col"]
FAR = [-2 ** 63, 2 ** 40, 2 ** 62]
IDX_SENTINEL = 7777777
ID_K = (1, 15, 16, 17, 33, 128)
ID_SHAPES = sorted({(k, n) for k in ID_K for n in (k + 1, 255, 256, 257, 513) if k < n}) + [(12, 12)]
ID_SHAPES_COMPLEX = [(1, 2), (16, 257), (33, 513)]


def is_complex(dtype):
    return np.dtype(dtype).kind == "c"


def real_of(dtype):
    return np.zeros(0, dtype=dtype).real.dtype


def sentinel(dtype, which=0):
    v = (-7.25, 5.5)[which]
    return complex(v, 3.5) if is_complex(dtype) else v


def rand(rng, shape, dtype):
    x = rng.standard_normal(shape)
    if is_complex(dtype):
        x = x + 1j * rng.standard_normal(shape)
    return x.astype(dtype)


class Guarded:
    """A rows x cols operand as a view inside a sentinel-filled allocation, row-major or column-major (.t() of a contiguous tensor)."""

    def __init__(self, arr, layout="row", which=0):
        arr = np.asarray(arr)
        self.rows, self.cols = arr.shape
        self.layout, self.fill, self.want = layout, sentinel(arr.dtype, which), arr.copy()
        shape = (self.rows + 2 * GUARD, self.cols + 2 * GUARD)
        big = torch.full(shape if layout == "row" else shape[::-1], self.fill, dtype=torch.from_numpy(arr[:0]).dtype, device="cuda")
        self.big = big if layout == "row" else big.t()
        self.view = self.big[GUARD:GUARD + self.rows, GUARD:GUARD + self.cols]
        self.view.copy_(torch.from_numpy(np.ascontiguousarray(arr)).cuda())
        if self.rows > 1 and self.cols > 1:
            assert (self.view.stride(1) == 1) == (layout == "row") and (self.view.stride(0) == 1) == (layout == "col")

    @classmethod
    def output(cls, rows, cols, dtype, layout="row"):
        """An output operand: the view itself starts at a second finite sentinel, so a column the call leaves alone shows."""
        return cls(np.full((rows, cols), sentinel(dtype, 1), dtype=dtype), layout)

    def mat(self):
        return _lib.mat(self.view)

    def get(self):
        return npy(self.view)

    def guards_intact(self):
        b = npy(self.big)
        mask = np.ones(b.shape, dtype=bool)
        mask[GUARD:GUARD + self.rows, GUARD:GUARD + self.cols] = False
        return bool((b[mask] == self.fill).all())

    def unchanged(self):
        return self.guards_intact() and np.array_equal(self.get(), self.want)


class GuardedIndex:
    """An int64 device array with `lead` spare elements in front and GUARD behind."""

    def __init__(self, values, lead=GUARD, fill=IDX_SENTINEL):
        self.want = np.asarray(values, dtype=np.int64).copy()
        self.n, self.lead, self.fill = len(self.want), lead, fill
        self.big = torch.full((self.n + lead + GUARD,), fill, dtype=torch.int64, device="cuda")
        self.view = self.big[lead:lead + self.n]
        self.view.copy_(torch.from_numpy(self.want).cuda())

    def ptr(self):
        return ctypes.c_void_p(self.view.data_ptr())

    def get(self):
        return npy(self.view)

    def guards_intact(self):
        b = npy(self.big)
        return bool((b[:self.lead] == self.fill).all() and (b[self.lead + self.n:] == self.fill).all())

    def unchanged(self):
        return self.guards_intact() and np.array_equal(self.get(), self.want)


def call(name, *args):
    """One call of the C ABI with the health word drained before and read twice after: returns the first read."""
    ctx = _lib.default_context()
    ctx.get_health()
    ctx.call(name, *args)
    torch.cuda.synchronize()
    health = ctx.get_health()
    assert ctx.get_health() == 0  # read and cleared
    return health


def near_bad_inputs(rng, n):
    """[(label, perm)]: a random valid permutation with one of -1, n, n + 1 in the first, a middle and the last position."""
    out = []
    for pos in sorted({0, n // 2, n - 1}):
        for bad in (-1, n, n + 1):
            perm = rng.permutation(n).astype(np.int64)
            perm[pos] = bad
            out.append((f"{bad - n if bad > 0 else bad:+d}@{pos}", perm))
    return out


def duplicate_input(rng, n):
    perm = rng.permutation(n).astype(np.int64)
    a, b = rng.choice(n, 2, replace=False)
    perm[a] = perm[b]
    return perm


def suffix(dtype):
    return {"float64": "f64", "float32": "f32", "complex128": "c64", "complex64": "c32"}[np.dtype(dtype).name]


# ------------------------------------------------------------------------------------------------------------ 1. gathers
@pytest.mark.parametrize("out_layout", LAYOUTS)
@pytest.mark.parametrize("in_layout", LAYOUTS)
@pytest.mark.parametrize("mode", pr.MODES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_apply_permutation_matrix(dtype, mode, in_layout, out_layout):
    m, n = 37, 53
    rng = np.random.default_rng(101)
    a = rand(rng, (m, n), dtype)
    plen = n if mode.startswith("COL") else m
    inputs = [("valid", rng.permutation(plen).astype(np.int64)), ("duplicate", duplicate_input(rng, plen))] + near_bad_inputs(rng, plen)
    for label, perm in inputs:
        src, dst, idx = Guarded(a, in_layout), Guarded.output(m, n, dtype, out_layout), GuardedIndex(perm)
        health = call(f"rc_apply_permutation_matrix_{suffix(dtype)}", ctypes.c_int32(pr.MODES.index(mode)), src.mat(), idx.ptr(), ctypes.c_int64(plen), dst.mat())
        choices, rejected = pr.apply_matrix(a, perm, mode)
        # a duplicate is legal without the inverse (the column is repeated); with it a destination is unnamed
        assert rejected == (label != "valid" and (label != "duplicate" or mode.endswith("INV"))), label
        got = dst.get() if mode.startswith("COL") else dst.get().T
        assert pr.admissible(got, choices).all(), label  # exact: no arithmetic happens
        assert health == (BAD_INDEX if rejected else 0), label
        assert dst.guards_intact() and src.unchanged() and idx.unchanged(), label


@pytest.mark.parametrize("out_layout", LAYOUTS)
@pytest.mark.parametrize("in_layout", LAYOUTS)
@pytest.mark.parametrize("mode", pr.VMODES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_apply_permutation_vector(dtype, mode, in_layout, out_layout):
    n = 53
    rng = np.random.default_rng(102)
    v = rand(rng, (n, 1), dtype)
    inputs = [("valid", rng.permutation(n).astype(np.int64)), ("duplicate", duplicate_input(rng, n))] + near_bad_inputs(rng, n)
    for label, perm in inputs:
        src, dst, idx = Guarded(v, in_layout), Guarded.output(n, 1, dtype, out_layout), GuardedIndex(perm)
        health = call(f"rc_apply_permutation_vector_{suffix(dtype)}", ctypes.c_int32(pr.VMODES.index(mode)), src.mat(), idx.ptr(), ctypes.c_int64(n), dst.mat())
        choices, rejected = pr.apply_vector(v[:, 0], perm, mode)
        assert rejected == (label != "valid" and (label != "duplicate" or mode == "INV")), label
        assert pr.admissible(dst.get().T, choices).all(), label
        assert health == (BAD_INDEX if rejected else 0), label
        assert dst.guards_intact() and src.unchanged() and idx.unchanged(), label


# ------------------------------------------------------------------------------------------------------------ 2. grid-stride loops
def test_gather_beyond_the_grid_cap():
    """k_gather_cols launches at most 8192 x 256 threads: 1449 x 1449 = 2 099 601 elements take a second trip of the loop."""
    n = 1449
    assert n * n > 8192 * 256 > (n - 1) * (n - 1)
    rng = np.random.default_rng(103)
    a = rng.standard_normal((n, n)).astype(np.float32)
    perm = rng.permutation(n).astype(np.int64)
    perm[-1] = n
    src, dst, idx = Guarded(a), Guarded.output(n, n, np.float32), GuardedIndex(perm)
    health = call("rc_apply_permutation_matrix_f32", ctypes.c_int32(pr.MODES.index("COL")), src.mat(), idx.ptr(), ctypes.c_int64(n), dst.mat())
    want, rejected = pr.checked_gather(a, perm)
    assert rejected and health == BAD_INDEX
    assert np.array_equal(dst.get(), want)
    assert dst.guards_intact() and src.unchanged() and idx.unchanged()


def test_invert_permutation_beyond_the_grid_cap():
    """k_invert_perm launches at most 4096 x 256 threads: n = 1 048 579 takes a second trip of the loop (and k_fill_words its tail)."""
    n = 1048579
    assert n > 4096 * 256
    rng = np.random.default_rng(104)
    perm = rng.permutation(n).astype(np.int64)
    perm[-1] = n + 1
    idx, inv = GuardedIndex(perm), GuardedIndex(np.full(n, 5, dtype=np.int64), fill=-IDX_SENTINEL)
    health = call("rc_invert_permutation", idx.ptr(), ctypes.c_int64(n), inv.ptr())
    assert np.array_equal(inv.get(), pr.checked_invert_unique(perm, n))
    assert health == 0  # the call raises no bit itself: the gather that consumes the -1 does
    assert inv.guards_intact() and idx.unchanged()


# ------------------------------------------------------------------------------------------------------------ 3. rc_invert_permutation
@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "offset"])
@pytest.mark.parametrize("n", [1, 2, 3, 1025])
def test_invert_permutation(n, offset):
    """k_fill_words writes uint4 where `inverse` is 16-byte aligned (an odd n leaves a tail of two words) and words where it is not."""
    rng = np.random.default_rng(105 + n)
    inputs = [("valid", rng.permutation(n).astype(np.int64))] + near_bad_inputs(rng, n)
    if n >= 2:
        inputs.append(("duplicate", duplicate_input(rng, n)))
    for label, perm in inputs:
        idx = GuardedIndex(perm)
        inv = GuardedIndex(np.full(n, 5, dtype=np.int64), lead=2 + offset, fill=-IDX_SENTINEL)
        assert inv.view.data_ptr() % 16 == 8 * offset
        health = call("rc_invert_permutation", idx.ptr(), ctypes.c_int64(n), inv.ptr())
        adm = pr.checked_invert(perm, n)
        assert pr.inverse_admissible(inv.get(), adm).all(), (label, inv.get(), adm)
        assert health == 0, label
        assert inv.guards_intact() and idx.unchanged(), label


# ------------------------------------------------------------------------------------------------------------ 4. to_mat
def check_columns(got, src64, adm, tol):
    """Column j of `got` is exactly zero where adm[j] is empty; the others agree with one admissible column of src64 each, to `tol`
    in the relative Frobenius norm over all of them."""
    want = np.zeros(src64.shape, dtype=src64.dtype)
    for j, v in enumerate(adm):
        if not v:
            assert not got[:, j].any(), j
        else:
            want[:, j] = min((src64[:, p] for p in v), key=lambda c: np.linalg.norm(got[:, j] - c))
    assert np.linalg.norm(got - want) <= tol * np.linalg.norm(want)


def to_mat_inputs(rng, n):
    near = near_bad_inputs(rng, n)
    return [("valid", rng.permutation(n).astype(np.int64)), ("duplicate", duplicate_input(rng, n)), near[0], near[4], near[8]]


@pytest.mark.parametrize("dtype", DTYPES)
def test_qr_to_mat(dtype):
    m, k, n = 40, 12, 30
    rng = np.random.default_rng(106)
    q, r = rand(rng, (m, k), dtype), rand(rng, (k, n), dtype)
    full = q.astype(np.complex128 if is_complex(dtype) else np.float64) @ r
    for label, ind in to_mat_inputs(rng, n):
        gq, gr, out, idx = Guarded(q), Guarded(r), Guarded.output(m, n, dtype), GuardedIndex(ind)
        health = call(f"rc_qr_to_mat_{suffix(dtype)}", gq.mat(), gr.mat(), idx.ptr(), out.mat())
        adm = pr.checked_invert(ind, n)
        check_columns(out.get(), full, adm, TOL[real_of(dtype)]["factor"])  # out = Q colinv(R)
        assert health == (0 if label == "valid" else BAD_INDEX), label
        assert out.guards_intact() and gq.unchanged() and gr.unchanged() and idx.unchanged(), label


@pytest.mark.parametrize("dtype", DTYPES)
def test_lq_to_mat(dtype):
    m, k, n = 30, 12, 40
    rng = np.random.default_rng(107)
    l, q = rand(rng, (m, k), dtype), rand(rng, (k, n), dtype)
    full = l.astype(np.complex128 if is_complex(dtype) else np.float64) @ q
    for label, ind in to_mat_inputs(rng, m):
        gl, gq, out, idx = Guarded(l), Guarded(q), Guarded.output(m, n, dtype), GuardedIndex(ind)
        health = call(f"rc_lq_to_mat_{suffix(dtype)}", gl.mat(), gq.mat(), idx.ptr(), out.mat())
        adm = pr.checked_invert(ind, m)
        check_columns(out.get().T, full.T, adm, TOL[real_of(dtype)]["factor"])  # out = rowinv(L) Q: the same statement about rows
        assert health == (0 if label == "valid" else BAD_INDEX), label
        assert out.guards_intact() and gl.unchanged() and gq.unchanged() and idx.unchanged(), label


# ------------------------------------------------------------------------------------------------------------ 5. column and row ID
def run_id(kind, dtype, q, r, ind, r_layout="row", z_layout="row"):
    """rc_qr_column_id_* on (q, r, ind) or rc_lq_row_id_* on (l, q', ind) = (r^H, q^H, ind), whose outputs are the adjoints of the
    column ID's.  Returns (C, Z, health) in the column ID's orientation after checking guards and inputs."""
    m, k = q.shape
    n = r.shape[1]
    idx = GuardedIndex(ind)
    if kind == "qr":
        gq, gr = Guarded(q), Guarded(r, r_layout)
        c, z = Guarded.output(m, k, dtype), Guarded.output(k, n, dtype, z_layout)
        health = call(f"rc_qr_column_id_{suffix(dtype)}", gq.mat(), gr.mat(), idx.ptr(), c.mat(), z.mat())
        cm, zm = c.get(), z.get()
    else:
        gq, gr = Guarded(np.conj(q.T)), Guarded(np.conj(r.T), r_layout)
        c, z = Guarded.output(k, m, dtype), Guarded.output(n, k, dtype, z_layout)
        health = call(f"rc_lq_row_id_{suffix(dtype)}", gr.mat(), gq.mat(), idx.ptr(), z.mat(), c.mat())
        cm, zm = np.conj(c.get().T), np.conj(z.get().T)
    assert c.guards_intact() and z.guards_intact() and gq.unchanged() and gr.unchanged() and idx.unchanged()
    return cm, zm, health


def trsm_reference(dtype, r, k, layout):
    """The public rc_trsm_upper_* applied to R11 and a copy of R12 (real dtypes)."""
    t, b = Guarded(r[:, :k], layout), Guarded(r[:, k:].copy())
    assert call(f"rc_trsm_upper_{suffix(dtype)}", t.mat(), b.mat()) == 0
    assert t.unchanged() and b.guards_intact()
    return b.get()


def id_bad_inputs(rng, ind, k, n, variant):
    """(near, dup): `ind` with one near bad entry at a position >= k and one at a position < k (the values rotate with `variant`), and
    `ind` with a duplicate between a position < k and one >= k (variant even: the identity column's entry is the copy)."""
    lo, hi = [(-1, n), (n, n + 1), (n + 1, -1), (-1, n + 1)][variant % 4]
    near = ind.copy()
    near[int(rng.integers(0, k))] = lo
    if k < n:
        near[int(rng.integers(k, n))] = hi
    dup = ind.copy()
    a, b = (int(rng.integers(0, k)), int(rng.integers(k, n))) if k < n else tuple(int(v) for v in rng.choice(n, 2, replace=False))
    if variant % 2:
        a, b = b, a
    dup[a] = dup[b]
    return near, dup


def check_id_shape(kind, dtype, k, n):
    m = 24
    rng = np.random.default_rng(1000 * k + n)
    q, r = pr.id_factors(rng, m, k, n, dtype)
    wide = np.complex128 if is_complex(dtype) else np.float64
    c_want = q.astype(wide) @ r[:, :k].astype(wide)
    tol = TOL[real_of(dtype)]["factor"]
    worst = 0.0
    for variant, (r_layout, z_layout) in enumerate([(a, b) for a in LAYOUTS for b in LAYOUTS]):
        ind = rng.permutation(n).astype(np.int64)
        c_valid, z_valid, health = run_id(kind, dtype, q, r, ind, r_layout, z_layout)
        assert health == 0
        # 1. the identity, and (real dtypes) the bits of k_trsm_upper at every tile and workgroup edge
        assert np.array_equal(z_valid[:, ind[:k]], np.eye(k, dtype=dtype))
        if k < n and not is_complex(dtype):
            assert np.array_equal(z_valid[:, ind[k:]], trsm_reference(dtype, r, k, r_layout))
        # 2. the backward error of the solve.  Back substitution with k terms per row satisfies |R11 Z12 - R12| <= gamma_k |R11| |Z12|
        # componentwise (Higham, Theorem 8.5), and so in the Frobenius norm.  The tile-blocked order adds at most one more accumulation
        # per tile row over Higham's bound, which is the reason for the factor 2.  (rho_factor() is 3 only where np.longdouble is not
        # x86 extended and the evaluation of rho is itself no more accurate than the data.)
        if k < n:
            rho = pr.backward_error(r[:, :k], z_valid[:, ind[k:]], r[:, k:], pr.wide_type(dtype))
            ratio = rho / pr.gamma(k, dtype)
            worst = max(worst, ratio)
            print(f"RHO {np.dtype(dtype).name} {kind} k={k} n={n} r={r_layout} z={z_layout} rho={rho:.3e} rho/gamma_k={ratio:.4f}")
            assert ratio <= pr.rho_factor(), (rho, pr.gamma(k, dtype))
        # 3. C = Q R11
        assert np.linalg.norm(c_valid - c_want) <= tol * np.linalg.norm(c_want)
        # 4. an ind that is no permutation
        for bad in id_bad_inputs(rng, ind, k, n, variant):
            c_bad, z_bad, health = run_id(kind, dtype, q, r, bad, r_layout, z_layout)
            assert np.array_equal(c_bad, c_valid)  # C does not depend on ind
            adm = pr.checked_invert(bad, n)
            assert any(not v for v in adm)
            choices = [[z_valid[:, ind[p]] for p in v] if v else [np.zeros(k, dtype=dtype)] for v in adm]
            assert pr.admissible(z_bad, choices).all(), (bad, np.nonzero(~pr.admissible(z_bad, choices))[0])
            assert health == BAD_INDEX
    return worst


@pytest.mark.parametrize("shape", ID_SHAPES, ids=lambda s: f"k{s[0]}n{s[1]}")
@pytest.mark.parametrize("dtype", REAL_DTYPES)
@pytest.mark.parametrize("kind", ["qr", "lq"])
def test_id_real(kind, dtype, shape):
    check_id_shape(kind, dtype, *shape)


@pytest.mark.parametrize("shape", ID_SHAPES_COMPLEX, ids=lambda s: f"k{s[0]}n{s[1]}")
@pytest.mark.parametrize("dtype", [np.complex128, np.complex64])
@pytest.mark.parametrize("kind", ["qr", "lq"])
def test_id_complex(kind, dtype, shape):
    check_id_shape(kind, dtype, *shape)


# ------------------------------------------------------------------------------------------------------------ 6. the Python surface
def test_qr_and_lq_objects_with_a_bad_ind():
    """The call a user makes: the constructors accept any index tensor."""
    m, k, n = 24, 5, 9
    rng = np.random.default_rng(108)
    q, r = pr.id_factors(rng, m, k, n, np.float64)
    ind = rng.permutation(n).astype(np.int64)
    missing, ind[6] = int(ind[6]), n
    ctx = _lib.default_context()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    ctx.get_health()
    cid = rc.QR(dev(q), dev(r), dev(ind)).column_id()
    torch.cuda.synchronize()
    assert ctx.get_health() == BAD_INDEX and ctx.get_health() == 0
    z = npy(cid.z)
    assert not z[:, missing].any() and all(z[:, j].any() for j in range(n) if j != missing)
    rid = rc.LQ(dev(r.T), dev(q.T), dev(ind)).row_id()
    torch.cuda.synchronize()
    assert ctx.get_health() == BAD_INDEX and ctx.get_health() == 0
    x = npy(rid.x)
    assert not x[missing].any() and all(x[j].any() for j in range(n) if j != missing)
    assert np.array_equal(x, z.T)


# ------------------------------------------------------------------------------------------------------------ 7. far indices (last)
def far_inputs(rng, n):
    """Permutations with the far values in the first, a middle and the last position, one value at a time and all three at once."""
    out = []
    for i, bad in enumerate(FAR):
        perm = rng.permutation(n).astype(np.int64)
        perm[sorted({0, n // 2, n - 1})[i % len({0, n // 2, n - 1})]] = bad
        out.append(perm)
    perm = rng.permutation(n).astype(np.int64)
    for pos, bad in zip(sorted({0, n // 2, n - 1}), FAR):
        perm[pos] = bad
    return out + [perm]


@pytest.mark.parametrize("mode", pr.MODES)
def test_far_indices_apply_permutation_matrix(mode):
    m, n = 37, 53
    rng = np.random.default_rng(109)
    a = rand(rng, (m, n), np.float64)
    plen = n if mode.startswith("COL") else m
    for perm in far_inputs(rng, plen):
        src, dst, idx = Guarded(a), Guarded.output(m, n, np.float64), GuardedIndex(perm)
        health = call("rc_apply_permutation_matrix_f64", ctypes.c_int32(pr.MODES.index(mode)), src.mat(), idx.ptr(), ctypes.c_int64(plen), dst.mat())
        want, rejected = pr.apply_matrix_unique(a, perm, mode)
        assert rejected and health == BAD_INDEX
        assert np.array_equal(dst.get(), want)
        assert dst.guards_intact() and src.unchanged() and idx.unchanged()


@pytest.mark.parametrize("mode", pr.VMODES)
def test_far_indices_apply_permutation_vector(mode):
    n = 53
    rng = np.random.default_rng(110)
    v = rand(rng, (n, 1), np.float64)
    for perm in far_inputs(rng, n):
        src, dst, idx = Guarded(v), Guarded.output(n, 1, np.float64), GuardedIndex(perm)
        health = call("rc_apply_permutation_vector_f64", ctypes.c_int32(pr.VMODES.index(mode)), src.mat(), idx.ptr(), ctypes.c_int64(n), dst.mat())
        choices, rejected = pr.apply_vector(v[:, 0], perm, mode)
        assert rejected and health == BAD_INDEX
        assert pr.admissible(dst.get().T, choices).all()
        assert dst.guards_intact() and src.unchanged() and idx.unchanged()


def test_far_indices_invert_permutation():
    for n in (1, 3):
        rng = np.random.default_rng(111)
        for perm in far_inputs(rng, n):
            idx, inv = GuardedIndex(perm), GuardedIndex(np.full(n, 5, dtype=np.int64), lead=2, fill=-IDX_SENTINEL)
            health = call("rc_invert_permutation", idx.ptr(), ctypes.c_int64(n), inv.ptr())
            assert pr.inverse_admissible(inv.get(), pr.checked_invert(perm, n)).all()
            assert health == 0 and inv.guards_intact() and idx.unchanged()


def test_far_indices_to_mat():
    m, k, n = 40, 12, 30
    rng = np.random.default_rng(112)
    q, r = rand(rng, (m, k), np.float64), rand(rng, (k, n), np.float64)
    for ind in far_inputs(rng, n):
        adm = pr.checked_invert(ind, n)
        gq, gr, out, idx = Guarded(q), Guarded(r), Guarded.output(m, n, np.float64), GuardedIndex(ind)
        assert call("rc_qr_to_mat_f64", gq.mat(), gr.mat(), idx.ptr(), out.mat()) == BAD_INDEX
        check_columns(out.get(), q @ r, adm, TOL[np.dtype(np.float64)]["factor"])
        assert out.guards_intact() and gq.unchanged() and gr.unchanged() and idx.unchanged()
        gl, gq, out, idx = Guarded(r.T), Guarded(q.T), Guarded.output(n, m, np.float64), GuardedIndex(ind)
        assert call("rc_lq_to_mat_f64", gl.mat(), gq.mat(), idx.ptr(), out.mat()) == BAD_INDEX
        check_columns(out.get().T, q @ r, adm, TOL[np.dtype(np.float64)]["factor"])
        assert out.guards_intact() and gl.unchanged() and gq.unchanged() and idx.unchanged()


@pytest.mark.parametrize("kind", ["qr", "lq"])
def test_far_indices_id(kind):
    k, n = 1, 2
    rng = np.random.default_rng(113)
    q, r = pr.id_factors(rng, 24, k, n, np.float64)
    ind = np.array([1, 0], dtype=np.int64)
    c_valid, z_valid, health = run_id(kind, np.float64, q, r, ind)
    assert health == 0
    for bad in ([FAR[0], 0], [1, FAR[1]], [FAR[2], FAR[0]], [FAR[1], FAR[2]]):
        bad = np.array(bad, dtype=np.int64)
        c_bad, z_bad, health = run_id(kind, np.float64, q, r, bad)
        adm = pr.checked_invert(bad, n)
        choices = [[z_valid[:, ind[p]] for p in v] if v else [np.zeros(k)] for v in adm]
        assert pr.admissible(z_bad, choices).all() and np.array_equal(c_bad, c_valid)
        assert health == BAD_INDEX
