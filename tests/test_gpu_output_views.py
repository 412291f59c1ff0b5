"""Every dense entry point of the C ABI that writes a matrix, with caller-allocated output VIEWS of every layout the header promises
to accept (include/rusty_compression_amd.h, "Conventions"), on every dispatch branch that treats an output differently.

The Python package allocates every dense output with types.empty(): fresh, C order, unpadded, 256-byte aligned.  Here the outputs
are the views of tests/view_layouts.py -- C (that baseline), F, FP (column-major, odd pitch, odd element offset, guard band), CP (its
row-major twin), S (both strides non-unit) -- inside allocations filled with a quiet-NaN sentinel, passed through the C ABI the way
tests/test_gpu_index_contract.py passes its views.  One test is one (entry point, scalar type, shape); it loops over the layouts
(all outputs of a call in the same layout) and adds one call whose outputs take different layouts ("mixed").  Per call:

  1. status RC_OK, health word 0 afterwards, every input bit-identical to before;
  2. every element outside an output view still holds the sentinel bits (guard band, gaps of S; for the in-place calls: nothing
     outside the view changed), and no element inside was left unwritten;
  3. integer outputs (ind, ranks, histories) and vectors (singular values, tau) are identical to the C baseline;
  4. matrix outputs are bit-identical to the C baseline, except the (entry point, output, type) triples of ROUNDING_ONLY.

Which branch a shape reaches is asserted from the library's own profile labels, not assumed.

Real family, dispatch predicates (rc_api.hip qrcp_core / lapack_geqp3 / column_id_rank; m x n is the matrix the pivoted QR sees):
  tall-skinny fast path  tsqr_supported (kernels_tsqr.hip:221): n >= 2, m >= 4 n, m >= 1024              1031 x 9
  cooperative short-wide wide_coop_supported (kernels_wqcoop.hip:670): 2 <= m <= 256, n >= max(4 m, 256)   5 x 259
  lazy short-wide        wide_lazy_supported (kernels_qr.hip:1022): same domain, RC_OPT_WIDE_COOP_QRCP = 0 5 x 259
  blocked panels         geqp3_blocked_supported (kernels_qrblk.hip:1391): m, n >= 128, k >= 8             131 x 137, k = 131 and 9
  per-step chain         everything else                                                                   37 x 23, 23 x 37
Q is formed in the caller's buffer when q.rs == 1 && q.cs >= q.rows (rc_api.hip qrcp_core, three places; lapack_orgqr), handed to
qrcp_tall_fast / geqp3_wide_lazy / geqp3_blocked as it is, and goes through a column-major temporary and copy_mat otherwise; form_q
itself splits at m <= 128 (k_form_q_small), m <= 512, m <= 2048 (k_form_q<2>, <8>).  1 x 7, 7 x 1 and 1 x 1 are the shapes where
the strides of a size-1 dimension make that predicate ambiguous.  compute_svd switches at tsqr_supported(M, r) of the tall
orientation: 1031 x 9 / 9 x 1031 against 1023 x 9 / 9 x 1023.

Complex family (rc_complex.hip): ONE pivoted-QR path (c_geqp3, the per-step chain: no tall-skinny, short-wide or blocked branch
exists for c64 / c32), every output written into a column-major temporary and copied (c_copy) or combined (k_c_combine) into the
caller's view.  The only output-relevant switch is c_compute_svd's qr_first (max(m, n) >= 2 min(m, n) and min(m, n) >= 2): 37 x 23
against 61 x 23, and their transposes.  So the complex list is the chain shapes, that switch and the degenerate shapes.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from oracle import ref_lapack as o
from rusty_compression_amd import _lib
from tests import view_layouts as vl
from tests.helpers import TOL, npy

pytestmark = pytest.mark.gpu

NP = {"f64": np.float64, "f32": np.float32, "c64": np.complex128, "c32": np.complex64}
REAL = {"f64": np.float64, "f32": np.float32, "c64": np.float64, "c32": np.float32}
ALL, REALS, CPLX = ("f64", "f32", "c64", "c32"), ("f64", "f32"), ("c64", "c32")
MIXED = ("FP", "S", "CP", "F", "C")
ASSIGNMENTS = [(name, (lambda i, name=name: name)) for name in vl.LAYOUTS] + [("mixed", lambda i: MIXED[i % len(MIXED)])]
IDX_SENTINEL = 7777777

# (entry point, output, scalar type) -> "file:line" of the layout-dispatched product the output is the C operand of, or whose
# operand layout it inherits.  A triple may be listed only after the mismatch has been traced to that product in the code; the
# listed outputs are checked against the same product in f64 / c128 on the host instead (rounding_check below).
ROUNDING_ONLY = {}


# ------------------------------------------------------------------------------------------------------------ inputs
@functools.lru_cache(maxsize=None)
def matrix(sfx, m, n, seed=1, smin=None):
    """Oracle's random_approximate_low_rank_matrix with a spectrum wide enough that the working precision decides the pivots
    (tests/test_gpu_lapack.py::_mat)."""
    if smin is None:
        smin = 1e-3 if REAL[sfx] == np.float32 else 1e-6
    a = o.random_approximate_low_rank_matrix((m, n), 1.0, smin, np.random.default_rng(1000 * seed + 7 * m + n), NP[sfx])
    a.setflags(write=False)
    return a


def gaussian(sfx, rows, cols, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((rows, cols))
    if sfx in CPLX:
        x = x + 1j * rng.standard_normal((rows, cols))
    return x.astype(NP[sfx])


@functools.lru_cache(maxsize=None)
def qr_factors(sfx, m, n, k, smin=None):
    q, r, ind = o.pivoted_qr(matrix(sfx, m, n, 2, smin))
    return np.ascontiguousarray(q[:, :k]).astype(NP[sfx]), np.ascontiguousarray(r[:k]).astype(NP[sfx]), np.asarray(ind, dtype=np.int64)


@functools.lru_cache(maxsize=None)
def svd_factors(sfx, m, n, k):
    u, s, vt = o.compute_svd(matrix(sfx, m, n, 3))
    return np.ascontiguousarray(u[:, :k]).astype(NP[sfx]), s[:k].astype(REAL[sfx]), np.ascontiguousarray(vt[:k]).astype(NP[sfx])


@functools.lru_cache(maxsize=None)
def range_of(sfx, m, n, rr, smin=None):
    a = matrix(sfx, m, n, 4, smin)
    wide = np.complex128 if sfx in CPLX else np.float64
    q, _ = np.linalg.qr(a.astype(wide) @ gaussian(sfx, n, rr, 5).astype(wide))
    return a, np.ascontiguousarray(q[:, :rr]).astype(NP[sfx])


# ------------------------------------------------------------------------------------------------------------ one call
def profile_labels(fn):
    ctx, lib = _lib.default_context(), _lib.lib()
    names = []
    ctx.check(lib.rc_profile_enable(ctx._h, 1))
    try:
        ctx.check(lib.rc_profile_reset(ctx._h))
        fn()
        cnt = ctypes.c_int32(0)
        ctx.check(lib.rc_profile_count(ctx._h, ctypes.byref(cnt)))
        for i in range(cnt.value):
            name = ctypes.create_string_buffer(192)
            ms, calls = ctypes.c_double(0), ctypes.c_int64(0)
            ctx.check(lib.rc_profile_get(ctx._h, i, name, 192, ctypes.byref(ms), ctypes.byref(calls)))
            names.append(name.value.decode())
    finally:
        lib.rc_profile_enable(ctx._h, 0)
        lib.rc_profile_reset(ctx._h)
    return names


class Call:
    """The operands of one call of the C ABI: inputs (kept to compare afterwards), output views in the layouts `assign` names,
    guarded integer and real vectors, host scalars."""

    def __init__(self, sfx, assign):
        self.sfx, self.assign = sfx, assign
        self.ins, self.outs, self.vecs, self.extras, self.labels = [], [], [], {}, []

    def inp(self, name, arr):
        t = torch.from_numpy(np.array(arr, order="C", copy=True)).cuda()
        self.ins.append((name, t, vl.bits(t)))
        return t

    def mat(self, name, arr):
        return _lib.mat(self.inp(name, arr))

    def ptr(self, name, arr):
        return ctypes.c_void_p(self.inp(name, arr).data_ptr())

    def out(self, name, rows, cols, init=None):
        """An output view (sentinel-filled; `init`: the in-place operand's input values)."""
        layout = self.assign(len(self.outs))
        view, buffer, inside = vl.make_view(rows, cols, NP[self.sfx], layout, "cuda")
        if init is not None:
            view.copy_(torch.from_numpy(np.array(init, order="C", copy=True)).cuda())
        self.outs.append(dict(name=name, view=view, buffer=buffer, inside=inside, layout=layout, cols_written=cols))
        return _lib.mat(view)

    def vec(self, name, n, dtype):
        """A device vector of n entries (int64: index sentinel; else the NaN sentinel) with GUARD spare entries on both sides."""
        g = vl.GUARD
        if np.dtype(dtype) == np.int64:
            big = torch.full((n + 2 * g,), IDX_SENTINEL, dtype=torch.int64, device="cuda")
        else:
            big = vl.sentinel_buffer(n + 2 * g, dtype, "cuda")
        self.vecs.append((name, big, n))
        return ctypes.c_void_p(big[g:g + n].data_ptr() if n else big[g:].data_ptr())

    def call(self, entry, *args, expect=None, forbid=()):
        """rc_<entry>_<sfx>(ctx, *args): health drained before and 0 after.  A HIP runtime error ends the session: nothing more is
        started on a device that has reported one."""
        ctx = _lib.default_context()
        ctx.get_health()

        def go():
            try:
                ctx.call(f"rc_{entry}_{self.sfx}", *args)
                torch.cuda.synchronize()
            except (_lib.HipRuntimeError, RuntimeError) as e:
                pytest.exit(f"rc_{entry}_{self.sfx}: the device reported {e!r}; no further call is made on it", returncode=3)

        if expect is None:
            go()
        else:
            self.labels = profile_labels(go)
            assert any(l.startswith(expect) for l in self.labels), (expect, self.labels)
            assert not any(l.startswith(f) for l in self.labels for f in forbid), (forbid, self.labels)
        health = ctx.get_health()
        assert health == 0 and ctx.get_health() == 0, f"health word {health}"

    def finish(self):
        """Checks 1 and 2 of the module text; returns ({output name: bits}, {name: values})."""
        for name, t, want in self.ins:
            assert np.array_equal(vl.bits(t), want), f"input {name} was modified"
        out_bits, values = {}, dict(self.extras)
        for ov in self.outs:
            what = f"{ov['name']} ({ov['layout']})"
            vl.assert_outside_untouched(ov["buffer"], ov["inside"], what)
            vl.assert_inside_written(ov["view"][:, :ov["cols_written"]], what)
            out_bits[ov["name"]] = vl.bits(ov["view"])
            values[ov["name"]] = npy(ov["view"])
            # (a NaN the call computed -- from a sentinel it read before writing, say -- has another payload than the sentinel's)
            assert np.isfinite(values[ov["name"]][:, :ov["cols_written"]]).all(), f"{what}: non-finite result"
        g = vl.GUARD
        for name, big, n in self.vecs:
            b = vl.bits(big)
            fill = IDX_SENTINEL if big.dtype == torch.int64 else vl.SENTINEL_BITS[b.dtype.itemsize]
            assert (b[:g] == fill).all() and (b[g + n:] == fill).all(), f"{name}: written outside its {n} entries"
            assert not (b[g:g + n] == fill).any(), f"{name}: entries never written"
            values[name] = b[g:g + n]
        return out_bits, values


# ------------------------------------------------------------------------------------------------------------ entry points
I64, U64 = ctypes.c_int64, ctypes.c_uint64
CHAIN, TALL, COOP, LAZY, BLOCKED = "op:geqp3 ", "op:qrcp_tall_fast", "op:geqp3_wide_coop", "op:geqp3_wide_lazy", "op:geqp3_blocked"
FUSED = "stage:qrcp of B | svd of the core"
FORBID = {TALL: (CHAIN, BLOCKED), COOP: (LAZY, CHAIN), LAZY: (COOP, CHAIN), BLOCKED: (CHAIN,), CHAIN: (TALL, COOP, LAZY, BLOCKED)}


def branch(expect):
    return dict(expect=expect, forbid=FORBID[expect]) if expect else {}


def ep_pivoted_qr(c, m, n, k=None, expect=None, smin=None):
    k = min(m, n) if k is None else k
    c.call("pivoted_qr", c.mat("a", matrix(c.sfx, m, n, 1, smin)), c.out("q", m, k), c.out("r", k, n), c.vec("ind", n, np.int64), **branch(expect))


def ep_pivoted_lq(c, m, n, k=None, expect=None, smin=None):
    k = min(m, n) if k is None else k
    c.call("pivoted_lq", c.mat("a", matrix(c.sfx, m, n, 1, smin)), c.out("l", m, k), c.out("q", k, n), c.vec("ind", m, np.int64), **branch(expect))


def ep_orgqr(c, m, n, kq):
    f, _, tau = o.geqp3_raw(matrix(c.sfx, m, n, 6))
    c.call("orgqr", c.mat("a", f.astype(NP[c.sfx])), c.ptr("tau", tau.astype(NP[c.sfx])), I64(kq), c.out("q", m, kq))


def ep_trsm_upper(c, k, nrhs):
    _, r, _ = o.pivoted_qr(matrix(c.sfx, k + 3, k, 7))
    c.call("trsm_upper", c.mat("t", np.triu(r[:k, :k]).astype(NP[c.sfx])), c.out("b", k, nrhs, init=gaussian(c.sfx, k, nrhs, 8)))


def ep_geqp3(c, m, n, kmax=None, expect=None):
    kmax = min(m, n) if kmax is None else kmax
    c.call("geqp3", c.out("a", m, n, init=matrix(c.sfx, m, n, 1)), I64(kmax), c.vec("jpvt", n, np.int64), c.vec("tau", kmax, NP[c.sfx]), **branch(expect))


def ep_compute_svd(c, m, n, expect=None, smin=None):
    r = min(m, n)
    kw = dict(expect=expect, forbid=(CHAIN,) if expect == "op:cholqr2" else ("op:cholqr2",)) if expect else {}
    c.call("compute_svd", c.mat("a", matrix(c.sfx, m, n, 1, smin)), c.out("u", m, r), c.vec("s", r, REAL[c.sfx]), c.out("vt", r, n), **kw)


def ep_qr_to_mat(c, m, k, n):
    q, r, ind = qr_factors(c.sfx, m, n, k)
    c.call("qr_to_mat", c.mat("q", q), c.mat("r", r), c.ptr("ind", ind), c.out("out", m, n))


def ep_lq_to_mat(c, m, k, n):
    q, r, ind = qr_factors(c.sfx, n, m, k)  # A^H P = Q R  =>  P^T A = R^H Q^H
    c.call("lq_to_mat", c.mat("l", r.conj().T), c.mat("q", q.conj().T), c.ptr("ind", ind), c.out("out", m, n))


def ep_svd_to_mat(c, m, k, n):
    u, s, vt = svd_factors(c.sfx, m, n, k)
    c.call("svd_to_mat", c.mat("u", u), c.ptr("s", s), c.mat("vt", vt), c.out("out", m, n))


def ep_svd_to_qr(c, m, k, n, expect=None):
    u, s, vt = svd_factors(c.sfx, m, n, k)
    c.call("svd_to_qr", c.mat("u", u), c.ptr("s", s), c.mat("vt", vt), c.out("q", m, k), c.out("r", k, n), c.vec("ind", n, np.int64), **branch(expect))


def ep_qr_column_id(c, m, k, n):
    q, r, ind = qr_factors(c.sfx, m, n, k)
    c.call("qr_column_id", c.mat("q", q), c.mat("r", r), c.ptr("ind", ind), c.out("c", m, k), c.out("z", k, n))


def ep_lq_row_id(c, m, k, n):
    q, r, ind = qr_factors(c.sfx, n, m, k)
    c.call("lq_row_id", c.mat("l", r.conj().T), c.mat("q", q.conj().T), c.ptr("ind", ind), c.out("x", m, k), c.out("r_rows", k, n))


def ep_column_id_two_sided(c, m, k, expect=None):
    c.call("column_id_two_sided", c.mat("c", matrix(c.sfx, m, k, 9)), c.out("c_out", m, k), c.out("x", k, k), c.vec("row_ind", m, np.int64), **branch(expect))


def ep_row_id_two_sided(c, k, n, expect=None):
    c.call("row_id_two_sided", c.mat("r", matrix(c.sfx, k, n, 10)), c.out("x", k, k), c.out("r_out", k, n), c.vec("col_ind", n, np.int64), **branch(expect))


def ep_column_id_rank(c, m, n, k, expect=None, smin=None):
    kk = min(k, m, n)
    c.call("column_id_rank", c.mat("a", matrix(c.sfx, m, n, 1, smin)), I64(k), c.out("c", m, kk), c.out("z", kk, n), c.vec("col_ind", n, np.int64), **branch(expect))


def ep_qr_from_range_estimate(c, m, n, rr, expect=None):
    a, rng = range_of(c.sfx, m, n, rr)
    k = min(rr, n)
    c.call("qr_from_range_estimate", c.mat("range", rng), c.mat("a", a), c.out("q", m, k), c.out("r", k, n), c.vec("ind", n, np.int64), **branch(expect))


def ep_svd_from_range_estimate(c, m, n, rr):
    a, rng = range_of(c.sfx, m, n, rr)
    r = min(rr, n)
    c.call("svd_from_range_estimate", c.mat("range", rng), c.mat("a", a), c.out("u", m, r), c.vec("s", r, REAL[c.sfx]), c.out("vt", r, n))


def ep_sample_range_by_rank(c, m, n, k, p, expect=None, smin=None):
    c.call("sample_range_by_rank", c.mat("a", matrix(c.sfx, m, n, 1, smin)), I64(k), I64(p), c.mat("omega", gaussian(c.sfx, n, k + p, 11)), U64(0), c.out("q", m, k),
           **branch(expect))


def ep_sample_range_power_iteration(c, m, n, k, p, expect=None, smin=None):
    c.call("sample_range_power_iteration", c.mat("a", matrix(c.sfx, m, n, 1, smin)), I64(k), I64(p), I64(2), c.mat("omega", gaussian(c.sfx, n, k + p, 11)), U64(0),
           c.out("q", m, k), **({"expect": expect} if expect else {}))


def ep_sample_range_adaptive(c, m, n, s, blocks, cap, rel_tol):
    rank, hlen = I64(-1), I64(-1)
    hist_rank, hist_res = (I64 * blocks)(), (ctypes.c_double * blocks)()
    c.call("sample_range_adaptive", c.mat("a", matrix(c.sfx, m, n, 1)), ctypes.c_double(rel_tol), I64(s), c.mat("omegas", gaussian(c.sfx, n, s * blocks, 12)), U64(0),
           c.out("q_cap", m, cap), ctypes.byref(rank), hist_rank, hist_res, I64(blocks), ctypes.byref(hlen))
    assert 0 < rank.value <= cap and 0 < hlen.value <= blocks
    c.outs[-1]["cols_written"] = rank.value   # "on return the basis is its first *rank columns"
    c.extras.update(rank=np.array(rank.value), hist_rank=np.array(hist_rank[:hlen.value]), hist_res=np.array(hist_res[:hlen.value]).view(np.int64))


def ep_rsvd_id(c, m, n, k, p, expect=None, smin=None):
    a, omega = c.mat("a", matrix(c.sfx, m, n, 1, smin)), c.mat("omega", gaussian(c.sfx, n, k + p, 13))
    out = _lib.rc_rsvd_id_out()
    out.range_q, out.u = c.out("range_q", m, k), c.out("u", m, k)
    out.s = c.vec("s", k, REAL[c.sfx])
    out.vt, out.qr_q, out.qr_r = c.out("vt", k, n), c.out("qr_q", m, k), c.out("qr_r", k, n)
    out.qr_ind = c.vec("qr_ind", n, np.int64)
    out.id_c, out.id_z = c.out("id_c", m, k), c.out("id_z", k, n)
    c.call("rsvd_id", a, I64(k), I64(p), omega, U64(0), ctypes.byref(out), **({"expect": expect} if expect else {}))
    if expect == FUSED:   # the tall QR of B^T certified and the fused launch ran: no second factorization of B afterwards
        assert not any(l.startswith(f) for l in c.labels for f in (CHAIN, LAZY, TALL)), c.labels


def ep_random_gaussian(c, rows, cols):
    c.call("random_gaussian", c.out("out", rows, cols), U64(20240607), U64(5))


DEGENERATE = [(1, 7), (7, 1), (1, 1)]
CASES = []


def add(ep, types, ident, **params):
    for sfx in types:
        CASES.append(pytest.param(ep, sfx, params, id=f"{ep.__name__[3:]}-{sfx}-{ident}"))


# pivoted QR / LQ, full and truncated, on every branch of qrcp_core (LQ: the QR of the transpose, so the shapes are mirrored)
for m, n, k, exp in [(37, 23, None, CHAIN), (37, 23, 5, CHAIN), (23, 37, None, CHAIN), (5, 259, None, COOP), (5, 259, 3, COOP),
                     (131, 137, None, BLOCKED), (131, 137, 9, BLOCKED)]:
    add(ep_pivoted_qr, REALS, f"{m}x{n}-k{k}", m=m, n=n, k=k, expect=exp)
    add(ep_pivoted_lq, REALS, f"{n}x{m}-k{k}", m=n, n=m, k=k, expect=exp)
# (f32 spectrum 1 .. 0.2: the CholeskyQR2 certificate needs cond^2 eps << 1, and the label check below insists on the fast path)
for sfx, smin in (("f64", None), ("f32", 0.2)):
    for k in (None, 4):
        add(ep_pivoted_qr, (sfx,), f"1031x9-k{k}", m=1031, n=9, k=k, expect=TALL, smin=smin)
        add(ep_pivoted_lq, (sfx,), f"9x1031-k{k}", m=9, n=1031, k=k, expect=TALL, smin=smin)
add(ep_pivoted_qr, REALS, "5x259-lazy", m=5, n=259, k=None, expect=LAZY, options={_lib.RC_OPT_WIDE_COOP_QRCP: 0})
add(ep_pivoted_lq, REALS, "259x5-lazy", m=259, n=5, k=None, expect=LAZY, options={_lib.RC_OPT_WIDE_COOP_QRCP: 0})
for m, n, k in [(37, 23, None), (37, 23, 5), (23, 37, None)]:
    add(ep_pivoted_qr, CPLX, f"{m}x{n}-k{k}", m=m, n=n, k=k)
    add(ep_pivoted_lq, CPLX, f"{n}x{m}-k{k}", m=n, n=m, k=k)
for m, n in DEGENERATE:
    add(ep_pivoted_qr, ALL, f"{m}x{n}", m=m, n=n)
    add(ep_pivoted_lq, ALL, f"{m}x{n}", m=m, n=n)
# ?orgqr: form_q's kernels split at m <= 128, <= 512, <= 2048 (kernels_qr.hip form_q); complex: k_c_form_q alone
for m, n, kq in [(37, 23, 23), (37, 23, 5), (131, 137, 131), (1031, 9, 9)]:
    add(ep_orgqr, REALS, f"{m}x{n}-k{kq}", m=m, n=n, kq=kq)
for m, n, kq in [(37, 23, 23), (37, 23, 5)]:
    add(ep_orgqr, CPLX, f"{m}x{n}-k{kq}", m=m, n=n, kq=kq)
for m, n in DEGENERATE:
    add(ep_orgqr, ALL, f"{m}x{n}", m=m, n=n, kq=1)
# triangular solve in place: 16 x 16 tiles (k_trsm_upper), 256 right-hand sides per workgroup
for k, nrhs in [(23, 37), (17, 300), (1, 7), (7, 1), (1, 1)]:
    add(ep_trsm_upper, ALL, f"k{k}-nrhs{nrhs}", k=k, nrhs=nrhs)
# ?geqp3 in place (lapack_geqp3: cooperative short-wide, blocked, chain; the result is gathered into a by gather_cols)
for m, n, kmax, exp in [(37, 23, None, CHAIN), (23, 37, None, CHAIN), (5, 259, None, COOP), (131, 137, None, BLOCKED), (131, 137, 9, BLOCKED)]:
    add(ep_geqp3, REALS, f"{m}x{n}-k{kmax}", m=m, n=n, kmax=kmax, expect=exp)
for m, n in [(37, 23), (23, 37)]:
    add(ep_geqp3, CPLX, f"{m}x{n}", m=m, n=n)
for m, n in DEGENERATE:
    add(ep_geqp3, ALL, f"{m}x{n}", m=m, n=n)
# SVD: both sides of tsqr_supported(M, r) in the tall orientation, tall and wide
for m, n in [(37, 23), (23, 37)] + DEGENERATE:
    add(ep_compute_svd, REALS, f"{m}x{n}", m=m, n=n)
for sfx, smin in (("f64", None), ("f32", 0.2)):
    for m, n in [(1031, 9), (9, 1031)]:
        add(ep_compute_svd, (sfx,), f"{m}x{n}", m=m, n=n, expect="op:cholqr2", smin=smin)
    for m, n in [(1023, 9), (9, 1023)]:
        add(ep_compute_svd, (sfx,), f"{m}x{n}", m=m, n=n, expect=CHAIN, smin=smin)
for m, n in [(37, 23), (23, 37), (61, 23), (23, 61)] + DEGENERATE:   # c_compute_svd: qr_first off / on
    add(ep_compute_svd, CPLX, f"{m}x{n}", m=m, n=n)
# to_mat: the output is the C operand of one product
for m, k, n in [(37, 9, 23), (131, 9, 137), (1, 1, 7), (7, 1, 1), (1, 1, 1)]:
    add(ep_qr_to_mat, ALL, f"{m}x{n}-k{k}", m=m, k=k, n=n)
    add(ep_lq_to_mat, ALL, f"{m}x{n}-k{k}", m=m, k=k, n=n)
    add(ep_svd_to_mat, ALL, f"{m}x{n}-k{k}", m=m, k=k, n=n)
# SVD -> QR: pivoted QR of diag(s) Vt (k x n)
for m, k, n, exp in [(37, 9, 23, CHAIN), (67, 5, 259, COOP)]:
    add(ep_svd_to_qr, REALS, f"{m}x{n}-k{k}", m=m, k=k, n=n, expect=exp)
add(ep_svd_to_qr, CPLX, "37x23-k9", m=37, k=9, n=23)
add(ep_svd_to_qr, ALL, "1x1-k1", m=1, k=1, n=1)
# IDs from given factors: k < n (the fused Z kernel, real types) and k == n (identity and gather)
for m, k, n in [(37, 9, 23), (37, 23, 23), (1, 1, 7), (1, 1, 1)]:
    add(ep_qr_column_id, ALL, f"{m}x{n}-k{k}", m=m, k=k, n=n)
    add(ep_lq_row_id, ALL, f"{n}x{m}-k{k}", m=n, k=k, n=m)
# two-sided IDs: the row ID of C factors C^T (k x m), the column ID of R factors R (k x n)
for m, k, exp in [(37, 9, CHAIN), (259, 5, COOP)]:
    add(ep_column_id_two_sided, REALS, f"{m}x{k}", m=m, k=k, expect=exp)
    add(ep_row_id_two_sided, REALS, f"{k}x{m}", k=k, n=m, expect=exp)
add(ep_column_id_two_sided, CPLX, "37x9", m=37, k=9)
add(ep_row_id_two_sided, CPLX, "9x37", k=9, n=37)
add(ep_column_id_two_sided, ALL, "1x1", m=1, k=1)
add(ep_row_id_two_sided, ALL, "1x1", k=1, n=1)
# rank-k column ID of a dense matrix: column_id_rank's own fast path (blocked, C and Z straight from the factored matrix) and the
# others through qr_column_id
for m, n, k, exp in [(37, 23, 9, CHAIN), (37, 23, 23, CHAIN), (131, 137, 9, BLOCKED), (5, 259, 3, COOP)]:
    add(ep_column_id_rank, REALS, f"{m}x{n}-k{k}", m=m, n=n, k=k, expect=exp)
add(ep_column_id_rank, REALS, "5x259-k3-lazy", m=5, n=259, k=3, expect=LAZY, options={_lib.RC_OPT_WIDE_COOP_QRCP: 0})
for sfx, smin in (("f64", None), ("f32", 0.2)):
    add(ep_column_id_rank, (sfx,), "1031x9-k4", m=1031, n=9, k=4, expect=TALL, smin=smin)
for m, n, k in [(37, 23, 9), (37, 23, 23)]:
    add(ep_column_id_rank, CPLX, f"{m}x{n}-k{k}", m=m, n=n, k=k)
add(ep_column_id_rank, ALL, "1x7-k1", m=1, n=7, k=1)
add(ep_column_id_rank, ALL, "1x1-k1", m=1, n=1, k=1)
# from a range estimate: B = range^H A is rr x n
for m, n, rr, exp in [(37, 23, 9, CHAIN), (67, 261, 5, COOP)]:
    add(ep_qr_from_range_estimate, REALS, f"{m}x{n}-r{rr}", m=m, n=n, rr=rr, expect=exp)
    add(ep_svd_from_range_estimate, REALS, f"{m}x{n}-r{rr}", m=m, n=n, rr=rr)
add(ep_svd_from_range_estimate, REALS, "37x5-r9", m=37, n=5, rr=9)   # rr > n: B is tall (svd_from_range's other branch)
add(ep_qr_from_range_estimate, CPLX, "37x23-r9", m=37, n=23, rr=9)
add(ep_svd_from_range_estimate, CPLX, "37x23-r9", m=37, n=23, rr=9)
add(ep_svd_from_range_estimate, CPLX, "37x5-r9", m=37, n=5, rr=9)
add(ep_qr_from_range_estimate, ALL, "1x1-r1", m=1, n=1, rr=1)
add(ep_svd_from_range_estimate, ALL, "1x1-r1", m=1, n=1, rr=1)
# range finders with an explicit Omega: the sketch Y = A Omega is m x (k + p)
for ep in (ep_sample_range_by_rank, ep_sample_range_power_iteration):
    add(ep, REALS, "37x23-k5p3", m=37, n=23, k=5, p=3, expect=CHAIN)
    for sfx, smin in (("f64", None), ("f32", 0.2)):
        add(ep, (sfx,), "1031x41-k7p2", m=1031, n=41, k=7, p=2, expect=TALL, smin=smin)
    add(ep, CPLX, "37x23-k5p3", m=37, n=23, k=5, p=3)
    add(ep, ALL, "1x1-k1p0", m=1, n=1, k=1, p=0)
add(ep_sample_range_adaptive, ALL, "61x47-s8", m=61, n=47, s=8, blocks=8, cap=48, rel_tol=5e-2)
# the fused pipeline, all nine outputs: B = Q^H A is k x n
add(ep_rsvd_id, REALS, "67x261-k5p3", m=67, n=261, k=5, p=3, expect=COOP)
# (the lazy twin: with both consumers wanted qrcp_core is told to keep B and factors a column-major copy of it)
add(ep_rsvd_id, REALS, "67x261-k5p3-lazy", m=67, n=261, k=5, p=3, expect=LAZY, options={_lib.RC_OPT_WIDE_COOP_QRCP: 0})
for sfx, smin in (("f64", None), ("f32", 0.2)):
    add(ep_rsvd_id, (sfx,), "1031x41-k9p2", m=1031, n=41, k=9, p=2, expect=TALL, smin=smin)
# RC_OPT_FUSED_CONSUMERS (fused_consumers_qualify, rc_api.hip: f64, k = 128, tsqr_supported(n, k), wide_coop_jacobi_supported(k, n)):
# the launch the benchmark times; qr_r, qr_ind and s are written by it and its tails straight into the caller's arrays
add(ep_rsvd_id, ("f64",), "140x1031-k128p5-fused", m=140, n=1031, k=128, p=5, expect=FUSED, smin=1e-4)
add(ep_rsvd_id, CPLX, "37x23-k5p3", m=37, n=23, k=5, p=3)
add(ep_rsvd_id, ALL, "3x2-k1p1", m=3, n=2, k=1, p=1)
# the generator: element (i, j) is number i * cols + j of the stream whatever the strides
for rows, cols in [(37, 23), (1, 7), (7, 1), (1, 1)]:
    add(ep_random_gaussian, ALL, f"{rows}x{cols}", rows=rows, cols=cols)


# ------------------------------------------------------------------------------------------------------------ rounding-only outputs
def wide(sfx):
    return np.complex128 if sfx in CPLX else np.float64


def rel_err(got, want):
    return float(np.linalg.norm(got - want) / max(np.linalg.norm(want), 1e-300))


def rounding_check(ep, name, sfx, values, inputs):
    """(error, bound) of a ROUNDING_ONLY output: the same product evaluated in f64 / c128 on the host from the call's own bit-identical
    siblings (C = Q R11 from the device's q and r), or, where the siblings do not determine it (U = Q_w U_c), the reconstruction
    against the input; bound: tests/helpers.py TOL "factor" / "recon" of the scalar type.  The table is empty, so no case is written."""
    raise AssertionError(f"{ep}.{name} ({sfx}) is listed in ROUNDING_ONLY without a check against its product (TOL: {TOL[np.dtype(REAL[sfx])]})")


# ------------------------------------------------------------------------------------------------------------ the test
@pytest.mark.parametrize("ep, sfx, params", CASES)
def test_output_views(ep, sfx, params):
    params = dict(params)
    options = params.pop("options", {})
    ctx = _lib.default_context()
    problems, worst = [], {}
    try:
        for opt, value in options.items():
            ctx.set_option(opt, value)
        base_bits = base_values = None
        for label, assign in ASSIGNMENTS:
            call = Call(sfx, assign)
            ep(call, **params)
            out_bits, values = call.finish()
            if base_bits is None:
                base_bits, base_values = out_bits, values
                continue
            for name in values:
                if name in out_bits:
                    continue
                if not np.array_equal(values[name], base_values[name]):   # check 3: integers, singular values, tau, histories
                    problems.append(f"{label}: {name} differs from the C baseline")
            for name, b in out_bits.items():                               # check 4
                if np.array_equal(b, base_bits[name]):
                    continue
                key = (ep.__name__[3:], name, sfx)
                if key not in ROUNDING_ONLY:
                    diff = np.argwhere(b != base_bits[name])
                    err = rel_err(values[name].astype(wide(sfx)), base_values[name].astype(wide(sfx)))
                    problems.append(f"{label}: {name} is not bit-identical to the C baseline ({len(diff)} words, first {diff[0].tolist()}, relative {err:.3e})")
                    continue
                err, bound = rounding_check(key[0], name, sfx, values, {n: npy(t) for n, t, _ in call.ins})
                worst[key] = max(worst.get(key, 0.0), err / bound)
                if err > bound:
                    problems.append(f"{label}: {name} misses {ROUNDING_ONLY[key]}'s product by {err:.3e} > {bound:.1e}")
    finally:
        for opt in options:
            ctx.set_option(opt, 1)
    for key, ratio in worst.items():
        print(f"ROUNDING_ONLY {key}: worst error / bound = {ratio:.3e}")
    assert not problems, "\n".join(problems)
