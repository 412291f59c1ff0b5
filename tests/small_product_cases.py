"""Inputs and runners shared by tests/test_gpu_small_product_folds.py and its worker (tests/small_product_folds_worker.py).

The second pass of the tall-skinny CholeskyQR2 reduces to the identity whenever the first pass left max |Q1^T Q1 - I| below
2.5e-14 (f64) / 1e-6 (f32): every Gaussian input does.  graded() builds inputs on which it does not: A = U diag(geomspace(1, lo,
n)) V^T with U, V from the QR of seeded Gaussians.  The first-pass defect is about cond(A)^2 eps (5e-10 .. 1e-9 at lo = 1e-4 in
f64, 1e-5 at lo = 1/30 in f32), inside the window in which the second pass runs and certifies; with V dense the pivots are
determined by the data (runner-up ratio of every pivot <= 0.99994).  Scaling the columns of a Gaussian does NOT do it: the
Cholesky factor absorbs a column scaling and the defect stays at 1e-15."""
import ctypes

import numpy as np


def graded(m, n, lo, seed, dtype=np.float64):
    rng = np.random.default_rng(seed)
    u, _ = np.linalg.qr(rng.standard_normal((m, n)))
    v, _ = np.linalg.qr(rng.standard_normal((n, n)))
    return np.ascontiguousarray((u * np.geomspace(1.0, lo, n)) @ v.T).astype(dtype)


# (name, m, n, k, lo, dtype): through rc_pivoted_qr_*
QR_CASES = [
    ("48_nt2", 1024, 48, 48, 1e-4, np.float64),      # k_chol_inv<., 2>, Q2 formed inside k_qrcp_small, the products in their own launch
    ("72_k64", 1024, 72, 64, 1e-4, np.float64),
    ("133_k128", 1024, 133, 128, 1e-4, np.float64),  # the shapes of the flagship workload's range finder
    ("139_full", 1024, 139, 139, 1e-4, np.float64),  # the largest triangle of the route
    ("72_k64_f32", 1024, 72, 64, 1.0 / 30.0, np.float32),
]
SVD_CASE = ("svd_128", 1024, 128, 1e-4)              # through rc_compute_svd_f64: the small product's own launch, U_c side


def qr_case_input(case):
    name, m, n, k, lo, dtype = case
    return graded(m, n, lo, 1000 + n, dtype)


def svd_case_input():
    _, m, n, lo = SVD_CASE
    return graded(m, n, lo, 2000 + n)


def op_names(ctx, lib):
    """{name: calls} of the stage timers."""
    cnt = ctypes.c_int32(0)
    ctx.check(lib.rc_profile_count(ctx._h, ctypes.byref(cnt)))
    names = {}
    for i in range(cnt.value):
        name = ctypes.create_string_buffer(192)
        ms, calls = ctypes.c_double(0), ctypes.c_int64(0)
        ctx.check(lib.rc_profile_get(ctx._h, i, name, 192, ctypes.byref(ms), ctypes.byref(calls)))
        names[name.value.decode()] = calls.value
    return names


def pivoted_qr_at(a, k, settings):
    """{(hint, slots): (q, r, ind, names)} of rc_pivoted_qr_f64 / _f32 on one context; outputs poisoned before each run."""
    import torch

    from rusty_compression_amd import _lib
    from tests.helpers import npy

    lib = _lib.lib()
    m, n = a.shape
    tdt = torch.float64 if a.dtype == np.float64 else torch.float32
    fn = "rc_pivoted_qr_f64" if a.dtype == np.float64 else "rc_pivoted_qr_f32"
    st = torch.cuda.Stream()
    out = {}
    with torch.cuda.stream(st):
        ctx = _lib.Context(torch.cuda.current_device(), st.cuda_stream)
        ta = torch.from_numpy(a).to("cuda")
        q = torch.empty((m, k), dtype=tdt, device="cuda")
        r = torch.empty((k, n), dtype=tdt, device="cuda")
        ind = torch.empty(n, dtype=torch.int64, device="cuda")
        st.synchronize()
        for hint, slots in settings:
            ctx.set_option(_lib.RC_OPT_KERNEL_SLOTS, slots)
            ctx.set_option(_lib.RC_OPT_CONCURRENCY_HINT, hint)
            q.fill_(float("nan")), r.fill_(float("nan")), ind.fill_(-1)
            lib.rc_profile_enable(ctx._h, 1)
            lib.rc_profile_reset(ctx._h)
            ctx.call(fn, _lib.mat(ta), _lib.mat(q), _lib.mat(r), ctypes.c_void_p(ind.data_ptr()))
            names = op_names(ctx, lib)
            lib.rc_profile_enable(ctx._h, 0)
            ctx.synchronize()
            assert ctx.get_health() == 0, (hint, slots, ctx.get_health())
            out[(hint, slots)] = (npy(q).copy(), npy(r).copy(), npy(ind).copy(), names)
        ctx.close()
    return out


def compute_svd_at(a, settings):
    """{(hint, slots): (u, s, vt, names)} of rc_compute_svd_f64 on one context."""
    import torch

    from rusty_compression_amd import _lib
    from tests.helpers import npy

    lib = _lib.lib()
    m, n = a.shape
    r_ = min(m, n)
    st = torch.cuda.Stream()
    out = {}
    with torch.cuda.stream(st):
        ctx = _lib.Context(torch.cuda.current_device(), st.cuda_stream)
        ta = torch.from_numpy(a).to("cuda")
        u = torch.empty((m, r_), dtype=torch.float64, device="cuda")
        s = torch.empty(r_, dtype=torch.float64, device="cuda")
        vt = torch.empty((r_, n), dtype=torch.float64, device="cuda")
        st.synchronize()
        for hint, slots in settings:
            ctx.set_option(_lib.RC_OPT_KERNEL_SLOTS, slots)
            ctx.set_option(_lib.RC_OPT_CONCURRENCY_HINT, hint)
            u.fill_(float("nan")), s.fill_(float("nan")), vt.fill_(float("nan"))
            lib.rc_profile_enable(ctx._h, 1)
            lib.rc_profile_reset(ctx._h)
            ctx.call("rc_compute_svd_f64", _lib.mat(ta), _lib.mat(u), ctypes.c_void_p(s.data_ptr()), _lib.mat(vt))
            names = op_names(ctx, lib)
            lib.rc_profile_enable(ctx._h, 0)
            ctx.synchronize()
            assert ctx.get_health() == 0, (hint, slots, ctx.get_health())
            out[(hint, slots)] = (npy(u).copy(), npy(s).copy(), npy(vt).copy(), names)
        ctx.close()
    return out


def qr_identities(a, k, q, r, ind, ref):
    """The properties of a truncated pivoted QR that hold whatever the summation order; ref = oracle.ref_lapack.pivoted_qr(a), the
    FULL factorization.  After k steps the first k pivots, Q[:, :k] and the first k rows of every column of R are final, so
    those are compared; the order of the n - k columns that never became a pivot is the library's own (it stops after k steps,
    LAPACK goes on), so column j >= k of R is held against LAPACK's column of the same index ind[j].
    Returns (max |Q - Q_lapack|, max |R - R_lapack|) for the caller's entry-wise bound."""
    f64 = a.dtype == np.float64
    oq, orr, oind = (np.asarray(x) for x in ref)
    n = a.shape[1]
    a64, q64, r64 = a.astype(np.float64), q.astype(np.float64), r.astype(np.float64)
    assert np.array_equal(ind[:k], oind[:k]), np.nonzero(ind[:k] != oind[:k])[0][:4]
    assert sorted(ind.tolist()) == list(range(n))
    orth = float(np.abs(q64.T @ q64 - np.eye(k)).max())
    assert orth <= (1e-13 if f64 else 1e-5), orth                # (f32: the bound of tests/test_gpu_parity.py for the tall pivoted QR)
    res = float(np.linalg.norm(a64[:, ind[:k]] - q64 @ r64[:, :k]) / np.linalg.norm(a64))
    assert res <= (1e-13 if f64 else 1e-5), res
    assert np.array_equal(np.tril(r, -1), np.zeros_like(r))
    assert np.array_equal(np.sign(np.diag(r)), np.sign(np.diag(orr)[:k])), "signs of diag(R) differ from LAPACK's"
    opos = np.empty(n, dtype=np.int64)
    opos[oind] = np.arange(n)
    r_ref = orr.astype(np.float64)[:k][:, opos[ind]]             # LAPACK's first k rows, columns in the library's order
    return float(np.abs(q64 - oq.astype(np.float64)[:, :k]).max()), float(np.abs(r64 - r_ref).max())


def small_products_left(names):
    """The entries of the stage timers that are a product with all of M, N, K <= 144, or the slab reduction of one.  A reduction's
    name carries M, N and its split count only: it is attributed to the products of the same M x N, all of which must then have
    K > 144 (and there must be at least as many of them as reductions)."""
    import re

    gemms, left = {}, []
    for nm, calls in names.items():
        mt = re.match(r"kernel:k_gemm_mfma<\w+> M=(\d+) N=(\d+) K=(\d+)", nm)
        if mt:
            m_, n_, k_ = map(int, mt.groups())
            gemms.setdefault((m_, n_), []).append((k_, calls))
            if max(m_, n_, k_) <= 144:
                left.append(nm)
    for nm, calls in names.items():
        mt = re.match(r"kernel:k_splitk_reduce M=(\d+) N=(\d+)", nm)
        if mt and max(map(int, mt.groups())) <= 144:
            same = gemms.get(tuple(map(int, mt.groups())), [])
            if not same or any(k_ <= 144 for k_, _ in same):
                left.append(nm)
    for (m_, n_), ks in gemms.items():
        red = sum(c for nm, c in names.items() if nm.startswith("kernel:k_splitk_reduce M=%d N=%d " % (m_, n_)))
        if max(m_, n_) <= 144 and red > sum(c for _, c in ks):
            left.append("more reductions than products of %d x %d" % (m_, n_))
    return left
