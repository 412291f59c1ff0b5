"""Every route of the real dense SVD (rc_compute_svd_f64 / _f32) and of the batched SVD on tiny and zero singular values.

The inputs, the bounds and the route table come from tests/svd_cases.py (tests/test_svd_cases_cpu.py shows that LAPACK meets every
bound on every input used here).  Orthonormality is asked of ALL min(m, n) columns of U and V.

Routes, by the size r = min(m, n) of the square core (jacobi_svd, launch_lds, jacobi_pitch):
    r <= 128                       k_jacobi_lds, V accumulated by the second workgroup of the same launch ("fused")
    129 <= r <= last LDS core      k_jacobi_lds + k_jacobi_replay_v ("replay"); last LDS core: f64 141 (LDS bytes, pitch n | 1),
                                   f32 192 (16 lanes x 12 rows)
    beyond                         k_jacobi_round per round in global memory ("global")
Which of them ran is read from the event profile: op:jacobi_svd n=<r> always, info:jacobi_sweeps n=<r> from the LDS launches only.
Fused versus replay is NOT observed: it follows from r by launch_lds_impl's rule (svd_cases.core_is_fused), which the summary uses.
Reductions to the core: the unpivoted Householder QR (op:geqp3) for square and moderately tall inputs, CholeskyQR2 (op:cholqr2) where
tsqr_supported holds (M >= 1024, M >= 4 r, the r x r image fits LDS: in f64 r <= 139, so the first global f64 core, 142, is always
reduced by Householder), with the fall-back to Householder when CholeskyQR2's certificate fails (rank-deficient input: both labels)."""
import ctypes

import numpy as np
import pytest
import torch

import rusty_compression_amd as rc
from rusty_compression_amd import _lib
from tests import svd_cases as sc
from tests.helpers import npy

pytestmark = pytest.mark.gpu

DTYPES = [np.float64, np.float32]
WORST = {}  # (dtype name, route) -> {"sval", "orth", "recon", "cases"}


def profiled(fn):
    """fn() on the default context with the event profile on: (fn's result, {label: calls})."""
    ctx = _lib.default_context()
    lib = _lib.lib()
    labels = {}
    ctx.check(lib.rc_profile_enable(ctx._h, 1))
    try:
        ctx.check(lib.rc_profile_reset(ctx._h))
        out = fn()
        cnt = ctypes.c_int32(0)
        ctx.check(lib.rc_profile_count(ctx._h, ctypes.byref(cnt)))
        for i in range(cnt.value):
            name = ctypes.create_string_buffer(192)
            ms, calls = ctypes.c_double(0), ctypes.c_int64(0)
            ctx.check(lib.rc_profile_get(ctx._h, i, name, 192, ctypes.byref(ms), ctypes.byref(calls)))
            labels[name.value.decode()] = calls.value
    finally:
        lib.rc_profile_enable(ctx._h, 0)
        lib.rc_profile_reset(ctx._h)
    return out, labels


def core_route(r, dtype):
    return ("lds-fused" if sc.core_is_fused(r) else "lds-replay") if sc.core_is_lds(r, dtype) else "global"


def route_name(m, n, dtype):
    """<route of the core>+<reduction the shape is eligible for>, the key of the summary lines."""
    r = min(m, n)
    return core_route(r, dtype) + ("+cholqr2" if sc.tsqr_supported(max(m, n), r, dtype) else "+householder")


def record(dtype, route, m):
    w = WORST.setdefault((np.dtype(dtype).name, route), {"sval": 0.0, "orth": 0.0, "recon": 0.0, "cases": 0})
    w["sval"] = max(w["sval"], m.get("sval", 0.0))
    w["orth"] = max(w["orth"], m.get("orth_u", 0.0), m.get("orth_v", 0.0))
    w["recon"] = max(w["recon"], m.get("recon", 0.0))
    w["cases"] += 1


@pytest.fixture(scope="module", autouse=True)
def worst_values_summary():
    """One line per (dtype, route) with the worst values seen (failed cases included), printed when the module is done: the lines
    are the teardown output of the module's last test (shown with `pytest -s`, or with `-rA` in the summary of that test)."""
    yield
    print()
    for (dt, route), w in sorted(WORST.items()):
        print("svd-routes worst %s %-24s cases=%-3d sval=%.2e orth=%.2e recon=%.2e" % (dt, route, w["cases"], w["sval"], w["orth"], w["recon"]))


def run_dense(a, dtype):
    """rc.compute_svd(a) with the health word read and cleared before and asserted clean after, the core's route asserted from the
    profile labels, every bound of check_svd asserted; returns (u, s, vt, labels)."""
    m, n = a.shape
    r = min(m, n)
    ctx = _lib.default_context()
    ctx.get_health()
    (u, s, vt), labels = profiled(lambda: tuple(npy(t) for t in rc.compute_svd(torch.from_numpy(a).cuda())))
    health = ctx.get_health()
    lds = sc.core_is_lds(r, dtype)
    assert labels.get("op:jacobi_svd n=%d" % r) == 1, sorted(labels)
    assert [k for k in labels if k.startswith("op:jacobi_svd")] == ["op:jacobi_svd n=%d" % r], sorted(labels)
    assert (labels.get("info:jacobi_sweeps n=%d" % r) == 1) == lds, (lds, sorted(labels))
    assert [k for k in labels if k.startswith("info:jacobi_sweeps")] == (["info:jacobi_sweeps n=%d" % r] if lds else []), sorted(labels)
    measured = {}
    try:
        sc.check_svd(a, u, s, vt, dtype, measured=measured)
    finally:
        record(dtype, route_name(m, n, dtype), measured)
    assert health == 0, health
    return u, s, vt, labels


def reduction_labels(labels):
    return any(k.startswith("op:cholqr2 ") for k in labels), any(k.startswith("op:geqp3 ") for k in labels)


def route_params():
    return [pytest.param(dt, case, id="%s-%s" % (np.dtype(dt).name, sc.case_id(case))) for dt in DTYPES for case in sc.route_cases(dt)]


def test_route_edges_follow_the_sources():
    """The sizes the cases below are written around, derived from the restated formulas: a change of kJacobiLdsCap, of the pitch
    rule or of the largest LDS instance moves last_lds_core, and the label assertions of the cases at 141 / 142 and 192 / 193 fail."""
    assert sc.last_lds_core(np.float64) == 141 and sc.last_lds_core(np.float32) == 192
    for dt in DTYPES:
        last = sc.last_lds_core(dt)
        assert {129, last, last + 1, last + 2} <= set(sc.CORE_SIZES[np.dtype(dt)])
        assert core_route(128, dt) == "lds-fused" and core_route(129, dt) == "lds-replay" and core_route(last, dt) == "lds-replay"
        assert core_route(last + 1, dt) == "global"


@pytest.mark.parametrize("dtype,case", route_params())
def test_dense_svd_route(dtype, case):
    """Gaussian, numerically rank-deficient (scale * X Y^T, f32 at the scales 1, 4^-5, 4^-8) and exactly rank-deficient inputs on
    every core size at an edge of the route table and through every reduction to the core."""
    shape, gen, scale = case
    m, n = shape
    r = min(m, n)
    a = sc.make_case(shape, gen, scale, dtype)
    chol_shape = sc.tsqr_supported(max(m, n), r, dtype)
    u, s, vt, labels = run_dense(a, dtype)
    chol, house = reduction_labels(labels)
    if not chol_shape:
        assert (chol, house) == (False, True), sorted(labels)
    elif gen == "gaussian":
        assert (chol, house) == (True, False), sorted(labels)
    else:  # the certificate of CholeskyQR2 fails on a rank-deficient Gram matrix and the call falls back
        assert (chol, house) == (True, True), sorted(labels)
    if gen == "exact_zeros":
        rank = sc.exact_zeros_rank(m, n)
        assert np.all(s[rank:] == 0) and np.all(s[:rank] > 0)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("which", [0, 1, 2])
def test_dense_svd_of_clustered_spectra(dtype, which):
    """Clustered, repeated and two-cluster singular values on a fused core (64), a replay core (129) and the first global core."""
    r = sc.reduction_sizes(dtype)[which]
    for name, a in sc.clustered(r, r, dtype).items():
        run_dense(a, dtype)


@pytest.mark.parametrize("dtype,n", [(dt, n) for dt in DTYPES for n in sc.GRADED_SIZES[np.dtype(dt)]])
def test_dense_svd_of_graded_cores(dtype, n):
    """G diag(2^-linspace(0, 30, n)): the input on which the recompression kernel's f32 Jacobi lost the orthogonality of U."""
    run_dense(sc.graded(n, dtype), dtype)


@pytest.mark.parametrize("dtype,shape", [(np.float64, (142, 142)), (np.float32, (150, 150))])
@pytest.mark.parametrize("gen", ["gaussian", "low_rank"])
def test_captured_svd_replays_the_eager_bits(dtype, shape, gen):
    """rc_compute_svd recorded into a hipGraph on a private context and replayed twice into zeroed outputs: both replays equal the
    eager outputs bit for bit.  f64 142 x 142 is the global route (kMaxSweeps = 30 recorded sweeps, of which the ones after
    convergence return at once; eagerly the loop stops at the same sweep), f32 150 x 150 the LDS route with the replay of V; square
    inputs take the unpivoted Householder reduction with and without capture, so no kernel differs between the two.  The low_rank
    core needs 22 sweeps: with the 16 sweeps recorded before, its replay came back unconverged with health bit 4 raised."""
    lib = _lib.lib()
    m, n = shape
    r = min(m, n)
    an = sc.make_case(shape, gen, 1.0, dtype)
    tdt = torch.float64 if dtype == np.float64 else torch.float32
    name = "rc_compute_svd_f64" if dtype == np.float64 else "rc_compute_svd_f32"
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        ctx = _lib.Context(torch.cuda.current_device(), st.cuda_stream)
        a = torch.from_numpy(an).cuda()
        u = torch.empty((m, r), dtype=tdt, device="cuda")
        s = torch.empty(r, dtype=tdt, device="cuda")
        vt = torch.empty((r, n), dtype=tdt, device="cuda")
        args = (_lib.mat(a), _lib.mat(u), ctypes.c_void_p(s.data_ptr()), _lib.mat(vt))
        ctx.get_health()
        ctx.call(name, *args)
        ctx.synchronize()
        eu, es, evt = u.clone(), s.clone(), vt.clone()
        graph = ctypes.c_void_p(None)
        ctx.check(lib.rc_graph_begin_capture(ctx._h))
        ctx.call(name, *args)
        ctx.check(lib.rc_graph_end_capture(ctx._h, ctypes.byref(graph)))
        replays = []
        for _ in range(2):
            u.zero_(); s.zero_(); vt.zero_()
            ctx.check(lib.rc_graph_launch(ctx._h, graph))
            ctx.synchronize()
            replays.append((u.clone(), s.clone(), vt.clone()))
        health = ctx.get_health()
        ctx.check(lib.rc_graph_destroy(ctx._h, graph))
        ctx.close()
    measured = {}
    try:
        sc.check_svd(an, npy(eu), npy(es), npy(evt), dtype, measured=measured)
    finally:
        record(dtype, route_name(m, n, dtype), measured)
    for i, (gu, gs, gvt) in enumerate(replays):
        assert torch.equal(gs, es) and torch.equal(gu, eu) and torch.equal(gvt, evt), "replay %d differs from the eager call" % i
    assert health == 0, health


@pytest.mark.parametrize("dtype", [np.float32, np.complex64, np.float64, np.complex128])
@pytest.mark.parametrize("shape", sc.BATCHED_SHAPES)
def test_batched_svd_of_scaled_low_rank_neighbours(dtype, shape):
    """rc_svd_rank_batched_* at full rank (k = min(m, n), tol = 0) on a batch of 5 whose matrices 1 and 3 are low_rank at the scales
    4^-5 and 4^-8: every matrix through check_one of the batched SVD's own test file (f64 and c64 are controls)."""
    from tests.test_gpu_batched_svd import check_one as check_real
    from tests.test_gpu_batched_svd_complex import check_one as check_complex

    m, n = shape
    k = min(m, n)
    cplx = np.dtype(dtype).kind == "c"
    a = sc.batched_case(m, n, dtype)
    ctx = _lib.default_context()
    ctx.get_health()
    fn = rc.svd_rank_batched_complex if cplx else rc.svd_rank_batched
    u, s, vt, ranks = (npy(t) for t in fn(torch.from_numpy(a).cuda(), k, 0.0))
    torch.cuda.synchronize()
    health = ctx.get_health()
    real = np.float64 if np.dtype(dtype) in (np.dtype(np.float64), np.dtype(np.complex128)) else np.float32
    failures, orths = [], []
    for i in range(5):
        wide = a[i].astype(np.complex128 if cplx else np.float64)
        uu, vv = u[i].astype(wide.dtype), vt[i].astype(wide.dtype)
        orth = max(np.abs(uu.conj().T @ uu - np.eye(k)).max(), np.abs(vv @ vv.conj().T - np.eye(k)).max())
        orths.append(float(orth))
        record(real, "batched-" + np.dtype(dtype).name, {"orth_u": float(orth), "recon": float(np.linalg.norm(wide - (uu * s[i].astype(np.float64)) @ vv) / np.linalg.norm(wide))})
        assert ranks[i] == k, (i, ranks[i])  # (tol = 0: fixed rank unless a singular value is exactly zero)
        try:
            if cplx:
                check_complex(a[i], u[i], s[i], vt[i], k, dtype)
            else:
                check_real(a[i], u[i], s[i], vt[i], k, k, dtype)
        except AssertionError as e:
            failures.append((i, str(e).splitlines()[0][:120] if str(e) else ""))
    assert not failures, "check_one fails on %s; max |U^H U - I|, |V^H V - I| per matrix: %s" % (failures, ["%.2e" % x for x in orths])
    assert health == 0, health
