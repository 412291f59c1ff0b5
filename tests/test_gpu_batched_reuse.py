"""The six batched kernels where one workgroup factors several matrices in a row.

k_batched_id, k_batched_two_sided, k_batched_svd and their complex twins run a persistent grid of G workgroups; workgroup w
factors b = w, w + G, w + 2G, ... and keeps its LDS arrays and its slot of the global workspace across that loop.  "Matrix b's bits
depend on matrix b alone" therefore needs every later iteration to start from state as good as fresh.  Each case below

  * reads G (`slots`) and the storage plan from the profile label of a one-matrix probe call (tests.helpers.batched_launch),
  * launches count = 2 G + G // 2 + 1 matrices and asserts from that call's own label that grid == G, count > 2 grid (a third
    iteration ran) and that the shape selected the plan the case is named after,
  * fills block 0 (b < G) with predecessors of eight kinds (full rank, zero, rank 1, rank 5, one NaN, an Inf column, x 1e3,
    x 1e-3) and blocks 1 and 2 with four fixed successors S0 .. S3 so that every (predecessor kind, successor) pair occurs and
    every successor also follows another successor,
  * and requires every output of every successor to equal, bit for bit, the output of the same matrix in a four-matrix call (count
    <= grid: each matrix first on a fresh workgroup), whose results in turn pass the family's own check against the SciPy-LAPACK
    oracle with the tolerances of that family's test file.

Shapes: the smallest / nearest-to-the-boundary ones that select each plan, from bid_lds_bytes, bts_lds_bytes, bsv_lds_bytes,
bic_lds_bytes, btc_lds_bytes, bsc_lds_bytes and BID_MAX_LDS = 162816 bytes (kernels_batched_id.hip, kernels_batched_id_c.hip):

  IDs (W in LDS iff n (m|1) elements + the small arrays fit; the two-sided kernel reserves max(n (m|1), m (k|1))):
    f64  203 x 96 -> 162588 B (LDS), 206 x 96 (workspace);  96 x 201 -> 162620 B (LDS),  96 x 202 (workspace)
    f32  307 x 128 -> 162500 B,      312 x 128;             128 x 305 -> 162672 B,       128 x 307
    c64  153 x 64 -> 161204 B,       156 x 64;              64 x 152 -> 162592 B,        64 x 153
    c32  207 x 96 -> 162452 B,       210 x 96;              96 x 205 -> 162532 B,        96 x 206
  SVD, real (plans in the order batched_svd tries them; pad = 32 ((N + 15) / 32) + 16, odd = N | 1):
    0 W,V,G in LDS, pad   96 x 40 (f64 63952 B, f32 32400 B)      3 W ws, odd          160 x 96 f64 (153424 B)
    1 W,V,G in LDS, odd   92 x 79 f64 (162384 B), 118 x 114 f32   4 W,V ws, pad        200 x 128 f64 (153168 B)
    2 W ws, pad           200 x 64 f64, 200 x 128 f32             5 W,V ws, odd        unreachable
    Plan 5 needs N pad sizeof(T) + the small arrays > BID_MAX_LDS; at the largest admissible core, N = 128 (pad = 144) in f64,
    plan 4 takes 153168 B, so no admissible shape (m, n <= 512, min <= 128) selects plan 5.  In f32 plan 2 at N = 128 takes
    151088 B and fits for every M, so plans 3, 4 and 5 are unreachable too.
  SVD, complex (a seventh plan keeps the core G in the workspace as well):
    c64  0: 96 x 40   1: 60 x 56   2: 200 x 40   3: 160 x 64   4: 160 x 80   5: 160 x 96   6: 160 x 128 (and 128 x 128)
    c32  0: 96 x 40   1: 92 x 79   2: 200 x 64   3: 160 x 96   4: 200 x 128;  plans 5 and 6 are unreachable: plan 4 at
         N = 128 takes 152112 B.
These strings are asserted against the launch's label, so a retuned BID_MAX_LDS or LDS formula fails here instead of silently
moving the shapes onto one plan."""
import ctypes

import numpy as np
import pytest
import torch

import rusty_compression_amd as rc
from oracle import ref_lapack as o
from rusty_compression_amd import _lib
from tests import test_gpu_batched_id as t_id
from tests import test_gpu_batched_id_complex as t_idc
from tests import test_gpu_batched_svd as t_svd
from tests import test_gpu_batched_svd_complex as t_svdc
from tests import test_gpu_batched_two_sided_id as t_ts
from tests import test_gpu_batched_two_sided_id_complex as t_tsc
from tests.helpers import batched_launch

pytestmark = pytest.mark.gpu

F64, F32, C64, C32 = np.float64, np.float32, np.complex128, np.complex64
KINDS = "abcdefgh"  # full rank, zero, rank 1, rank 5, one NaN, an Inf column, x 1e3, x 1e-3
CLEAN = [KINDS.index(c) for c in "acdgh"]
NSUCC = 4


def _real(dtype):
    return np.dtype(F64) if np.dtype(dtype) in (np.dtype(F64), np.dtype(C64)) else np.dtype(F32)


def _id_check(mod):
    def check(a, out, k, tol, dtype):
        c, z, ind, r = out
        mod.check_one(a, c, z, ind, int(r), k, dtype, oracle_tol=tol if tol > 0 and r < k else None)
    return check


def _ts_check(mod):
    def check(a, out, k, tol, dtype):
        mod.check_one(a, *out[:5], int(out[5]), k, dtype)
    return check


def _svd_check(a, out, k, tol, dtype):
    u, s, vt, r = out
    if np.dtype(dtype).kind == "c":
        t_svdc.check_one(a, u, s, vt, int(r), dtype)
    else:
        t_svd.check_one(a, u, s, vt, int(r), k, dtype)


# family -> (op of the label, the C entry point's stem, per scalar kind: the call, the test file's host-side call, its check)
FAMILIES = {
    "column_id": ("batched_column_id", "rc_column_id_rank_batched", {"f": (rc.column_id_rank_batched, t_id.batched, _id_check(t_id)),
                                                                     "c": (rc.column_id_rank_batched, t_idc.batched, _id_check(t_idc))}),
    "two_sided_id": ("batched_two_sided_id", "rc_two_sided_id_rank_batched", {"f": (rc.two_sided_id_rank_batched, t_ts.two_sided, _ts_check(t_ts)),
                                                                              "c": (rc.two_sided_id_rank_batched, t_tsc.two_sided, _ts_check(t_tsc))}),
    "svd": ("batched_svd", "rc_svd_rank_batched", {"f": (rc.svd_rank_batched, t_svd.batched, _svd_check),
                                                   "c": (rc.svd_rank_batched_complex, t_svdc.batched, _svd_check)}),
}
N_FACTORS = {"column_id": 2, "two_sided_id": 3, "svd": 3}  # the leading outputs that are factors (zero for a zero matrix)


def clustered(p):
    """The clustered spectrum of test_clean_inputs_leave_the_health_word_clear (10 / 40 / 78 of 128 values), scaled to p values."""
    n1 = max(1, p * 10 // 128)
    n2 = min(p - n1, max(1, p * 40 // 128))
    n3 = p - n1 - n2
    return np.concatenate([np.ones(n1), 0.5 * np.ones(n2), 1e-3 * (1 + 1e-9 * np.arange(n3))])


def host_matrices(m, n, dtype, seed):
    """The eight predecessors (KINDS) and the four successors S0 .. S3 as one [12, m, n] host array."""
    rng = np.random.default_rng(seed)
    cplx = np.dtype(dtype).kind == "c"
    wide = C64 if cplx else F64
    svd_mod = t_svdc if cplx else t_svd

    def gauss(scale=1.0):
        return (o.random_gaussian((m, n), rng, wide) * scale).astype(dtype)

    def low_rank(r):
        return (o.random_gaussian((m, r), rng, wide) @ o.random_gaussian((r, n), rng, wide)).astype(dtype)

    nan = gauss()
    nan[m // 3, n // 2] = np.nan
    inf = gauss()
    inf[:, n // 3] = np.inf
    preds = [gauss(), np.zeros((m, n), dtype=dtype), low_rank(1), low_rank(5), nan, inf, gauss(1e3), gauss(1e-3)]
    lo = 1e-10 if _real(dtype) == np.dtype(F64) else 1e-4
    succ = [svd_mod.decaying(rng, m, n, dtype, lo), gauss(), svd_mod.with_spectrum(rng, m, n, clustered(min(m, n)), dtype), low_rank(3)]
    return np.stack(preds + succ)


def sources(g, count, clean_only=False):
    """Which host matrix each batch entry is: block 0 cycles through the predecessor kinds; workgroup w's first successor is
    S[(w // 8) % 4], so that G >= 32 gives every (kind, successor) pair; block 2 is block 1 shifted by one."""
    w = torch.arange(g)
    kind = w % len(KINDS)
    if clean_only:
        kind = torch.where((kind == KINDS.index("e")) | (kind == KINDS.index("f")), torch.zeros_like(kind), kind)
    s1 = (w // len(KINDS)) % NSUCC
    w2 = torch.arange(count - 2 * g)
    s2 = ((w2 // len(KINDS)) % NSUCC + 1) % NSUCC
    return torch.cat([kind, len(KINDS) + s1, len(KINDS) + s2])


def bits(t):
    """The tensor as integers: equality of these is equality bit for bit (NaN payloads and signed zeros included)."""
    if t.is_complex():
        t = torch.view_as_real(t)
    if t.is_floating_point():
        t = t.contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32)
    return t


def same_bits(x, y):
    return bool((bits(x) == bits(y)).all())


def raw_call(ctx, stem, family, a, k, tol, outs):
    """The C entry point on `ctx` with the wrappers' contiguous output layout (for the captured launch)."""
    cnt, m, n = a.shape
    kk = min(k, m, n)
    i64, mat = ctypes.c_int64, _lib.mat
    head = (_lib.rc_matrix(a.data_ptr(), m, n, a.stride(1), a.stride(2)), i64(a.stride(0)), ctypes.c_int32(cnt), i64(k), ctypes.c_double(tol))
    if family == "column_id":
        c, z, ind, ranks = outs
        tail = (mat(c[0]), i64(m * kk), mat(z[0]), i64(kk * n), _lib.i64p(ind), _lib.i64p(ranks))
    elif family == "two_sided_id":
        c, x, r, row_ind, col_ind, ranks = outs
        tail = (mat(c[0]), i64(m * kk), mat(x[0]), i64(kk * kk), mat(r[0]), i64(kk * n), _lib.i64p(row_ind), _lib.i64p(col_ind), _lib.i64p(ranks))
    else:
        u, s, vt, ranks = outs
        tail = (mat(u[0]), i64(m * kk), ctypes.c_void_p(s.data_ptr()), mat(vt[0]), i64(kk * n), _lib.i64p(ranks))
    ctx.check(getattr(_lib.lib(), f"{stem}_{_lib.suffix(a.dtype)}")(ctx._h, *head, *tail))


def graph_replay(stem, family, a, k, tol, eager):
    """test_graph_capture_replays_the_eager_bits' pattern on the reuse batch: the replayed launch gives the eager bits."""
    lib = _lib.lib()
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        ctx = _lib.Context(torch.cuda.current_device(), st.cuda_stream)
        outs = tuple(torch.zeros_like(t) for t in eager)
        st.synchronize()
        raw_call(ctx, stem, family, a, k, tol, outs)  # eager once: sizes the workspace
        ctx.synchronize()
        ctx.get_health()
        for t in outs:
            t.zero_()
        st.synchronize()
        graph = ctypes.c_void_p(None)
        ctx.check(lib.rc_graph_begin_capture(ctx._h))
        raw_call(ctx, stem, family, a, k, tol, outs)
        ctx.check(lib.rc_graph_end_capture(ctx._h, ctypes.byref(graph)))
        try:
            ctx.check(lib.rc_graph_launch(ctx._h, graph))
            ctx.synchronize()
            for v, w in zip(eager, outs):
                assert same_bits(v, w)
            ctx.get_health()  # whatever the non-finite predecessors raised
        finally:
            ctx.check(lib.rc_graph_destroy(ctx._h, graph))
            ctx.close()


def run_case(family, dtype, m, n, k, tol, plan, graph=False):
    op, stem, by_kind = FAMILIES[family]
    cplx = np.dtype(dtype).kind == "c"
    call, host_call, check = by_kind["c" if cplx else "f"]
    op = op + ("<complex>" if cplx else "")
    kk = min(k, m, n)
    h = torch.from_numpy(host_matrices(m, n, dtype, seed=1000 * m + n)).cuda()
    succ = h[len(KINDS):]

    # ---- the grid and the plan, from a one-matrix probe ---------------------------------------------------------------------------
    _, probe = batched_launch(lambda: call(succ[:1], k, tol))
    assert (probe["op"], probe["m"], probe["n"], probe["count"], probe["grid"]) == (op, m, n, 1, 1), probe
    assert probe["plan"] == plan, probe
    g = probe["slots"]
    assert g >= len(KINDS) * NSUCC, probe  # every (predecessor kind, successor) pair needs 32 workgroups
    count = 2 * g + g // 2 + 1

    # ---- the reference: each successor first on a fresh workgroup, checked against the oracle ------------------------------------------
    ref_host, lab = batched_launch(lambda: host_call(succ, k, tol))
    assert lab["grid"] == lab["count"] == NSUCC and lab["plan"] == plan, lab
    for i in range(NSUCC):
        check(succ[i].cpu().numpy(), tuple(x[i] for x in ref_host), kk, tol, dtype)
    ref = tuple(torch.from_numpy(x).cuda() for x in ref_host)
    alone = call(h[CLEAN], k, tol)

    # ---- the reuse batch -----------------------------------------------------------------------------------------------------------------
    src = sources(g, count).cuda()
    a = h[src]
    outs, lab = batched_launch(lambda: call(a, k, tol))
    torch.cuda.synchronize()
    print(f"{op} {np.dtype(dtype).name} {m}x{n} k={k} tol={tol}: {lab}")
    assert lab["op"] == op and lab["plan"] == plan, lab
    assert lab["grid"] == lab["slots"] == g and lab["count"] == count and count > 2 * lab["grid"], lab
    later = src[g:] - len(KINDS)
    for name, big, small in zip(range(len(outs)), outs, ref):
        assert same_bits(big[g:], small[later]), f"output {name}: a successor's bits depend on what its workgroup factored before"
    kind = src[:g]
    for j, kd in enumerate(CLEAN):
        sel = (kind == kd).nonzero().flatten()
        for name, big, small in zip(range(len(outs)), outs, alone):
            assert same_bits(big[sel], small[j:j + 1]), f"output {name}: predecessor kind {KINDS[kd]}"
    ranks = outs[-1][:g]
    assert bool(((ranks >= 0) & (ranks <= kk)).all())
    zero = (kind == KINDS.index("b")).nonzero().flatten()
    assert not bool(ranks[zero].any())
    for t in outs[:N_FACTORS[family]]:
        assert not bool(bits(t[zero]).any())

    if graph:
        graph_replay(stem, family, a, k, tol, outs)
    if family == "svd":
        # ---- the health word: drained, then clear after the same batch with clean predecessors only -----------------------------------
        ctx = _lib.default_context()
        ctx.synchronize()
        ctx.get_health()
        del a, outs
        clean = call(h[sources(g, count, clean_only=True).cuda()], k, tol)
        ctx.synchronize()
        assert ctx.get_health() == 0
        for big, small in zip(clean, ref):
            assert same_bits(big[g:], small[later])


# ---------------------------------------------------------------- column ID and two-sided ID: W in LDS / in the workspace slot
# (dtype, m, n, k, tol, plan): a tall and a wide shape on either side of the LDS boundary; tol = 0 with k = 3 (the rank of S3: a
# fixed-rank ID past the rank of its matrix has no oracle) or tolerance mode with k = 16
ID_CASES = [
    (F64, 203, 96, 3, 0.0, "W:lds"), (F64, 96, 201, 16, 1e-8, "W:lds"), (F64, 206, 96, 16, 1e-8, "W:ws"), (F64, 96, 202, 3, 0.0, "W:ws"),
    (F32, 307, 128, 3, 0.0, "W:lds"), (F32, 128, 305, 16, 1e-4, "W:lds"), (F32, 312, 128, 16, 1e-4, "W:ws"), (F32, 128, 307, 3, 0.0, "W:ws"),
    (C64, 153, 64, 3, 0.0, "W:lds"), (C64, 64, 152, 16, 1e-8, "W:lds"), (C64, 156, 64, 16, 1e-8, "W:ws"), (C64, 64, 153, 3, 0.0, "W:ws"),
    (C32, 207, 96, 3, 0.0, "W:lds"), (C32, 96, 205, 16, 1e-4, "W:lds"), (C32, 210, 96, 16, 1e-4, "W:ws"), (C32, 96, 206, 3, 0.0, "W:ws"),
]
GRAPH_ID = {(F64, 96, 201), (C64, 64, 152)}


def _id(case):
    return f"{np.dtype(case[0]).name}-{case[1]}x{case[2]}-k{case[3]}-{case[5]}"


@pytest.mark.parametrize("case", ID_CASES, ids=_id)
def test_column_id_successors_keep_their_bits(case):
    dtype, m, n, k, tol, plan = case
    run_case("column_id", dtype, m, n, k, tol, plan, graph=(dtype, m, n) in GRAPH_ID)


@pytest.mark.parametrize("case", ID_CASES, ids=_id)
def test_two_sided_id_successors_keep_their_bits(case):
    dtype, m, n, k, tol, plan = case
    run_case("two_sided_id", dtype, m, n, k, tol, plan, graph=(dtype, m, n) in GRAPH_ID)


# ---------------------------------------------------------------- batched SVD: every reachable plan (see the module docstring)
# tall shapes for every plan, a wide one for the all-LDS and the all-workspace plan, and N odd <= 16 (bsv_jacobi<T, 1> /
# bsc_jacobi<R, 1>, the dummy column of an odd N) at the all-LDS plan
SVD_CASES = [
    (F64, 96, 40, 20, 1e-8, "W:lds,V:lds,G:lds,ld=48"), (F64, 40, 13, 3, 0.0, "W:lds,V:lds,G:lds,ld=16"),
    (F64, 92, 79, 40, 1e-8, "W:lds,V:lds,G:lds,ld=79"), (F64, 200, 64, 32, 1e-8, "W:ws,V:lds,G:lds,ld=80"),
    (F64, 160, 96, 48, 1e-8, "W:ws,V:lds,G:lds,ld=97"), (F64, 200, 128, 64, 1e-8, "W:ws,V:ws,G:lds,ld=144"),
    (F64, 40, 96, 20, 1e-8, "W:lds,V:lds,G:lds,ld=48"), (F64, 128, 200, 64, 1e-8, "W:ws,V:ws,G:lds,ld=144"),
    (F32, 96, 40, 20, 1e-4, "W:lds,V:lds,G:lds,ld=48"), (F32, 40, 13, 3, 0.0, "W:lds,V:lds,G:lds,ld=16"),
    (F32, 118, 114, 56, 1e-4, "W:lds,V:lds,G:lds,ld=115"), (F32, 200, 128, 64, 1e-4, "W:ws,V:lds,G:lds,ld=144"),
    (F32, 40, 96, 20, 1e-4, "W:lds,V:lds,G:lds,ld=48"), (F32, 128, 200, 64, 1e-4, "W:ws,V:lds,G:lds,ld=144"),
    (C64, 96, 40, 20, 1e-8, "W:lds,V:lds,G:lds,ld=48"), (C64, 40, 13, 3, 0.0, "W:lds,V:lds,G:lds,ld=16"),
    (C64, 60, 56, 28, 1e-8, "W:lds,V:lds,G:lds,ld=57"), (C64, 200, 40, 20, 1e-8, "W:ws,V:lds,G:lds,ld=48"),
    (C64, 160, 64, 32, 1e-8, "W:ws,V:lds,G:lds,ld=65"), (C64, 160, 80, 40, 1e-8, "W:ws,V:ws,G:lds,ld=80"),
    (C64, 160, 96, 48, 1e-8, "W:ws,V:ws,G:lds,ld=97"), (C64, 160, 128, 64, 1e-8, "W:ws,V:ws,G:ws,ld=128"),
    (C64, 128, 128, 64, 1e-8, "W:ws,V:ws,G:ws,ld=128"), (C64, 40, 96, 20, 1e-8, "W:lds,V:lds,G:lds,ld=48"),
    (C64, 128, 200, 64, 1e-8, "W:ws,V:ws,G:ws,ld=128"),
    (C32, 96, 40, 20, 1e-4, "W:lds,V:lds,G:lds,ld=48"), (C32, 40, 13, 3, 0.0, "W:lds,V:lds,G:lds,ld=16"),
    (C32, 92, 79, 40, 1e-4, "W:lds,V:lds,G:lds,ld=79"), (C32, 200, 64, 32, 1e-4, "W:ws,V:lds,G:lds,ld=80"),
    (C32, 160, 96, 48, 1e-4, "W:ws,V:lds,G:lds,ld=97"), (C32, 200, 128, 64, 1e-4, "W:ws,V:ws,G:lds,ld=144"),
    (C32, 40, 96, 20, 1e-4, "W:lds,V:lds,G:lds,ld=48"), (C32, 128, 200, 64, 1e-4, "W:ws,V:ws,G:lds,ld=144"),
]
GRAPH_SVD = {(F64, 200, 64), (C64, 160, 80)}


@pytest.mark.parametrize("case", SVD_CASES, ids=_id)
def test_svd_successors_keep_their_bits(case):
    dtype, m, n, k, tol, plan = case
    run_case("svd", dtype, m, n, k, tol, plan, graph=(dtype, m, n) in GRAPH_SVD)
