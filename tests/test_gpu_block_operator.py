"""The block-sparse operator of a batch of low-rank and dense blocks in one launch (rc_block_operator_apply_*, batch.block_operator_apply,
operator.BlockLowRankOperator): y = H x with the gather of x, the batched apply and the scatter-add fused, for the reference's MatMat /
ConjMatMat (src/types.rs:40-101) on the outputs of the batched compressors.

Two yardsticks.  Bits: the contribution of a low-rank entry is what rc.lowrank_apply_batched writes for that block on the gathered
segment of x, and a group is the host sum acc = 0; acc = acc + c_e in the dtype of the call, then y_old + acc: np.array_equal.
Accuracy (derived, not measured): against NumPy in float64 / complex128, elementwise |y - y_ref| <= (n + 2K + 4 + t) c u E with E the
sum over the group's entries of |left| |mid| diag(|s|) |right| |x| (or |D| |x|) plus |y_old|, t = entries + 1, u the unit roundoff and
c = 1 for real, 4 for complex data: the bound of tests/test_gpu_batched_apply.py for one entry plus the t-term sum of the group."""
import ctypes

import numpy as np
import pytest
import torch

import rusty_compression_amd as rc
from rusty_compression_amd import _lib
from rusty_compression_amd.batch import _BlockOperatorCall
from tests.helpers import batched_launch, npy

pytestmark = pytest.mark.gpu

INVALID = 5
BAD_INDEX = 64
DTYPES = [np.float64, np.float32, np.complex128, np.complex64]
SHAPES = [(37, 29, 16, 1), (37, 29, 16, 5), (130, 70, 48, 3), (512, 33, 7, 17), (65, 512, 128, 1)]  # (m, n, K, nrhs)
MODES = ["none", "mid", "s"]


def is_complex(dtype):
    return np.iscomplexobj(np.zeros(0, dtype=dtype))


def real_of(dtype):
    return np.zeros(0, dtype=dtype).real.dtype


def unit_roundoff(dtype):
    return np.finfo(np.dtype(dtype)).eps / 2


def rand(rng, shape, dtype):
    x = rng.standard_normal(shape)
    if is_complex(dtype):
        x = x + 1j * rng.standard_normal(shape)
    return x.astype(dtype)


def dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def mixed_ranks(count, k):
    base = [k, 0, k // 2, 1, max(k - 1, 0), min(2, k), k // 3]
    return np.array([base[i % len(base)] for i in range(count)], dtype=np.int64)


def build(rng, dtype, m, n, k, nrhs, mode="none", count=5, dense_count=0, pattern=None, spare=7):
    """A case: factor batches, ranks (mixed, 0 included), dense blocks, a pattern [(group_row, [(block, entry_col), ...]), ...] and x.
    The default pattern has 4 groups of 3, 0, 4 and 2 entries, block 0 twice in one group and blocks in several groups, overlapping x
    ranges, and rows of y between and around the groups that belong to nobody."""
    N = 3 * n + spare
    if pattern is None:
        blocks = [[0, 1, 2], [], [3, 0, 4, 0], [1, 3]]
        if dense_count:
            blocks = [[0, count, 2], [count + dense_count - 1, count], [3, count + 1 if dense_count > 1 else count, 4, 0], []]
        pattern, row = [], 3
        for ids in blocks:
            pattern.append((row, [(b, int(rng.integers(0, N - n - spare + 1))) for b in ids]))
            row += m + 2
    M = max(r for r, _ in pattern) + m + 4
    c = dict(dtype=dtype, m=m, n=n, k=k, nrhs=nrhs, count=count, dense_count=dense_count, pattern=pattern, M=M, N=N)
    c["left"], c["right"] = rand(rng, (count, m, k), dtype), rand(rng, (count, k, n), dtype)
    c["mid"] = rand(rng, (count, k, k), dtype) if mode == "mid" else None
    c["s"] = (np.abs(rng.standard_normal((count, k + 3))) + 0.1).astype(real_of(dtype)) if mode == "s" else None  # read with stride k + 3
    c["ranks"] = mixed_ranks(count, k)
    c["dense"] = rand(rng, (dense_count, m, n), dtype) if dense_count else None
    c["x"] = rand(rng, (N, nrhs), dtype)
    c["y0"] = rand(rng, (M, nrhs), dtype)
    return c


def csr(pattern):
    ptr, rows, blocks, cols = [0], [], [], []
    for row, entries in pattern:
        rows.append(row)
        blocks += [b for b, _ in entries]
        cols += [col for _, col in entries]
        ptr.append(len(blocks))
    return tuple(np.array(v, dtype=np.int64) for v in (ptr, rows, blocks, cols))


def run(c, x=None, y0=None, accumulate=False, conj=False, pattern=None, **over):
    """batch.block_operator_apply on the case (operands replaceable by name, numpy or device tensors); returns y on the host."""
    ops = {name: over.get(name, c[name]) for name in ("left", "right", "mid", "s", "ranks", "dense")}
    ops = {name: dev(v) if isinstance(v, np.ndarray) else v for name, v in ops.items()}
    x = c["x"] if x is None else x
    y = dev(c["y0"] if y0 is None else y0) if not isinstance(y0, torch.Tensor) else y0
    out = rc.block_operator_apply(dev(x) if isinstance(x, np.ndarray) else x, *csr(c["pattern"] if pattern is None else pattern), y=y,
                                  accumulate=accumulate, conj=conj, **ops)
    torch.cuda.synchronize()
    assert out is y
    return npy(y)


def rows_outside(c, pattern=None):
    mask = np.ones(c["M"], dtype=bool)
    for row, _ in (c["pattern"] if pattern is None else pattern):
        mask[row:row + c["m"]] = False
    return mask


def host_sum(c, accumulate, x=None, y0=None, pattern=None, **over):
    """The contract's arithmetic on the host: per entry what rc.lowrank_apply_batched writes for the block on the gathered segment of
    x (one call for all entries), summed per group in list order in the dtype of the call; dense entries are not handled here."""
    pattern = c["pattern"] if pattern is None else pattern
    x = c["x"] if x is None else x
    y = (c["y0"] if y0 is None else y0).copy()
    entries = [(b, col) for _, es in pattern for b, col in es]
    ops = {name: over.get(name, c[name]) for name in ("left", "right", "mid", "s", "ranks")}
    ops = {name: dev(v) if isinstance(v, np.ndarray) else v for name, v in ops.items()}
    contrib = None
    if entries:
        ids = torch.tensor([b for b, _ in entries], dtype=torch.int64, device="cuda")
        b = dev(np.stack([x[col:col + c["n"]] for _, col in entries]))

        def pick(t):  # the entries' blocks, keeping the stride order of the views (the bits depend on it)
            if t is None or t.dim() != 3 or t.stride(1) >= t.stride(2):
                return None if t is None else t[ids]
            return t.transpose(1, 2)[ids].transpose(1, 2)

        contrib = npy(rc.lowrank_apply_batched(pick(ops["left"]), pick(ops["right"]), b=b, mid=pick(ops["mid"]), s=pick(ops["s"]),
                                               ranks=pick(ops["ranks"])))
    e = 0
    for row, es in pattern:
        acc = np.zeros((c["m"], x.shape[1]), dtype=c["dtype"])
        for _ in es:
            acc = acc + contrib[e]
            e += 1
        y[row:row + c["m"]] = y[row:row + c["m"]] + acc if accumulate else acc
    return y


def reference(c, accumulate, x=None, y0=None, pattern=None, conj=False):
    """(y_ref, E, t) in float64 / complex128 at the blocks' ranks; E and t (entries + 1) per row of y, zero outside the groups."""
    pattern = c["pattern"] if pattern is None else pattern
    wide = np.complex128 if is_complex(c["dtype"]) else np.float64
    x = (c["x"] if x is None else x).astype(wide)
    y0 = (c["y0"] if y0 is None else y0).astype(wide)
    cj = (lambda a: np.conj(a)) if conj else (lambda a: a)
    y, e_all, t_all = y0.copy(), np.zeros(y0.shape), np.zeros(y0.shape[0])
    for row, es in pattern:
        acc, e_acc = np.zeros((c["m"], x.shape[1]), dtype=wide), np.zeros((c["m"], x.shape[1]))
        for blk, col in es:
            xb = x[col:col + c["n"]]
            if blk >= c["count"]:
                d = cj(c["dense"][blk - c["count"]].astype(wide))
                acc, e_acc = acc + d @ xb, e_acc + np.abs(d) @ np.abs(xb)
                continue
            r = int(np.clip(c["ranks"][blk], 0, c["k"]))
            w, ew = cj(c["right"][blk, :r].astype(wide)) @ xb, np.abs(c["right"][blk, :r]).astype(np.float64) @ np.abs(xb)
            if c["s"] is not None:
                sv = c["s"][blk, :r].astype(np.float64)[:, None]
                w, ew = sv * w, np.abs(sv) * ew
            if c["mid"] is not None:
                mw = cj(c["mid"][blk, :r, :r].astype(wide))
                w, ew = mw @ w, np.abs(mw) @ ew
            lw = cj(c["left"][blk, :, :r].astype(wide))
            acc, e_acc = acc + lw @ w, e_acc + np.abs(lw) @ ew
        sl = slice(row, row + c["m"])
        y[sl] = y0[sl] + acc if accumulate else acc
        e_all[sl] = e_acc + (np.abs(y0[sl]) if accumulate else 0.0)
        t_all[sl] = len(es) + 1
    return y, e_all, t_all


def check_bound(y, c, accumulate, n_inner=None, **kw):
    ref, e, t = reference(c, accumulate, **kw)
    cc = 4 if is_complex(c["dtype"]) else 1
    bnd = ((c["n"] if n_inner is None else n_inner) + 2 * c["k"] + 4 + t)[:, None] * cc * unit_roundoff(c["dtype"]) * e
    err = np.abs(y.astype(ref.dtype) - ref)
    worst = float((err / np.maximum(bnd, np.finfo(np.float64).tiny)).max())
    print(f"max |y - y_ref| / bound = {worst:.3e}")
    assert np.all(np.isfinite(y))
    assert np.all(err <= bnd), worst


# ---------------------------------------------------------------- 1. bits against the apply
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("m,n,k,nrhs", SHAPES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_bits_against_the_batched_apply(dtype, m, n, k, nrhs, mode):
    rng = np.random.default_rng(m * 7 + n * 3 + k + nrhs + MODES.index(mode))
    c = build(rng, dtype, m, n, k, nrhs, mode)
    assert 0 in c["ranks"] and len(c["pattern"]) == 4 and [len(es) for _, es in c["pattern"]] == [3, 0, 4, 2]
    outside = rows_outside(c)
    assert outside.any()
    for accumulate in (False, True):
        y = run(c, accumulate=accumulate)
        assert np.array_equal(y, host_sum(c, accumulate))
        assert np.array_equal(y[outside], c["y0"][outside])  # rows of no group keep their values
        check_bound(y, c, accumulate)
    row = c["pattern"][1][0]  # the empty group: zeros, or y_old when accumulating
    assert not np.any(run(c)[row:row + m]) and np.array_equal(run(c, accumulate=True)[row:row + m], c["y0"][row:row + m])


# ---------------------------------------------------------------- 2. dense entries
@pytest.mark.parametrize("mode", ["none", "mid"])
@pytest.mark.parametrize("m,n,k,nrhs", [(37, 29, 16, 5), (130, 70, 48, 3), (512, 33, 7, 17), (65, 512, 128, 1)])
@pytest.mark.parametrize("dtype", DTYPES)
def test_dense_entries_alone_and_mixed_with_low_rank_entries(dtype, m, n, k, nrhs, mode):
    rng = np.random.default_rng(m + n + k + nrhs)
    c = build(rng, dtype, m, n, k, nrhs, mode, dense_count=3)
    kinds = [{b >= c["count"] for b, _ in es} for _, es in c["pattern"]]
    assert {True} in kinds and {True, False} in kinds  # a group of dense entries only, and groups that mix both kinds
    for accumulate in (False, True):
        check_bound(run(c, accumulate=accumulate), c, accumulate)
    # dense blocks alone, without a low-rank batch; for n <= 128 bit-equal to the low-rank entry left = D, right = I_n
    only = [(row, [(b - c["count"], col) for b, col in es if b >= c["count"]]) for row, es in c["pattern"]]
    y = rc.block_operator_apply(dev(c["x"]), *csr(only), dense=dev(c["dense"]), y=dev(c["y0"]), accumulate=True)
    d = dict(c, count=0, pattern=only, k=0)
    check_bound(npy(y), d, True)
    if n <= 128:
        eye = torch.eye(n, dtype=dev(c["dense"]).dtype, device="cuda").expand(3, n, n)
        as_lowrank = rc.block_operator_apply(dev(c["x"]), *csr(only), left=dev(c["dense"]), right=eye, y=dev(c["y0"]), accumulate=True)
        assert np.array_equal(npy(y), npy(as_lowrank))


# ---------------------------------------------------------------- 3. the LDS corner
@pytest.mark.parametrize("dtype", [np.float64, np.complex128])
def test_lds_corner_steps_the_tile_down(dtype):
    m, n, k, nrhs = 512, 512, 128, 16
    rng = np.random.default_rng(3)
    pattern = [(0, [(0, 5), (1, 0)]), (m, [(2, 7), (0, 3)])]
    c = build(rng, dtype, m, n, k, nrhs, "mid", count=3, pattern=pattern)
    c["ranks"] = np.array([k, k - 1, k // 2], dtype=np.int64)
    y, lab = batched_launch(lambda: run(c))
    assert lab["op"].startswith("batched_operator_apply") and (lab["m"], lab["n"], lab["k"], lab["count"]) == (m, n, k, 2)
    plan = dict(f.split(":") for f in lab["plan"].split(",") if ":" in f)
    widest = 8 if is_complex(dtype) else 16  # the apply's tile for 16 columns, which does not fit beside the accumulator here
    assert int(plan["nb"]) == widest // 2 and int(plan["cols"]) == nrhs and int(plan["tiles"]) == nrhs // (widest // 2)
    assert "mid" in lab["plan"].split(",")
    for col in range(nrhs):  # the bits of a column do not depend on the tile it travels in
        alone = run(c, x=c["x"][:, col:col + 1], y0=c["y0"][:, col:col + 1])
        assert np.array_equal(alone[:, 0], y[:, col]), col
    check_bound(y, c, False)


# ---------------------------------------------------------------- 4. rank-aware reads
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_tails_and_unreferenced_rows_of_x_are_never_read(dtype, mode):
    m, n, k, nrhs = 130, 70, 48, 5
    rng = np.random.default_rng(4)
    c = build(rng, dtype, m, n, k, nrhs, mode, dense_count=2)
    clean = run(c, accumulate=True)
    dirty = {name: None if c[name] is None else c[name].copy() for name in ("left", "right", "mid", "s")}
    for i, r in enumerate(c["ranks"]):
        dirty["left"][i, :, r:] = np.nan
        dirty["right"][i, r:, :] = np.nan
        if dirty["mid"] is not None:
            dirty["mid"][i, r:, :] = np.nan
            dirty["mid"][i, :, r:] = np.nan
        if dirty["s"] is not None:
            dirty["s"][i, r:] = np.nan
    x = c["x"].copy()
    read = np.zeros(c["N"], dtype=bool)
    for _, es in c["pattern"]:
        for _, col in es:
            read[col:col + n] = True
    assert not read.all()
    x[~read] = np.nan
    got = run(c, x=x, accumulate=True, **dirty)
    assert np.all(np.isfinite(got)) and np.array_equal(got, clean)


# ---------------------------------------------------------------- 5. invariances, bit for bit
@pytest.mark.parametrize("dtype", [np.float64, np.complex64])
def test_a_group_alone_and_among_more_groups_than_slots(dtype):
    m, n, k, nrhs = 24, 29, 16, 5
    rng = np.random.default_rng(5)
    c = build(rng, dtype, m, n, k, nrhs, "mid", dense_count=1)
    group = [(0, 4), (5, 11), (2, 0), (0, 9)]  # low-rank, dense, low-rank, the first block again
    alone, probe = batched_launch(lambda: run(c, pattern=[(0, group)], y0=c["y0"][:m]))
    assert probe["count"] == 1 and probe["grid"] == 1
    groups = probe["slots"] + 3
    pattern = [(g * m, [(int(b), int(col)) for b, col in zip(rng.integers(0, 6, 2), rng.integers(0, c["N"] - n + 1, 2))]) for g in range(groups)]
    pattern[0], pattern[-1] = (0, group), ((groups - 1) * m, group)
    y0 = rand(rng, (groups * m, nrhs), dtype)
    y, lab = batched_launch(lambda: run(c, pattern=pattern, y0=y0))
    assert lab["count"] == groups and lab["grid"] == lab["slots"] < groups  # some workgroups take a second unit
    assert np.array_equal(y[:m], alone) and np.array_equal(y[-m:], alone)
    big = dict(c, pattern=pattern, M=groups * m, y0=y0)
    check_bound(y, big, False)


@pytest.mark.parametrize("dtype", [np.float64, np.complex64])
def test_padded_and_column_major_views(dtype):
    m, n, k, nrhs = 37, 29, 16, 5
    rng = np.random.default_rng(6)
    c = build(rng, dtype, m, n, k, nrhs, "mid", dense_count=2)
    base = run(c, accumulate=True)

    def padded(a):  # the same values inside a larger allocation: same stride order, other strides, spare space all around
        if a is None or a.ndim != 3:
            return a
        big = torch.full((a.shape[0] + 2, a.shape[1] + 3, a.shape[2] + 5), float("nan"), dtype=dev(a).dtype, device="cuda")
        big[1:-1, 2:-1, 1:-4] = dev(a)
        return big[1:-1, 2:-1, 1:-4]

    def padded2(a):
        big = torch.full((a.shape[0] + 6, a.shape[1] + 3), float("nan"), dtype=dev(a).dtype, device="cuda")
        big[4:-2, 1:-2] = dev(a)
        return big[4:-2, 1:-2]

    ops = {name: padded(c[name]) for name in ("left", "right", "mid", "dense")}
    yp = padded2(c["y0"])
    out = rc.block_operator_apply(padded2(c["x"]), *csr(c["pattern"]), y=yp, accumulate=True, ranks=dev(c["ranks"]), **ops)
    assert out is yp and np.array_equal(npy(yp), base)
    assert torch.isnan(yp._base).sum().item() == yp._base.numel() - yp.numel()  # nothing outside the view was written
    # x and y column-major: the loads and the store change, no sum does
    xt, yt = dev(c["x"]).t().contiguous().t(), dev(c["y0"]).t().contiguous().t()
    assert xt.stride() == (1, c["N"])
    assert np.array_equal(run(c, x=xt, y0=yt, accumulate=True), base)
    # column-major factors change which index is the fast one, hence the order of the sums: the bits are the apply's on the same views
    cm = lambda a: None if a is None else dev(a).transpose(1, 2).contiguous().transpose(1, 2)  # noqa: E731
    low = dict(c, dense=None, dense_count=0, pattern=[(row, [(b, col) for b, col in es if b < c["count"]]) for row, es in c["pattern"]])
    views = {name: cm(c[name]) for name in ("left", "right", "mid")}
    got = run(low, accumulate=True, **views)
    assert np.array_equal(got, host_sum(low, True, **views))
    check_bound(got, low, True)
    got = run(c, accumulate=True, dense=cm(c["dense"]), **views)
    check_bound(got, c, True)


def test_a_shared_factor_and_the_number_of_right_hand_sides():
    m, n, k = 37, 29, 16
    rng = np.random.default_rng(7)
    c = build(rng, np.float64, m, n, k, 17, "s")
    shared = dev(c["left"][2:3]).expand(c["count"], m, k)
    assert shared.stride(0) == 0
    copies = np.repeat(c["left"][2:3], c["count"], axis=0)
    assert np.array_equal(run(c, left=shared), run(c, left=copies))
    y17 = run(c)
    y5 = run(c, x=c["x"][:, 3:8], y0=c["y0"][:, 3:8])
    y1 = run(c, x=c["x"][:, 16:17], y0=c["y0"][:, 16:17])
    assert np.array_equal(y5, y17[:, 3:8]) and np.array_equal(y1, y17[:, 16:17])
    v = rc.block_operator_apply(dev(c["x"][:, 16]), *csr(c["pattern"]), left=dev(c["left"]), right=dev(c["right"]), s=dev(c["s"]),
                                ranks=dev(c["ranks"]), rows=c["M"])  # a vector, into a zero-filled result
    outside = rows_outside(c)
    assert v.shape == (c["M"],) and np.array_equal(npy(v)[~outside], y17[~outside, 16]) and not np.any(npy(v)[outside])


def test_graph_capture_replays_the_eager_bits():
    m, n, k, nrhs = 96, 128, 24, 5
    rng = np.random.default_rng(8)
    c = build(rng, np.float64, m, n, k, nrhs, "mid", dense_count=2)
    lib = _lib.lib()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        eager = run(c, accumulate=True)
        call = _BlockOperatorCall("test", csr(c["pattern"]), dev(c["left"]), dev(c["right"]), dev(c["mid"]), None, dev(c["ranks"]), dev(c["dense"]))
        x, y = dev(c["x"]), dev(c["y0"])
        ctx = _lib.Context(torch.cuda.current_device(), st.cuda_stream)
        st.synchronize()
        graph = ctypes.c_void_p(None)
        ctx.check(lib.rc_graph_begin_capture(ctx._h))
        assert getattr(lib, call.name)(ctx._h, *call.args(_lib.mat(x), _lib.mat(y), True, False)) == 0
        ctx.check(lib.rc_graph_end_capture(ctx._h, ctypes.byref(graph)))
        try:
            st.synchronize()
            assert np.array_equal(npy(y), c["y0"])  # captured, not run
            ctx.check(lib.rc_graph_launch(ctx._h, graph))
            ctx.synchronize()
            assert np.array_equal(npy(y), eager)
        finally:
            ctx.check(lib.rc_graph_destroy(ctx._h, graph))
            ctx.close()


# ---------------------------------------------------------------- 6. conj
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_conj_flag(dtype, mode):
    m, n, k, nrhs = 37, 29, 16, 5
    rng = np.random.default_rng(9)
    c = build(rng, dtype, m, n, k, nrhs, mode, dense_count=2)
    got = run(c, accumulate=True, conj=True)
    if is_complex(dtype):
        copies = {name: None if c[name] is None else np.conj(c[name]) for name in ("left", "right", "mid", "dense")}
        assert np.array_equal(got, run(c, accumulate=True, **copies))
        assert not np.array_equal(got, run(c, accumulate=True))
        check_bound(got, c, True, conj=True)
    else:
        assert np.array_equal(got, run(c, accumulate=True))  # real data: the flag changes nothing


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dtype", [np.complex128, np.complex64, np.float64])
def test_swapped_views_with_conj_are_the_adjoint(dtype, mode):
    """A^H z: the pattern grouped by column (block_csr's twin), left = right^T, right = left^T, mid^T and dense^T as strided views, conj."""
    m, n, k, nrhs = 40, 32, 12, 3
    rng = np.random.default_rng(10)
    br, bc = 3, 4
    count = br * bc - 2
    c = build(rng, dtype, m, n, k, nrhs, mode, count=count, dense_count=2, pattern=[(0, [])])
    rows, cols = np.repeat(np.arange(br) * m, bc), np.tile(np.arange(bc) * n, br)
    ids = rng.permutation(br * bc)  # ids count and count + 1 are the dense blocks
    by_row, by_col = rc.block_csr(rows, cols, ids)
    z = rand(rng, (br * m, nrhs), dtype)
    t = lambda a: None if a is None else dev(a).transpose(1, 2)  # noqa: E731
    out = rc.block_operator_apply(dev(z), *by_col, left=t(c["right"]), right=t(c["left"]), mid=t(c["mid"]), s=dev(c["s"]), ranks=dev(c["ranks"]),
                                  dense=t(c["dense"]), rows=bc * n, conj=True)
    fwd = dict(c, M=br * m, N=bc * n, y0=np.zeros((br * m, bc * n), dtype=dtype),
               pattern=[(int(by_row[1][g]), [(int(by_row[2][e]), int(by_row[3][e])) for e in range(by_row[0][g], by_row[0][g + 1])]) for g in range(br)])
    wide = np.complex128 if is_complex(dtype) else np.float64
    a, ea, _ = reference(fwd, False, x=np.eye(bc * n, dtype=dtype))  # the dense matrix and |left| |mid| |s| |right| per block
    ref, e = a.conj().T @ z.astype(wide), ea.T @ np.abs(z).astype(np.float64)
    cc = 4 if is_complex(dtype) else 1
    bnd = (m + 2 * k + 4 + br + 1) * cc * unit_roundoff(dtype) * e  # the chain's inner sizes are m, K, K here, br entries per group
    assert np.all(np.abs(npy(out).astype(wide) - ref) <= bnd)


# ---------------------------------------------------------------- 7. index guards
@pytest.mark.parametrize("bad", ["col_past_the_end", "col_negative", "block_past_the_end", "group_row_past_the_end"])
@pytest.mark.parametrize("dtype", [np.float64, np.complex64])
def test_out_of_range_indices_are_skipped_and_flagged(dtype, bad):
    m, n, k, nrhs = 37, 29, 16, 5
    rng = np.random.default_rng(11)
    c = build(rng, dtype, m, n, k, nrhs, "mid", dense_count=2)
    # every operand is a view with spare rows / one spare block in front of it and behind it: a missing guard reads or writes
    # finite sentinels inside an allocation and shows up as a wrong value below
    def inside(a, fill):
        if a is None:
            return None
        pad = (1,) + (0,) * (a.ndim - 1) if a.ndim == 3 else (2 * max(m, n),) + (0,) * (a.ndim - 1)
        big = torch.full(tuple(s + 2 * p for s, p in zip(a.shape, pad)), fill, dtype=dev(a).dtype, device="cuda")
        view = big[tuple(slice(p, p + s) for s, p in zip(a.shape, pad))]
        view.copy_(dev(a))
        return view

    ops = {name: inside(c[name], 3.0) for name in ("left", "right", "mid", "dense")}
    ctx = _lib.default_context()

    def call(pattern):
        y = inside(c["y0"], -5.0)
        rc.block_operator_apply(inside(c["x"], 9.0), *csr(pattern), y=y, ranks=dev(c["ranks"]), **ops)
        torch.cuda.synchronize()
        assert torch.all(y._base[:2 * max(m, n)] == -5.0) and torch.all(y._base[-2 * max(m, n):] == -5.0)  # nothing outside the view
        return npy(y), ctx.get_health()

    ctx.get_health()  # cleared: whatever an earlier test left behind is not this test's business
    clean, health = call(c["pattern"])
    assert health == 0
    pattern = [(row, list(es)) for row, es in c["pattern"]]
    g, e = 2, 1  # the second entry of the third group
    expect = [(row, list(es)) for row, es in c["pattern"]]
    if bad == "group_row_past_the_end":
        pattern[g] = (c["M"] - m + 1, pattern[g][1])
        del expect[g]
    else:
        blk, col = pattern[g][1][e]
        pattern[g][1][e] = {"col_past_the_end": (blk, c["N"] - n + 1), "col_negative": (blk, -1),
                            "block_past_the_end": (c["count"] + c["dense_count"], col)}[bad]
        del expect[g][1][e]
    got, health = call(pattern)
    assert health & BAD_INDEX and health & ~BAD_INDEX == 0
    want, health = call(expect)  # the same call without the offending entry / group
    assert health == 0
    assert np.array_equal(got, want)
    for gg, (row, _) in enumerate(c["pattern"]):
        if gg != g:
            assert np.array_equal(got[row:row + m], clean[row:row + m])  # every other group is untouched by the bad index
    if bad == "group_row_past_the_end":
        assert np.array_equal(got[c["pattern"][g][0]:c["pattern"][g][0] + m], c["y0"][c["pattern"][g][0]:c["pattern"][g][0] + m])
    assert ctx.get_health() == 0  # read and cleared


# ---------------------------------------------------------------- 8. arguments
def test_argument_checks():
    m, n, k, nrhs, count, dcount, groups = 40, 30, 16, 3, 2, 2, 2
    M, N = 2 * m, 2 * n
    z = lambda *shape: torch.zeros(shape, dtype=torch.float64, device="cuda")  # noqa: E731
    idx = lambda *v: torch.tensor(v, dtype=torch.int64, device="cuda")  # noqa: E731
    keep = dict(left=z(count, m, k), right=z(count, k, n), mid=z(count, k, k), dense=z(dcount, m, n), x=torch.ones((N, nrhs), dtype=torch.float64, device="cuda"),
                ptr=idx(0, 2, 3), row=idx(0, m), blk=idx(0, 2, 1), col=idx(0, n, 5), ranks=idx(k, k))
    sentinel = torch.full((M, nrhs), 7.0, dtype=torch.float64, device="cuda")
    fn = _lib.lib().rc_block_operator_apply_f64
    ctx = _lib.default_context()
    none = _lib.mat(None)

    def call(**over):
        a = dict(keep, y=sentinel, count=count, dense_count=dcount, groups=groups, accumulate=0)
        a.update(over)

        def view(t):
            if t is None:
                return none, ctypes.c_int64(0)
            if isinstance(t, _lib.rc_matrix):
                return t, ctypes.c_int64(t.rows * t.cols)
            return _lib.rc_matrix(t.data_ptr(), t.shape[1], t.shape[2], t.stride(1), t.stride(2)), ctypes.c_int64(t.stride(0))

        mat = lambda t: t if isinstance(t, _lib.rc_matrix) else _lib.mat(t)  # noqa: E731
        return fn(ctx._h, *view(a["left"]), *view(a["mid"]), None, ctypes.c_int64(0), *view(a["right"]), _lib.i64p(a["ranks"]), ctypes.c_int32(a["count"]),
                  *view(a["dense"]), ctypes.c_int32(a["dense_count"]), _lib.i64p(a["ptr"]), _lib.i64p(a["row"]), ctypes.c_int32(a["groups"]),
                  _lib.i64p(a["blk"]), _lib.i64p(a["col"]), mat(a["x"]), mat(a["y"]), ctypes.c_int32(a["accumulate"]), ctypes.c_int32(0))

    assert call(y=z(M, nrhs)) == 0                                                  # the valid call
    assert call(right=z(count, k + 1, n)) == INVALID                                # left.cols != right.rows
    assert "right" in _lib.lib().rc_last_error_message(ctx._h).decode()
    assert call(mid=z(count, k, k + 1)) == INVALID                                  # mid not K x K
    assert call(dense=z(dcount, m + 1, n)) == INVALID                               # dense does not agree with left / right
    assert call(dense=z(dcount, m, n - 1)) == INVALID
    assert call(x=z(N, nrhs + 1)) == INVALID                                        # x.cols != y.cols
    assert call(x=_lib.rc_matrix(keep["x"].data_ptr(), N, 0, 1, 1), y=_lib.rc_matrix(sentinel.data_ptr(), M, 0, 1, 1)) == INVALID  # nrhs = 0
    assert call(left=z(count, m, 129), right=z(count, 129, n), mid=None) == INVALID  # K = 129
    assert call(left=z(count, 513, k), dense=None) == INVALID                       # m = 513
    assert call(right=z(count, k, 513), dense=None) == INVALID                      # n = 513
    assert call(left=None, right=None, mid=None, ranks=None, count=0, dense=z(dcount, 513, n)) == INVALID  # the dense shape sets the domain then
    assert call(count=-1) == INVALID
    assert call(dense_count=-1) == INVALID
    assert call(groups=-1) == INVALID
    assert call(left=_lib.rc_matrix(None, m, k, k, 1)) == INVALID                   # null pointers
    assert call(right=_lib.rc_matrix(None, k, n, n, 1)) == INVALID
    for name in ("ptr", "row", "blk", "col"):
        assert call(**{name: None}) == INVALID, name
    assert call(x=_lib.rc_matrix(None, N, nrhs, nrhs, 1)) == INVALID
    assert call(y=_lib.rc_matrix(None, M, nrhs, nrhs, 1)) == INVALID
    assert call(left=None, right=None, mid=None, ranks=None, count=0, dense=None) == INVALID  # no blocks at all: the shape is unknown
    assert call(groups=0) == 0                                                      # nothing to do
    assert call(groups=0, left=None, right=None, mid=None, ranks=None, count=0, dense=None) == 0
    torch.cuda.synchronize()
    assert torch.all(sentinel == 7.0)  # no rejected call, and not the empty ones, wrote anything
    assert call(ptr=idx(0, 0, 0), accumulate=1) == 0  # no entries, accumulating: y_old stays
    torch.cuda.synchronize()
    assert torch.all(sentinel == 7.0)
    assert call(ptr=idx(0, 0, 0), row=idx(m, 0)[:1], groups=1) == 0  # no entries: the one group's rows become zero
    torch.cuda.synchronize()
    assert torch.all(sentinel[m:] == 0.0) and torch.all(sentinel[:m] == 7.0)
    assert ctx.get_health() == 0
    with pytest.raises(AssertionError, match="block_operator_apply"):  # RC_INVALID_ARGUMENT: the reference asserts
        rc.block_operator_apply(z(20, 1), idx(0, 1), idx(0), idx(0), idx(0), left=z(1, 600, 8), right=z(1, 8, 20), rows=600)
    with pytest.raises(TypeError):
        rc.block_operator_apply(z(20, 1), idx(0, 1), idx(0), idx(0), idx(0), left=z(1, 30, 8), right=z(1, 8, 20).float(), rows=30)
    with pytest.raises(AssertionError, match="mid and s"):
        rc.BlockLowRankOperator((30, 20), [0], [0], [0], left=z(1, 30, 8), right=z(1, 8, 20), mid=z(1, 8, 8), s=torch.ones((1, 8), dtype=torch.float64, device="cuda"))


# ---------------------------------------------------------------- 9. non-finite containment
@pytest.mark.parametrize("dtype", [np.float64, np.complex64])
def test_a_nan_stays_inside_the_groups_that_reference_its_block(dtype):
    m, n, k, nrhs = 37, 29, 16, 5
    rng = np.random.default_rng(12)
    c = build(rng, dtype, m, n, k, nrhs, "mid", dense_count=2)
    clean = run(c)
    for blk in (3, c["count"]):  # a low-rank block (groups 2 and 3), a dense block (groups 0 and 1)
        name = "left" if blk < c["count"] else "dense"
        bad = c[name].copy()
        bad[blk if blk < c["count"] else 0, 1, 0] = np.nan
        got = run(c, **{name: bad})
        for row, es in c["pattern"]:
            if any(b == blk for b, _ in es):
                assert np.isnan(got[row:row + m]).any()
            else:
                assert np.array_equal(got[row:row + m], clean[row:row + m])


# ---------------------------------------------------------------- 10. the operator
def tiled_rank6(rng, dtype):
    """A = U V^T of rank 6 cut into 4 x 3 tiles of 40 x 32: tile (i, j) is U_i V_j^T exactly, so the factors need no compressor."""
    br, bc, m, n, r = 4, 3, 40, 32, 6
    u, v = rand(rng, (br * m, r), dtype), rand(rng, (r, bc * n), dtype)
    left = np.stack([u[i * m:(i + 1) * m] for i in range(br) for _ in range(bc)])
    right = np.stack([v[:, j * n:(j + 1) * n] for _ in range(br) for j in range(bc)])
    rows, cols = np.repeat(np.arange(br) * m, bc), np.tile(np.arange(bc) * n, br)
    wide = np.complex128 if is_complex(dtype) else np.float64
    return u.astype(wide) @ v.astype(wide), np.abs(u).astype(np.float64) @ np.abs(v).astype(np.float64), left, right, rows, cols, (m, n, r, br, bc)


@pytest.mark.parametrize("dtype", [np.float64, np.float32, np.complex128])
def test_block_low_rank_operator_products(dtype):
    rng = np.random.default_rng(13)
    a, ea, left, right, rows, cols, (m, n, r, br, bc) = tiled_rank6(rng, dtype)
    op = rc.BlockLowRankOperator(a.shape, rows, cols, np.arange(br * bc), left=dev(left), right=dev(right))
    assert op.shape == a.shape and op.dtype == dev(left).dtype
    cc, u = (4 if is_complex(dtype) else 1), unit_roundoff(dtype)
    x, z = rand(rng, (a.shape[1], 5), dtype), rand(rng, (a.shape[0], 5), dtype)
    y = npy(op.matmat(dev(x)))
    assert np.all(np.abs(y - a @ x.astype(a.dtype)) <= (n + 2 * r + 4 + bc + 1) * cc * u * (ea @ np.abs(x)))
    w = npy(op.conj_matmat(dev(z)))
    assert np.all(np.abs(w - a.conj().T @ z.astype(a.dtype)) <= (m + 2 * r + 4 + br + 1) * cc * u * (ea.T @ np.abs(z)))
    # the raw forms on the library's own views, as the callback table calls them: uncovered rows are zero rows of the operator
    part = rc.BlockLowRankOperator(a.shape, rows[bc:], cols[bc:], np.arange(bc, br * bc), left=dev(left), right=dev(right))
    out = torch.full((a.shape[0], 5), 3.0, dtype=dev(x).dtype, device="cuda")
    assert part.matmat_raw(_lib.default_context()._h.value, _lib.mat(dev(x)), _lib.mat(out)) == 0
    torch.cuda.synchronize()
    assert not np.any(npy(out)[:m]) and np.array_equal(npy(out)[m:], y[m:])


def test_block_low_rank_operator_feeds_the_range_finder():
    rng = np.random.default_rng(14)
    a, _, left, right, rows, cols, (_, _, _, br, bc) = tiled_rank6(rng, np.float64)
    op = rc.BlockLowRankOperator(a.shape, rows, cols, np.arange(br * bc), left=dev(left), right=dev(right))
    q = npy(rc.sample_range_by_rank(op, 6, 4, rng.standard_normal((a.shape[1], 10))))  # through the callback table
    assert q.shape == (a.shape[0], 6)
    assert np.linalg.norm(a - q @ (q.conj().T @ a)) <= 1e-10 * np.linalg.norm(a)  # the project's f64 factor tolerance
