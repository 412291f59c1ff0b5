"""The multi-lane batch column ID (rc_batch_column_id_{f64,f32,c64,c32}) on every schedule and shape class: the optimistic pass with
all matrices verified, with some redone, with a flush in the middle; count against the lane count; the shapes the lone call takes off the
truncated blocked factorization; input layouts; the complex twins.

Every slot of every batch is held (a) to the oracle by tests/batch_lane_cases.check_slot and (b) bit for bit to rc_column_id_rank_* of the
same matrix, which is what the header promises; the health word of the default context and of every lane is 0 after each case.  The
cases and why the inputs do what the tests rely on: tests/batch_lane_cases.py, tests/test_batch_lane_cases_cpu.py."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from rusty_compression_amd import _lib, batch
from tests import batch_lane_cases as bl
from tests.helpers import TOL, npy, rel

pytestmark = pytest.mark.gpu

REAL = list(bl.REAL)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def lane_contexts(lanes):
    return batch._LanePool.get(torch.cuda.current_device(), lanes)


def run_batch(mats, k, lanes, ctxs=None, packed=None):
    """rc_batch_column_id_* through the C ABI on exactly `lanes` contexts (batch.batch_column_id_packed never takes more lanes than
    matrices).  mats: device tensors, any strides.  Returns (status, packed)."""
    ctxs = ctxs or lane_contexts(lanes)
    assert len(ctxs) == lanes
    m, n = mats[0].shape
    per = batch.packed_bytes(m, n, k, mats[0].element_size())
    if packed is None:
        packed = torch.empty(len(mats) * per, dtype=torch.uint8, device="cuda")
    arr = (ctypes.c_void_p * lanes)(*[c._h.value for c in ctxs])
    marr = (_lib.rc_matrix * max(len(mats), 1))(*[_lib.mat(a) for a in mats])
    torch.cuda.synchronize()  # the inputs were made on torch's stream, the lanes have their own
    fn = getattr(_lib.lib(), f"rc_batch_column_id_{_lib.suffix(mats[0].dtype)}")
    fn.restype = ctypes.c_int32
    st = fn(arr, ctypes.c_int32(lanes), marr, ctypes.c_int32(len(mats)), ctypes.c_int64(k), ctypes.c_void_p(packed.data_ptr()))
    return st, packed


def slots_of(mats, k, lanes):
    st, packed = run_batch(mats, k, lanes)
    assert st == _lib.RC_OK, _lib.lib().rc_last_error_message(lane_contexts(lanes)[0]._h)
    m, n = mats[0].shape
    return batch.unpack_factors(packed, len(mats), m, n, k, mats[0].dtype)


def assert_healthy(lanes):
    assert _lib.default_context().get_health() == 0
    for i, c in enumerate(lane_contexts(lanes)):
        assert c.get_health() == 0, f"lane {i}"


def check_all(hosts, mats, k, lanes, oracle_on=None):
    """Run the batch and hold EVERY slot to the lone call bit for bit; the oracle checker on every slot too, or on the slots listed."""
    out = slots_of(mats, k, lanes)
    assert len(out) == len(mats)
    for i, ((c, z, ind), a) in enumerate(zip(out, mats)):
        c1, z1, i1 = batch.column_id_rank(a, k)
        assert torch.equal(ind, i1), f"slot {i}: permutation differs from the lone call's"
        assert torch.equal(c, c1) and torch.equal(z, z1), f"slot {i}: factors differ from the lone call's"
    other = []  # slots that broke a near tie the other way than f64 LAPACK: held to the f64 ID of their own pivots (check_slot)
    for i in (range(len(mats)) if oracle_on is None else oracle_on):
        c, z, ind = out[i]
        if not bl.check_slot(npy(c), npy(z), npy(ind), hosts[i], k):
            other.append(i)
    print(f"{hosts[0].dtype} {hosts[0].shape} k={k} lanes={lanes}: {len(other)} of {len(mats)} slots with other near-tied pivots than the oracle's {other}")
    assert_healthy(lanes)
    return out


def dev(hosts):
    return [torch.from_numpy(np.array(a)).cuda() for a in hosts]


# ---------------------------------------------------------------- A: every matrix verified; count against the lane count
@pytest.mark.parametrize("dtype", REAL)
@pytest.mark.parametrize("count,lanes", bl.A_SCHEDULES)
def test_a_all_verified_for_every_count_and_lane_count(count, lanes, dtype):
    hosts = bl.case_a(dtype, count)
    check_all(hosts, dev(hosts), bl.A_SHAPE[2], lanes)


@pytest.mark.parametrize("dtype", REAL)
def test_a_count_zero_returns_an_empty_result(dtype):
    tdt = torch.from_numpy(np.zeros(1, dtype=dtype)).dtype
    assert batch.batch_column_id([], 40) == [] and batch.batch_column_id_packed([], 40).numel() == 0
    a = dev(bl.case_a(dtype, 1))[0]
    packed = torch.full((64,), 0xA5, dtype=torch.uint8, device="cuda")
    ctxs = lane_contexts(2)
    arr = (ctypes.c_void_p * 2)(*[c._h.value for c in ctxs])
    marr = (_lib.rc_matrix * 1)(_lib.mat(a))
    fn = getattr(_lib.lib(), f"rc_batch_column_id_{_lib.suffix(tdt)}")
    fn.restype = ctypes.c_int32
    assert fn(arr, ctypes.c_int32(2), marr, ctypes.c_int32(0), ctypes.c_int64(40), ctypes.c_void_p(packed.data_ptr())) == _lib.RC_OK
    torch.cuda.synchronize()
    assert bool((packed == 0xA5).all())
    assert_healthy(2)


# ---------------------------------------------------------------- B: verified matrices next to redone ones
@pytest.mark.parametrize("dtype", REAL)
@pytest.mark.parametrize("lanes", [3, 8])
def test_b_mixed_redo_every_slot(lanes, dtype):
    """[G, X, G, X, X, G, X]: the optimistic pass writes C, Z and ind of the four X from a half-factored working copy, the redo
    overwrites them (tests/test_gpu_batch_lanes.py::test_b_and_c_take_the_paths_they_are_meant_to shows that they are redone).  On 3
    lanes the redo list is longer than the lane count: the idle-lanes loop goes more than one round on redone work."""
    case = bl.case_b(dtype)
    hosts = [a for a, _ in case]
    out = check_all(hosts, dev(hosts), bl.X_K, lanes)
    m, n = bl.X_SHAPE
    for i, (a, is_x) in enumerate(case):
        if is_x:  # the designed gap: ten pivots from the low-rank group, then generic columns only
            low = bl.redo_trigger(dtype, bl.seed_of("B", m, n, i))[1]
            ind = npy(out[i][2])
            assert low[ind[:bl.X_RANK]].all() and not low[ind[bl.X_RANK:bl.X_K]].any()


# ---------------------------------------------------------------- C: a lane runs out of pinned state slots
def test_c_flush_in_the_middle_of_the_optimistic_pass():
    # a lane's pinned buffer, c->pinned_size = 65536 bytes (qrb_begin), holds 65536 // sizeof(QrbState) = 65536 // 160 = 409 panel
    # states; five panels per matrix: the 82nd matrix on one lane finds none left, the pass waits, checks and goes on
    slots = 65536 // 160
    assert slots == 409 == bl.pinned_slots_per_lane()
    count = slots // 5 + 3
    assert count == bl.case_c_count()
    hosts = bl.case_c(count)
    at = slots // 5
    check_all(hosts, dev(hosts), bl.C_SHAPE[2], 1, oracle_on=(0, at - 2, at - 1, at, at + 1, at + 2, count - 1))


# ---------------------------------------------------------------- D: k == n
@pytest.mark.parametrize("dtype", REAL)
def test_d_full_rank_of_the_columns(dtype):
    m, n, k = bl.D_SHAPE
    hosts = bl.case_shape("D", bl.D_SHAPE, dtype, 3)
    out = check_all(hosts, dev(hosts), k, 2)
    for (c, z, ind), a in zip(out, hosts):
        z, ind = npy(z), npy(ind)
        want = np.zeros((k, n), dtype=dtype)
        want[np.arange(k), ind] = 1
        assert np.array_equal(z, want)  # a permuted identity
        assert rel(npy(c).astype(np.float64) @ z.astype(np.float64), a) <= TOL[np.dtype(dtype)]["recon"]


# ---------------------------------------------------------------- E, F: shapes off the blocked route
@pytest.mark.parametrize("dtype", REAL)
@pytest.mark.parametrize("shape", bl.E_SHAPES)
def test_e_shapes_the_blocked_factorization_does_not_take(shape, dtype):
    hosts = bl.case_shape("E", shape, dtype, 5)
    check_all(hosts, dev(hosts), shape[2], 2)


@pytest.mark.parametrize("dtype", REAL)
@pytest.mark.parametrize("shape", bl.F_SHAPES)
def test_f_shape_classes_where_the_lone_call_leaves_the_blocked_route(shape, dtype):
    """128 x 512 (short-wide, cooperative), 1024 x 128 (tall-skinny, CholeskyQR2), 64 x 512 (short-wide, m < 128)."""
    hosts = bl.case_shape("F", shape, dtype, 3)
    check_all(hosts, dev(hosts), shape[2], 2)


_FRESH_LONE_SNIPPET = r"""
import numpy as np, torch
from rusty_compression_amd import batch
from tests import batch_lane_cases as bl
shape = (1024, 128, 32)
for a in bl.case_shape("F", shape, np.float32, 3):
    want = bl.oracle(a, shape[2])[0].ind[:shape[2]]
    t = torch.from_numpy(np.array(a)).cuda()
    for rep in range(4):
        ind = batch.column_id_rank(t, shape[2])[2].cpu().numpy()
        print("PIVOTS", int(np.array_equal(ind[:shape[2]], want)))
"""


def test_f_lone_tall_skinny_float32_in_a_fresh_process_has_the_oracles_pivots():
    """The lone float32 call on the three 1024 x 128 matrices of case F as the first GPU work of a child process, four times each:
    every call has the oracle's 32 pivots.  (The tall-skinny path's small pivoted QR, k_qrcp_small, reads the pad row of its LDS image;
    what lies there before the kernel writes it depends on what ran on the compute unit before.)"""
    res = subprocess.run([sys.executable, "-c", _FRESH_LONE_SNIPPET], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert res.returncode == 0, res.stdout[-1500:] + res.stderr[-1500:]
    got = [ln.split()[1] for ln in res.stdout.splitlines() if ln.startswith("PIVOTS ")]
    assert got == ["1"] * 12, got


# ---------------------------------------------------------------- G: layouts
def window(a):
    """a inside a larger buffer: odd element offset, row stride n + 9 > n."""
    m, n = a.shape
    buf = torch.zeros(1 + m * (n + 9), dtype=a.dtype, device=a.device)
    w = buf[1:].view(m, n + 9)[:, :n]
    w.copy_(a)
    assert w.storage_offset() == 1 and w.stride() == (n + 9, 1)
    return w


@pytest.mark.parametrize("dtype", REAL)
def test_g_input_layouts_give_the_contiguous_bits_and_leave_the_input_alone(dtype):
    k = bl.A_SHAPE[2]
    hosts = bl.case_a(dtype, 5)
    base = dev(hosts)
    want = check_all(hosts, base, k, 2)
    layouts = {"column-major": [a.t().contiguous().t() for a in base], "window": [window(a) for a in base]}
    for name, mats in layouts.items():
        assert all(not a.is_contiguous() and torch.equal(a, b) for a, b in zip(mats, base))
        got = slots_of(mats, k, 2)
        for i, (g, w) in enumerate(zip(got, want)):
            assert all(torch.equal(x, y) for x, y in zip(g, w)), f"{name}, slot {i}"
        for a, h in zip(mats, hosts):
            assert npy(a).tobytes() == np.ascontiguousarray(h).tobytes(), f"{name}: the input changed"
    for a, h in zip(base, hosts):
        assert npy(a).tobytes() == np.ascontiguousarray(h).tobytes()
    assert_healthy(2)


# ---------------------------------------------------------------- H: the complex twins
@pytest.mark.parametrize("dtype", list(bl.COMPLEX))
@pytest.mark.parametrize("count,lanes", [(5, 2), (3, 8)])
@pytest.mark.parametrize("shape", bl.H_SHAPES)
def test_h_complex_batches(shape, count, lanes, dtype):
    hosts = bl.case_shape("H", shape, dtype, count)
    mats = dev(hosts)
    mats[1] = window(mats[1])  # one strided input
    check_all(hosts, mats, shape[2], lanes)
    assert npy(mats[1]).tobytes() == np.ascontiguousarray(hosts[1]).tobytes()


# ---------------------------------------------------------------- contexts that would choose different factorizations
# (option, the value that differs from the default, the default, what the message must name)
OPTIONS = [("RC_OPT_BLOCKED_QRCP", 0, 1, "RC_OPT_BLOCKED_QRCP"), ("RC_OPT_COOP_PANEL", 0, 1, "RC_OPT_COOP_PANEL"),
           ("RC_OPT_TALL_SKINNY_FAST_PATH", 0, 1, "RC_OPT_TALL_SKINNY_FAST_PATH"), ("RC_OPT_WIDE_COOP_QRCP", 0, 1, "RC_OPT_WIDE_COOP_QRCP"),
           ("RC_OPT_WIDE_LAZY_QRCP", 0, 1, "RC_OPT_WIDE_LAZY_QRCP"),
           # min(hint, slots) sizes the launches (K splits, the small pivoted QR's launches): 3 against the other lanes' min(1, 4) = 1
           ("RC_OPT_CONCURRENCY_HINT", 3, 1, "RC_OPT_CONCURRENCY_HINT")]


def pattern_untouched(st, packed, ctx, lane):
    torch.cuda.synchronize()
    msg = _lib.lib().rc_last_error_message(ctx._h).decode()
    assert st == _lib.RC_INVALID_ARGUMENT, (st, msg)
    assert f"context {lane}" in msg, msg
    assert bool((packed == 0xA5).all()), "a kernel wrote into the packed buffer of a rejected call"


@pytest.mark.parametrize("dtype", REAL)
@pytest.mark.parametrize("option,other,default,named", OPTIONS, ids=[o[0] for o in OPTIONS])
def test_contexts_that_differ_in_a_factorization_option_are_rejected_before_any_launch(option, other, default, named, dtype):
    k = bl.A_SHAPE[2]
    mats = dev(bl.case_a(dtype, 3))
    dev_id = torch.cuda.current_device()
    streams = [torch.cuda.Stream() for _ in range(3)]
    c0, c1, c2 = (_lib.Context(dev_id, s.cuda_stream) for s in streams)
    try:
        c2.set_option(getattr(_lib, option), other)
        per = batch.packed_bytes(*mats[0].shape, k, mats[0].element_size())
        packed = torch.full((3 * per,), 0xA5, dtype=torch.uint8, device="cuda")
        st, packed = run_batch(mats, k, 3, ctxs=[c0, c1, c2], packed=packed)
        pattern_untouched(st, packed, c0, 2)
        assert named in _lib.lib().rc_last_error_message(c0._h).decode()
        c2.set_option(getattr(_lib, option), default)  # the same contexts in agreement: accepted, and every slot is the lone call's
        st, packed = run_batch(mats, k, 3, ctxs=[c0, c1, c2], packed=packed)
        assert st == _lib.RC_OK
        for (c, z, ind), a in zip(batch.unpack_factors(packed, 3, *mats[0].shape, k, mats[0].dtype), mats):
            c1_, z1_, i1_ = batch.column_id_rank(a, k)
            assert torch.equal(ind, i1_) and torch.equal(c, c1_) and torch.equal(z, z1_)
        assert [c.get_health() for c in (c0, c1, c2)] == [0, 0, 0]
    finally:
        for c in (c0, c1, c2):
            c.close()


@pytest.mark.parametrize("dtype", REAL + list(bl.COMPLEX))
def test_a_context_on_another_device_is_rejected_before_any_launch(dtype):
    if torch.cuda.device_count() < 2:
        pytest.skip("one device visible: a context on another device cannot be made")
    shape = bl.H_SHAPES[0] if bl.is_complex(dtype) else bl.A_SHAPE
    mats = dev(bl.case_shape("H", shape, dtype, 2) if bl.is_complex(dtype) else bl.case_a(dtype, 2))
    k = shape[2]
    c0 = _lib.Context(0, torch.cuda.Stream(0).cuda_stream)
    c1 = _lib.Context(1, torch.cuda.Stream(1).cuda_stream)
    try:
        per = batch.packed_bytes(*mats[0].shape, k, mats[0].element_size())
        packed = torch.full((2 * per,), 0xA5, dtype=torch.uint8, device="cuda:0")
        st, packed = run_batch(mats, k, 2, ctxs=[c0, c1], packed=packed)
        pattern_untouched(st, packed, c0, 1)
    finally:
        c0.close()
        c1.close()


# ---------------------------------------------------------------- proof that B and C took the paths they are meant to
_PATHS_SNIPPET = r"""
import sys
import numpy as np, torch
from tests import batch_lane_cases as bl
from tests import test_gpu_batch_lanes as t
def run(tag, hosts, k, lanes):
    mats = t.dev(hosts)
    sys.stderr.write("CASE " + tag + "\n"); sys.stderr.flush()
    out = t.slots_of(mats, k, lanes)
    assert len(out) == len(hosts)
for dtype in (np.float64, np.float32):
    for lanes in (3, 8):
        run("B %s %d" % (np.dtype(dtype).name, lanes), [a for a, _ in bl.case_b(dtype)], bl.X_K, lanes)
run("C float32 1", bl.case_c(bl.case_c_count()), bl.C_SHAPE[2], 1)
sys.stderr.write("CASE end\n")
"""


def test_b_and_c_take_the_paths_they_are_meant_to():
    """RC_BATCH_DEBUG is read once per process: cases B and C once more in one child, whose debug lines must report exactly the X
    matrices redone (4 of 7, by index) for B and at least one flush with nothing redone for C.  A condition, not a measurement: a run in
    which nothing was redone, or nothing flushed, fails."""
    res = subprocess.run([sys.executable, "-c", _PATHS_SNIPPET], env=dict(os.environ, RC_BATCH_DEBUG="1"), capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert res.returncode == 0, res.stdout[-1500:] + res.stderr[-1500:]
    seen = {}
    tag = None
    for ln in res.stderr.splitlines():
        if ln.startswith("CASE "):
            tag = ln[5:]
            continue
        mt = re.match(r"rc_batch optimistic: (\d+) matrices issued .* (\d+) to redo, (\d+) flushes, redo:((?: \d+)*)$", ln)
        if mt and tag:
            assert tag not in seen, f"two optimistic passes in {tag}"
            seen[tag] = (int(mt.group(1)), int(mt.group(2)), int(mt.group(3)), [int(v) for v in mt.group(4).split()])
    xs = [i for i, kind in enumerate(bl.B_KINDS) if kind == "X"]
    assert xs == [1, 3, 4, 6]
    for dtype in ("float64", "float32"):
        for lanes in (3, 8):
            assert seen.get(f"B {dtype} {lanes}") == (7, 4, 0, xs), (dtype, lanes, seen)
    count = bl.case_c_count()
    assert "C float32 1" in seen, seen
    issued, redone, flushes, which = seen["C float32 1"]
    assert issued == count and redone == 0 and which == [] and flushes >= 1, seen["C float32 1"]
