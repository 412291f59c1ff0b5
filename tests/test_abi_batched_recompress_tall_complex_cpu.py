"""CPU checks of the tall complex batched recompression at the drop-in boundary: rc_lowrank_recompress_tall_complex_batched_c64 / _c32 and the
plan query rc_lowrank_recompress_tall_complex_batched_plan are declared in include/rusty_compression_amd.h, exported by the built library,
listed in the Rust ffi, reject a null context before touching a device, are reachable from Python and through the C++ mirror's
recompress_tall_batched overloads.  rc_lowrank_recompress_tall_batched_c64 / _c32 stay absent: the stem of the complex pair is its own.

No context exists without a device, so the entry points' own argument checks are exercised in
tests/test_gpu_batched_recompress_tall_complex.py.  The shape domain is checked here through the plan query, which is host arithmetic and
applies the same bounds: it is also where the stage count, the slot size and the 2 GiB grid bound are pinned without a launch."""
import ctypes
import os
import re

import rusty_compression_amd as rc
from rusty_compression_amd import _lib
from tests.test_abi_cpu import build_cpp_mirror_examples

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = [f"rc_lowrank_recompress_tall_complex_batched_{s}" for s in ("c64", "c32")]
PLAN = "rc_lowrank_recompress_tall_complex_batched_plan"
H = 512  # the stage height


def plan(m, n, K, real_bytes=8, resident=256):
    """(status, stages, slot_bytes, grid) of rc_lowrank_recompress_tall_complex_batched_plan."""
    out = [ctypes.c_int64(-1) for _ in range(3)]
    st = getattr(_lib.lib(), PLAN)(ctypes.c_int64(m), ctypes.c_int64(n), ctypes.c_int64(K), ctypes.c_int32(real_bytes), ctypes.c_int64(resident),
                                   *[ctypes.byref(x) for x in out])
    return (st,) + tuple(x.value for x in out)


def stages(m, K):
    return 1 if m <= H else 1 + -(-(m - H) // (H - K))


def test_tall_complex_recompress_symbols_are_declared_exported_and_in_the_rust_ffi():
    declared = set(_lib.declared_symbols())
    lib = _lib.lib()
    with open(os.path.join(ROOT, "bindings", "rust", "src", "ffi.rs")) as f:
        ffi = set(re.findall(r"pub fn (rc_\w+)\(", f.read()))
    for s in SYMBOLS + [PLAN]:
        assert s in declared, s
        assert hasattr(lib, s), s
        assert s in ffi, s
    for s in ("c64", "c32"):  # the real stem has no complex members
        name = f"rc_lowrank_recompress_tall_batched_{s}"
        assert name not in declared and not hasattr(lib, name) and name not in ffi


def test_tall_complex_recompress_entry_points_reject_a_null_context():
    lib = _lib.lib()
    none = _lib.mat(None)
    zero = ctypes.c_int64(0)
    for s, tol in zip(SYMBOLS, (ctypes.c_double(0.0), ctypes.c_float(0.0))):  # tol has the real type of the data
        assert getattr(lib, s)(ctypes.c_void_p(None), none, zero, none, zero, None, zero, none, zero, None, ctypes.c_int32(0), ctypes.c_int64(1), tol,
                               none, zero, None, none, zero, None) == _lib.RC_INVALID_ARGUMENT
    with open(os.path.join(ROOT, "include", "rusty_compression_amd.h")) as f:
        header = f.read()
    assert re.search(r"rc_lowrank_recompress_tall_complex_batched_c32\([^;]*int64_t k, float tol,", header)
    assert re.search(r"rc_lowrank_recompress_tall_complex_batched_c64\([^;]*int64_t k, double tol,", header)


def test_domain_edges_through_the_plan_query():
    bad = _lib.RC_INVALID_ARGUMENT
    for rb in (8, 4):
        assert plan(65537, 64, 16, rb)[0] == bad      # m > 65536
        assert plan(2048, 513, 16, rb)[0] == bad      # n > 512
        assert plan(2048, 512, 129, rb)[0] == bad     # K > 128
        assert plan(2048, 12, 16, rb)[0] == bad       # K > min(m, n)
        assert plan(8, 64, 16, rb)[0] == bad
        assert plan(0, 64, 1, rb)[0] == bad and plan(64, 0, 1, rb)[0] == bad and plan(64, 64, 0, rb)[0] == bad
        assert plan(2048, 64, 16, rb, resident=0)[0] == bad
        for m in (1, 512, 513, 65536):                 # both sides of the first extra row, and the last row of the domain
            st, sg, slot, grid = plan(m, 64, 1 if m == 1 else 16, rb)
            assert st == 0 and sg == stages(m, 16 if m > 1 else 1), (m, st, sg)
    for rb in (2, 16, 0, -8):                          # 16 is the size of a c64 element, not of its real type
        assert plan(2048, 64, 16, rb)[0] == bad
    lib = _lib.lib()
    ok = [ctypes.c_int64(0) for _ in range(3)]
    for null in range(3):                              # a null output
        ptrs = [None if i == null else ctypes.byref(x) for i, x in enumerate(ok)]
        assert getattr(lib, PLAN)(ctypes.c_int64(2048), ctypes.c_int64(64), ctypes.c_int64(16), ctypes.c_int32(8), ctypes.c_int64(256), *ptrs) == bad


def test_stage_count_slot_and_grid_bound():
    for rb in (8, 4):
        elem = 2 * rb
        for m, n, K in ((513, 130, 128), (896, 130, 128), (897, 130, 128), (1021, 17, 17), (1022, 17, 17), (1500, 96, 40), (2100, 64, 64), (65536, 512, 128)):
            st, sg, slot, grid = plan(m, n, K, rb)
            assert st == 0 and sg == stages(m, K), (m, K, sg)
            copies = sg * (H * K + 2 * K) * elem
            # the stage copies, plus the copy of right, the rotations and the core when they leave LDS
            assert copies <= slot <= copies + (n * K + 2 * K * K) * elem, (m, n, K, rb, slot)
            assert grid == max(1, min(256, (2 << 30) // slot))
    # the largest block of the domain: 171 stages of 512 * 128 + 256 = 65 792 complex elements, 173 MiB a slot in c64 and half of it in c32, so
    # the 2 GiB bound leaves 11 and 23 of 256 resident workgroups (the real call's 23 at the same bytes per element).  (1.34 GiB and grids of
    # 1 and 2 would follow from 171 x 526 336 complex elements, but 526 336 is the bytes of one f64 stage: DESIGN.md 7p.)
    st, sg, slot64, grid64 = plan(65536, 512, 128, 8, 256)
    assert (st, sg) == (0, 171) and 170 << 20 < slot64 < 190 << 20 and grid64 == (2 << 30) // slot64 == 11
    st, sg, slot32, grid32 = plan(65536, 512, 128, 4, 256)
    assert (st, sg) == (0, 171) and 85 << 20 < slot32 < 95 << 20 and grid32 == (2 << 30) // slot32 == 23
    assert plan(65536, 512, 128, 8, 1)[3] == 1 and plan(65536, 512, 128, 8, 7)[3] == 7 and plan(65536, 512, 128, 4, 7)[3] == 7


def test_a_single_stage_has_the_existing_calls_plan():
    """(512, 64, 64) is one stage, and the slot is what the existing complex call's plan takes there, by the arithmetic of its LDS need against
    the 159 KiB cap (tests/test_gpu_batched_recompress_complex.py, PLAN_CASES): in c64 the core and the rotations fit at the odd pitch 65 only
    without either copy (133 KiB), so the copies of left (512 x 64) and of right^T (64 x 64) are in the slot; in c32 the copy of right^T,
    the core and the rotations fit at pitch 80 and the copy of left alone is in the slot."""
    st, sg, slot, grid = plan(512, 64, 64, 8, 256)
    assert (st, sg, grid) == (0, 1, 256) and slot == (512 * 64 + 64 * 64) * 16
    st, sg, slot, grid = plan(512, 64, 64, 4, 256)
    assert (st, sg, grid) == (0, 1, 256) and slot == 512 * 64 * 8
    # one row more: two stages, each a full 512 x K copy with its taus and pivots
    st, sg, slot, grid = plan(513, 64, 64, 4, 256)
    assert (st, sg) == (0, 2) and slot == 2 * (512 * 64 + 2 * 64) * 8


def test_python_names_exist():
    for name in ("lowrank_recompress_tall_batched_complex", "column_id_to_svd_tall_batched_complex", "svd_add_tall_batched_complex",
                 "sketch_svd_rank_batched_complex"):
        assert callable(getattr(rc, name)), name
        assert name in rc.__all__, name


def test_cpp_mirror_reaches_the_tall_complex_batched_recompress(tmp_path):
    exe = build_cpp_mirror_examples(tmp_path, "batched_recompress_tall_complex_example.cpp")
    assert os.path.exists(exe)
