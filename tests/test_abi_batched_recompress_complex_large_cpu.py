"""CPU checks of the complex batched recompression with both factors tall at the drop-in boundary:
rc_lowrank_recompress_complex_large_batched_c64 / _c32 and the plan query rc_lowrank_recompress_complex_large_batched_plan are declared in
include/rusty_compression_amd.h, exported by the built library, present in the Rust FFI, reject a null context before touching a device, are
reachable from Python and through the C++ mirror's recompress_large_batched overloads for c64 / c32.

The stem has "complex" before "large": the spellings a twin of rc_lowrank_recompress_large_batched_* might otherwise have taken are pinned as
absent by tests/test_abi_batched_recompress_large_cpu.py and stay absent.

No context exists without a device, so the entry points' own argument checks are exercised in tests/test_gpu_batched_recompress_large_complex.py.
The shape domain is checked here through the plan query, which is host arithmetic and applies the same bounds: it is also where the stage
counts of both sides, the slot layout and the 2 GiB grid bound are pinned without a launch."""
import ctypes
import os

import rusty_compression_amd as rc
from rusty_compression_amd import _lib
from tests.test_abi_cpu import build_cpp_mirror_examples

SYMBOLS = [f"rc_lowrank_recompress_complex_large_batched_{s}" for s in ("c64", "c32")]
PLAN = "rc_lowrank_recompress_complex_large_batched_plan"
H = 512  # the stage height
FFI = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bindings", "rust", "src", "ffi.rs")


def plan(m, n, K, real_bytes=8, resident=256):
    """(status, stages_left, stages_right, slot_bytes, grid) of rc_lowrank_recompress_complex_large_batched_plan."""
    out = [ctypes.c_int64(-1) for _ in range(4)]
    st = getattr(_lib.lib(), PLAN)(ctypes.c_int64(m), ctypes.c_int64(n), ctypes.c_int64(K), ctypes.c_int32(real_bytes), ctypes.c_int64(resident),
                                   *[ctypes.byref(x) for x in out])
    return (st,) + tuple(x.value for x in out)


def tall_plan(m, n, K, real_bytes=8, resident=256):
    """(status, stages, slot_bytes, grid) of rc_lowrank_recompress_tall_complex_batched_plan."""
    out = [ctypes.c_int64(-1) for _ in range(3)]
    st = _lib.lib().rc_lowrank_recompress_tall_complex_batched_plan(ctypes.c_int64(m), ctypes.c_int64(n), ctypes.c_int64(K), ctypes.c_int32(real_bytes),
                                                                  ctypes.c_int64(resident), *[ctypes.byref(x) for x in out])
    return (st,) + tuple(x.value for x in out)


def stages(x, K):
    return 1 if x <= H else 1 + -(-(x - H) // (H - K))


def test_complex_large_recompress_symbols_are_declared_exported_and_bound():
    declared = set(_lib.declared_symbols())
    lib = _lib.lib()
    ffi = open(FFI).read()
    for s in SYMBOLS + [PLAN]:
        assert s in declared, s
        assert hasattr(lib, s), s
        assert f"pub fn {s}(" in ffi, s


def test_complex_large_recompress_entry_points_reject_a_null_context():
    lib = _lib.lib()
    none = _lib.mat(None)
    zero = ctypes.c_int64(0)
    for s, tol in zip(SYMBOLS, (ctypes.c_double(0.0), ctypes.c_float(0.0))):
        assert getattr(lib, s)(ctypes.c_void_p(None), none, zero, none, zero, None, zero, none, zero, None, ctypes.c_int32(0), ctypes.c_int64(1),
                               tol, none, zero, None, none, zero, None) == _lib.RC_INVALID_ARGUMENT


def test_python_names_exist():
    for name in ("lowrank_recompress_large_batched_complex", "svd_add_large_batched_complex"):
        assert callable(getattr(rc, name)), name
        assert name in rc.__all__, name


def test_domain_edges_through_the_plan_query():
    bad = _lib.RC_INVALID_ARGUMENT
    assert plan(65537, 64, 16)[0] == bad and plan(64, 65537, 16)[0] == bad  # m or n > 65536
    assert plan(2048, 2048, 129)[0] == bad                                  # K > 128
    assert plan(2048, 12, 16)[0] == bad and plan(12, 2048, 16)[0] == bad    # K > min(m, n)
    assert plan(0, 64, 1)[0] == bad and plan(64, 0, 1)[0] == bad and plan(64, 64, 0)[0] == bad
    assert plan(2048, 2048, 16, real_bytes=2)[0] == bad and plan(2048, 2048, 16, resident=0)[0] == bad
    assert plan(2048, 2048, 16, real_bytes=16)[0] == bad  # the size of the real type, not of the element
    lib = _lib.lib()
    i64 = ctypes.c_int64
    outs = [i64(0) for _ in range(4)]
    for missing in range(4):  # a null output
        args = [ctypes.byref(x) if i != missing else None for i, x in enumerate(outs)]
        assert getattr(lib, PLAN)(i64(2048), i64(2048), i64(16), ctypes.c_int32(8), i64(256), *args) == bad
    edge = (1, 512, 513, 65536)  # both sides of the first extra row / column, and the last of the domain
    for m in edge:
        for n in edge:
            K = 1 if min(m, n) == 1 else 16
            for real_bytes in (8, 4):
                st, sl, sr, slot, grid = plan(m, n, K, real_bytes)
                assert st == 0 and sl == stages(m, K) and sr == stages(n, K), (m, n, st, sl, sr)
    assert stages(512, 16) == 1 and stages(513, 16) == 2 and stages(896, 128) == 2 and stages(897, 128) == 3
    assert stages(1021, 17) == 3 and stages(1022, 17) == 3 and stages(1023, 17) == 3 and stages(65536, 128) == 171


def test_narrow_right_factor_has_the_tall_complex_calls_plan():
    for real_bytes in (8, 4):
        for m, n, K in ((64, 64, 16), (512, 512, 128), (513, 130, 128), (2100, 64, 64), (1500, 512, 40), (65536, 512, 128), (300, 64, 16)):
            for resident in (1, 7, 256):
                st, sl, sr, slot, grid = plan(m, n, K, real_bytes, resident)
                tst, tsg, tslot, tgrid = tall_plan(m, n, K, real_bytes, resident)
                assert st == 0 and tst == 0 and sr == 1
                assert (sl, slot, grid) == (tsg, tslot, tgrid), (m, n, K, real_bytes)


def test_stage_counts_slot_and_grid_bound():
    for real_bytes in (8, 4):
        elem = 2 * real_bytes  # one interleaved complex element
        for m, n, K in ((513, 513, 3), (600, 897, 128), (897, 600, 128), (1022, 1022, 17), (1100, 1500, 40), (2048, 2048, 32), (1024, 1024, 64),
                        (4096, 4096, 64), (65536, 65536, 128), (65536, 513, 1), (513, 65536, 128)):
            st, sl, sr, slot, grid = plan(m, n, K, real_bytes)
            assert st == 0 and sl == stages(m, K) and sr == stages(n, K), (m, n, K, sl, sr)
            copies = (sl + sr) * (H * K + 2 * K) * elem
            assert copies <= slot <= copies + 2 * K * K * elem, (m, n, K, elem, slot, copies)  # the core and the rotations only when they leave LDS
            assert grid == max(1, min(256, (2 << 30) // slot))
        # a short left factor beside a staged right one: left's copy is in LDS or in the slot, the right factor's stages always in the slot
        for m, n, K in ((130, 513, 128), (130, 897, 128), (17, 1021, 17), (64, 2100, 64), (300, 2100, 64), (512, 65536, 128)):
            st, sl, sr, slot, grid = plan(m, n, K, real_bytes)
            assert st == 0 and sl == 1 and sr == stages(n, K)
            copies = sr * (H * K + 2 * K) * elem
            assert copies <= slot <= copies + (m * K + 2 * K * K) * elem, (m, n, K, elem, slot, copies)
            assert grid == max(1, min(256, (2 << 30) // slot))
    # the largest block of the domain in c64: two sides of 171 stages of 1052672 bytes, then the core at pitch K and the rotations (neither fits
    # in LDS at K = 128), leave 5 of 256 resident workgroups
    st, sl, sr, slot, grid = plan(65536, 65536, 128, 8, 256)
    assert (st, sl, sr) == (0, 171, 171) and (H * 128 + 2 * 128) * 16 == 1052672
    assert slot == 2 * 171 * 1052672 + 2 * 128 * 128 * 16 and grid == (2 << 30) // slot == 5
    assert plan(65536, 65536, 128, 8, 1)[4] == 1 and plan(65536, 65536, 128, 8, 3)[4] == 3
    # c32 at the same corner: the core fits in LDS at the padded pitch, the rotations do not
    st, sl, sr, slot, grid = plan(65536, 65536, 128, 4, 256)
    assert slot == 2 * 171 * 526336 + 128 * 128 * 8 and grid == (2 << 30) // slot == 11


def test_cpp_mirror_reaches_the_complex_large_batched_recompress(tmp_path):
    exe = build_cpp_mirror_examples(tmp_path, "batched_recompress_large_complex_example.cpp")
    assert os.path.exists(exe)
