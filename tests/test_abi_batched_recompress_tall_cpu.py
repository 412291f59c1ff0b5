"""CPU checks of the tall batched recompression at the drop-in boundary: rc_lowrank_recompress_tall_batched_f64 / _f32 and the plan query
rc_lowrank_recompress_tall_batched_plan are declared in include/rusty_compression_amd.h, exported by the built library, reject a null
context before touching a device, are reachable from Python and through the C++ mirror's recompress_tall_batched overloads.

No context exists without a device, so the entry points' own argument checks (tol, null outputs, batch strides, the shape of u) are
exercised in tests/test_gpu_batched_recompress_tall.py.  The shape domain is checked here through the plan query, which is host arithmetic
and applies the same bounds: it is also where the stage count, the slot size and the 2 GiB grid bound are pinned without a launch."""
import ctypes
import os

import rusty_compression_amd as rc
from rusty_compression_amd import _lib
from tests.test_abi_cpu import build_cpp_mirror_examples

SYMBOLS = [f"rc_lowrank_recompress_tall_batched_{s}" for s in ("f64", "f32")]
H = 512  # the stage height


def plan(m, n, K, elem_bytes=8, resident=256):
    """(status, stages, slot_bytes, grid) of rc_lowrank_recompress_tall_batched_plan."""
    out = [ctypes.c_int64(-1) for _ in range(3)]
    st = _lib.lib().rc_lowrank_recompress_tall_batched_plan(ctypes.c_int64(m), ctypes.c_int64(n), ctypes.c_int64(K), ctypes.c_int32(elem_bytes),
                                                          ctypes.c_int64(resident), *[ctypes.byref(x) for x in out])
    return (st,) + tuple(x.value for x in out)


def stages(m, K):
    return 1 if m <= H else 1 + -(-(m - H) // (H - K))


def test_tall_recompress_symbols_are_declared_and_exported():
    declared = set(_lib.declared_symbols())
    lib = _lib.lib()
    for s in SYMBOLS + ["rc_lowrank_recompress_tall_batched_plan"]:
        assert s in declared, s
        assert hasattr(lib, s), s
    for s in ("c64", "c32"):  # real scalars only
        assert f"rc_lowrank_recompress_tall_batched_{s}" not in declared
        assert not hasattr(lib, f"rc_lowrank_recompress_tall_batched_{s}")


def test_tall_recompress_entry_points_reject_a_null_context():
    lib = _lib.lib()
    none = _lib.mat(None)
    zero = ctypes.c_int64(0)
    for s in SYMBOLS:
        assert getattr(lib, s)(ctypes.c_void_p(None), none, zero, none, zero, None, zero, none, zero, None, ctypes.c_int32(0), ctypes.c_int64(1),
                               ctypes.c_double(0.0), none, zero, None, none, zero, None) == _lib.RC_INVALID_ARGUMENT


def test_domain_edges_through_the_plan_query():
    bad = _lib.RC_INVALID_ARGUMENT
    assert plan(65537, 64, 16)[0] == bad      # m > 65536
    assert plan(2048, 513, 16)[0] == bad      # n > 512
    assert plan(2048, 512, 129)[0] == bad     # K > 128
    assert plan(2048, 12, 16)[0] == bad       # K > min(m, n)
    assert plan(8, 64, 16)[0] == bad
    assert plan(0, 64, 1)[0] == bad and plan(64, 0, 1)[0] == bad and plan(64, 64, 0)[0] == bad
    assert plan(2048, 64, 16, elem_bytes=2)[0] == bad and plan(2048, 64, 16, resident=0)[0] == bad
    for m in (1, 512, 513, 65536):             # both sides of the first extra row, and the last row of the domain
        st, sg, slot, grid = plan(m, 64, 1 if m == 1 else 16)
        assert st == 0 and sg == stages(m, 16 if m > 1 else 1), (m, st, sg)


def test_stage_count_slot_and_grid_bound():
    for elem in (8, 4):
        for m, n, K in ((513, 130, 128), (896, 130, 128), (897, 130, 128), (1021, 17, 17), (1022, 17, 17), (1500, 96, 40), (2100, 64, 64), (65536, 512, 128)):
            st, sg, slot, grid = plan(m, n, K, elem)
            assert st == 0 and sg == stages(m, K), (m, K, sg)
            copies = sg * (H * K + 2 * K) * elem
            assert copies <= slot <= copies + (n * K + K * K) * elem  # the stage copies, plus the copy of right and the rotations when they leave LDS
            assert grid == max(1, min(256, (2 << 30) // slot))
    # the largest block of the domain in f64: 171 stages, about 90 MiB a slot, so the 2 GiB bound leaves 23 of 256 resident workgroups
    st, sg, slot, grid = plan(65536, 512, 128, 8, 256)
    assert (st, sg) == (0, 171) and 85 << 20 < slot < 95 << 20 and grid == (2 << 30) // slot == 23
    assert plan(65536, 512, 128, 8, 1)[3] == 1 and plan(65536, 512, 128, 8, 7)[3] == 7
    # one stage: the existing call's plan, nothing for the bound to do
    st, sg, slot, grid = plan(512, 64, 64, 8, 256)
    assert (st, sg, grid) == (0, 1, 256) and slot == 512 * 64 * 8


def test_python_names_exist():
    for name in ("lowrank_recompress_tall_batched", "column_id_to_svd_tall_batched", "svd_add_tall_batched", "sketch_svd_rank_batched"):
        assert callable(getattr(rc, name)), name
        assert name in rc.__all__, name


def test_cpp_mirror_reaches_the_tall_batched_recompress(tmp_path):
    exe = build_cpp_mirror_examples(tmp_path, "batched_recompress_tall_example.cpp")
    assert os.path.exists(exe)
