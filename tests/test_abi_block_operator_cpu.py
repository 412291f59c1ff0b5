"""CPU checks of the block-sparse operator at the drop-in boundary: rc_block_operator_apply_f64 / _f32 / _c64 / _c32 are declared in
include/rusty_compression_amd.h, exported by the built library, present in the generated Rust FFI, reject a null context before touching
a device, are reachable from Python and through the C++ mirror's BlockOperator; and batch.block_csr builds the block-CSR pattern and its
transposed twin on the host."""
import ctypes
import os

import numpy as np
import pytest

import rusty_compression_amd as rc
from rusty_compression_amd import _lib
from tests.test_abi_cpu import build_cpp_mirror_examples

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = [f"rc_block_operator_apply_{s}" for s in ("f64", "f32", "c64", "c32")]


def test_block_operator_symbols_are_declared_exported_and_bound_for_rust():
    declared = set(_lib.declared_symbols())
    lib = _lib.lib()
    with open(os.path.join(ROOT, "bindings", "rust", "src", "ffi.rs")) as f:
        ffi = f.read()
    for s in SYMBOLS:
        assert s in declared, s
        assert hasattr(lib, s), s
        assert f"pub fn {s}(" in ffi, s


def test_block_operator_entry_points_reject_a_null_context():
    lib = _lib.lib()
    none = _lib.mat(None)
    zero, izero = ctypes.c_int64(0), ctypes.c_int32(0)
    for s in SYMBOLS:
        assert getattr(lib, s)(ctypes.c_void_p(None), none, zero, none, zero, None, zero, none, zero, None, izero, none, zero, izero, None, None, izero,
                               None, None, none, none, izero, izero) == _lib.RC_INVALID_ARGUMENT


def test_python_names_exist():
    for name in ("block_operator_apply", "block_csr", "BlockLowRankOperator"):
        assert callable(getattr(rc, name)), name
        assert name in rc.__all__, name
    assert issubclass(rc.BlockLowRankOperator, rc.Operator)


def test_cpp_mirror_reaches_the_block_operator(tmp_path):
    exe = build_cpp_mirror_examples(tmp_path, "batched_operator_apply_example.cpp")
    assert os.path.exists(exe)


def dense_of(pattern, nblocks):
    """The pattern as a {(group_row, entry_col): [block ids in order]} map, and the groups' rows in order."""
    ptr, row, block, col = pattern
    assert all(a.dtype == np.int64 for a in pattern)
    assert ptr.shape == (row.size + 1,) and ptr[0] == 0 and np.all(np.diff(ptr) >= 0) and ptr[-1] == block.size == col.size
    assert block.size == 0 or (block.min() >= 0 and block.max() < nblocks)
    cells = {}
    for g in range(row.size):
        for e in range(ptr[g], ptr[g + 1]):
            cells.setdefault((int(row[g]), int(col[e])), []).append(int(block[e]))
    return cells, [int(r) for r in row]


def test_block_csr_on_an_unsorted_input_with_a_repeated_block():
    # a 3 x 2 grid of 40 x 32 tiles given out of order; block 1 sits in two cells, and cell (40, 0) holds two blocks (summed in input order)
    rows = [80, 0, 40, 0, 40, 80, 40]
    cols = [32, 32, 0, 0, 32, 0, 0]
    ids = [5, 1, 2, 0, 1, 4, 3]
    by_row, by_col = rc.block_csr(rows, cols, ids)
    cells, group_rows = dense_of(by_row, 6)
    assert group_rows == [0, 40, 80]
    assert cells == {(80, 32): [5], (0, 32): [1], (40, 0): [2, 3], (0, 0): [0], (40, 32): [1], (80, 0): [4]}
    ptr, _, block, col = by_row
    assert ptr.tolist() == [0, 2, 5, 7]
    assert block.tolist() == [1, 0, 2, 1, 3, 5, 4] and col.tolist() == [32, 0, 0, 32, 0, 32, 0]  # input order inside every group
    cells_t, group_cols = dense_of(by_col, 6)
    assert group_cols == [0, 32]
    assert cells_t == {(c, r): v for (r, c), v in cells.items()}  # the same cells with rows and columns exchanged
    ptr_t, _, block_t, col_t = by_col
    assert ptr_t.tolist() == [0, 4, 7]
    assert block_t.tolist() == [2, 0, 4, 3, 5, 1, 1] and col_t.tolist() == [40, 0, 80, 40, 80, 0, 40]


def test_block_csr_with_an_empty_group_and_listed_groups():
    by_row, by_col = rc.block_csr([64, 0], [0, 16], [7, 7], group_rows=[0, 32, 64], group_cols=[16, 0, 48])
    ptr, row, block, col = by_row
    assert ptr.tolist() == [0, 1, 1, 2] and row.tolist() == [0, 32, 64]  # the group at row 32 is empty
    assert block.tolist() == [7, 7] and col.tolist() == [16, 0]
    ptr_t, row_t, block_t, col_t = by_col
    assert row_t.tolist() == [16, 0, 48] and ptr_t.tolist() == [0, 1, 2, 2]  # listed order kept; column 48 has no entry
    assert block_t.tolist() == [7, 7] and col_t.tolist() == [0, 64]
    empty, empty_t = rc.block_csr([], [], [], group_rows=[0, 8])
    assert empty[0].tolist() == [0, 0, 0] and empty[1].tolist() == [0, 8] and empty[2].size == 0 and empty[3].size == 0
    assert empty_t[0].tolist() == [0] and empty_t[1].size == 0
    with pytest.raises(AssertionError):
        rc.block_csr([0, 8], [0, 0], [0, 1], group_rows=[0])  # the entry at row 8 belongs to no listed group
    with pytest.raises(AssertionError):
        rc.block_csr([0, 8], [0], [0, 1])
