"""The view harness of tests/view_layouts.py on CPU tensors, no library call: every fault tests/test_gpu_output_views.py relies on
it to report is planted here by hand and must be reported, so that the GPU file cannot pass vacuously."""
import numpy as np
import pytest
import torch

from tests import view_layouts as vl

DTYPES = [np.float64, np.float32, np.complex128, np.complex64]
SHAPES = [(5, 4), (4, 5), (1, 7), (7, 1), (1, 1), (8, 9)]


def index_of(view, buffer, i, j):
    """Flat index of the (possibly out-of-range) position (i, j) of the view."""
    off = (view.data_ptr() - buffer.data_ptr()) // view.element_size()
    return off + i * view.stride(0) + j * view.stride(1)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("layout", vl.LAYOUTS)
def test_a_fresh_view_is_all_sentinel_and_a_write_through_it_stays_inside(layout, shape, dtype):
    view, buffer, inside = vl.make_view(*shape, dtype, layout, "cpu")
    assert tuple(view.shape) == shape and int(inside.sum()) == shape[0] * shape[1]
    assert torch.isnan(torch.view_as_real(buffer) if buffer.is_complex() else buffer).all()  # quiet NaN in every part
    vl.assert_outside_untouched(buffer, inside)
    assert not vl.written(view).any()
    with pytest.raises(AssertionError, match="never written"):
        vl.assert_inside_written(view)
    view.copy_(torch.arange(shape[0] * shape[1], dtype=torch.float64).reshape(shape).to(view.dtype))
    vl.assert_outside_untouched(buffer, inside)
    vl.assert_inside_written(view)
    assert np.array_equal(view.numpy().real, np.arange(shape[0] * shape[1]).reshape(shape))
    assert np.array_equal(vl.bits(view), vl.bits(view.clone()))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("layout", ["FP", "CP"])
def test_a_one_element_write_in_each_guard_side_is_reported(layout, shape, dtype):
    rows, cols = shape
    sides = {"above": (-1, cols // 2), "below": (rows, cols // 2), "left": (rows // 2, -1), "right": (rows // 2, cols),
             "far corner": (rows + vl.GUARD - 1, cols + vl.GUARD - 1), "near corner": (-vl.GUARD, -vl.GUARD)}
    for side, (i, j) in sides.items():
        # a finite value, a NaN of another payload, and (complex) a write of the imaginary part alone
        for value in (0.0, float("nan")):
            view, buffer, inside = vl.make_view(rows, cols, dtype, layout, "cpu")
            view.fill_(1.0)
            e = index_of(view, buffer, i, j)
            assert 0 <= e < buffer.numel() and not inside[e], side
            buffer[e] = value
            with pytest.raises(AssertionError, match="outside the view"):
                vl.assert_outside_untouched(buffer, inside)
        if np.dtype(dtype).kind == "c":
            view, buffer, inside = vl.make_view(rows, cols, dtype, layout, "cpu")
            torch.view_as_real(buffer)[index_of(view, buffer, i, j), 1] = 2.0
            with pytest.raises(AssertionError, match="outside the view"):
                vl.assert_outside_untouched(buffer, inside)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES)
def test_a_write_into_the_gaps_of_the_strided_view_is_reported(shape, dtype):
    rows, cols = shape
    for di, dj in [(0, -1), (0, 1), (-1, 0), (1, 0), (-1, -1)]:  # in half steps of the view's strides: the buffer's neighbours
        view, buffer, inside = vl.make_view(rows, cols, dtype, "S", "cpu")
        view.fill_(1.0)
        e = index_of(view, buffer, rows // 2, cols // 2) + di * view.stride(0) // 2 + dj * view.stride(1) // 2
        if not 0 <= e < buffer.numel():
            continue  # the last row and column of the buffer are the view's own
        assert not inside[e]
        buffer[e] = 0.0
        with pytest.raises(AssertionError, match="outside the view"):
            vl.assert_outside_untouched(buffer, inside)
    # every second element of the buffer in both directions is the view's, and nothing else
    grid = inside.reshape(2 * rows, 2 * cols)
    assert grid[1::2, 1::2].all() and int(grid.sum()) == rows * cols


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("layout", ["FP", "CP", "S"])
def test_a_result_written_with_the_wrong_pitch_is_reported(layout, dtype):
    rows, cols = 5, 4
    view, buffer, inside = vl.make_view(rows, cols, dtype, layout, "cpu")
    off = (view.data_ptr() - buffer.data_ptr()) // view.element_size()
    rs, cs = view.stride()
    # the pitch a kernel would use that takes the view for contiguous, and the padded pitch rounded up to even
    wrong = [(1, rows), (1, cs + 1)] if layout == "FP" else [(cols, 1), (rs + 1, 1)] if layout == "CP" else [(rs // 2, cs), (rs, 1)]
    for strides in wrong:
        view, buffer, inside = vl.make_view(rows, cols, dtype, layout, "cpu")
        torch.as_strided(buffer, (rows, cols), strides, off).fill_(1.0)
        with pytest.raises(AssertionError, match="outside the view"):
            vl.assert_outside_untouched(buffer, inside)
        with pytest.raises(AssertionError, match="never written"):
            vl.assert_inside_written(view)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES + [(37, 23), (131, 137), (1031, 9)])
def test_padded_views_have_an_odd_pitch_an_odd_offset_and_an_unaligned_pointer(shape, dtype):
    rows, cols = shape
    esz = np.dtype(dtype).itemsize
    for layout in ("FP", "CP"):
        view, buffer, _ = vl.make_view(rows, cols, dtype, layout, "cpu")
        off = (view.data_ptr() - buffer.data_ptr()) // esz
        pitch = view.stride(1) if layout == "FP" else view.stride(0)
        assert pitch % 2 == 1 and off % 2 == 1 and (view.stride(0) if layout == "FP" else view.stride(1)) == 1
        assert esz == 16 or view.data_ptr() % 16 in (4, 8, 12)
        # the properties are asserted of the view itself, so a helper that lost them is reported: an even pitch, an even (16-byte
        # aligned) offset, and a band thinner than GUARD
        strides = (1, pitch - 1) if layout == "FP" else (pitch - 1, 1)
        with pytest.raises(AssertionError, match="is even"):
            vl.assert_layout_properties(torch.as_strided(buffer, shape, strides, off), buffer, layout)
        with pytest.raises(AssertionError, match="is even"):
            vl.assert_layout_properties(torch.as_strided(buffer, shape, view.stride(), off + 1), buffer, layout)
        with pytest.raises(AssertionError, match="guard band"):
            vl.assert_layout_properties(torch.as_strided(buffer, shape, view.stride(), 1), buffer, layout)
        if esz < 16:
            aligned = torch.as_strided(buffer, shape, view.stride(), off + 16 // esz - off % (16 // esz))
            assert aligned.data_ptr() % 16 == 0
            with pytest.raises(AssertionError):
                vl.assert_layout_properties(aligned, buffer, layout)


def test_a_view_that_overlaps_itself_or_leaves_its_allocation_is_refused():
    buffer = vl.sentinel_buffer(20, np.float64, "cpu")
    with pytest.raises(AssertionError, match="twice"):
        vl.inside_mask(torch.as_strided(buffer, (3, 3), (2, 1), 0), buffer)
    other = vl.sentinel_buffer(4, np.float64, "cpu")
    with pytest.raises(AssertionError):
        vl.inside_mask(torch.as_strided(buffer, (4, 4), (4, 1), 0), other)
