"""Caller-allocated output views for the tests of the C ABI: a rows x cols view of a named layout inside a larger allocation that
is filled with one quiet-NaN bit pattern (both parts for the complex types), and the checks that go with it.

    view, buffer, inside = make_view(rows, cols, dtype, layout, device)

`buffer` is the whole allocation as a flat tensor of `dtype`, `inside` a flat numpy bool mask of the elements the view names.  A call
may write the elements under the mask and nothing else: assert_outside_untouched compares every other element with the sentinel bit
for bit (through an integer view: NaN != NaN, and a NaN of another payload is a write too).  The sentinel also shows an output that
is read before it is written (a beta != 0 product, an accumulation into an uninitialised buffer): the NaN reaches the result, and
assert_inside_written finds an element the call never wrote.

Layouts (strides in elements):
    C   fresh C order, nothing around it: what the Python package passes
    F   Fortran order, contiguous: rs = 1, cs = rows
    FP  column-major interior view: rs = 1, cs = rows + pad with cs ODD, the first element at an ODD element offset from the
        allocation (element-aligned, not 16-byte aligned for every type narrower than 16 bytes), GUARD or more spare elements on all
        four sides
    CP  the row-major twin of FP: cs = 1, rs = cols + pad odd, odd offset, guard band
    S   both strides non-unit: the [1::2, 1::2] slice of a row-major buffer of 2 rows x 2 cols
"""
import numpy as np
import torch

LAYOUTS = ("C", "F", "FP", "CP", "S")
GUARD = 3
# quiet NaNs (exponent all ones, top mantissa bit set) with a payload no arithmetic produces
SENTINEL_BITS = {4: 0x7FC0BEEF, 8: 0x7FF8000000C0FFEE}
_INT = {4: torch.int32, 8: torch.int64}
_NP_INT = {4: np.int32, 8: np.int64}


def torch_dtype(dtype):
    return dtype if isinstance(dtype, torch.dtype) else torch.from_numpy(np.zeros(0, dtype=dtype)).dtype


def real_size(dtype):
    """Bytes of one real part of `dtype`."""
    dt = torch_dtype(dtype)
    return torch.empty(0, dtype=dt).element_size() // (2 if dt.is_complex else 1)


def sentinel_buffer(count, dtype, device):
    """A flat tensor of `count` elements of `dtype`, every real part of which holds the sentinel bits."""
    dt = torch_dtype(dtype)
    rs = real_size(dt)
    raw = torch.full((count * (2 if dt.is_complex else 1),), SENTINEL_BITS[rs], dtype=_INT[rs], device=device)
    real = raw.view(torch.float32 if rs == 4 else torch.float64)
    return torch.view_as_complex(real.view(-1, 2)) if dt.is_complex else real


def bits(t):
    """The elements of a tensor (or numpy array) as a numpy integer array of the same shape (complex: a trailing axis of 2)."""
    a = t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)
    a = np.ascontiguousarray(a)
    if a.dtype.kind == "c":
        a = a.view(a.real.dtype).reshape(a.shape + (2,))
    return a.view(_NP_INT[a.dtype.itemsize])


def _geometry(rows, cols, layout):
    """(count, offset, rs, cs) of the view inside its flat allocation."""
    if layout == "C":
        return rows * cols, 0, cols, 1
    if layout == "F":
        return rows * cols, 0, 1, rows
    if layout in ("FP", "CP"):
        fast, slow = (rows, cols) if layout == "FP" else (cols, rows)
        pitch = fast + 2 * GUARD + 1
        pitch += 1 - pitch % 2                       # odd
        offset = GUARD * pitch + GUARD
        offset += 1 - offset % 2                     # odd: GUARD or GUARD + 1 spare elements in front of every line, GUARD or more behind
        count = (slow + 2 * GUARD) * pitch + 1
        return (count, offset, 1, pitch) if layout == "FP" else (count, offset, pitch, 1)
    if layout == "S":
        return 4 * rows * cols, 2 * cols + 1, 4 * cols, 2
    raise ValueError(layout)


def flat_index(view, buffer):
    """Flat index into `buffer` of every element of `view` (rows x cols numpy int64 array)."""
    esz = buffer.element_size()
    off = (view.data_ptr() - buffer.data_ptr()) // esz
    assert off * esz == view.data_ptr() - buffer.data_ptr()
    i = np.arange(view.shape[0], dtype=np.int64)[:, None]
    j = np.arange(view.shape[1], dtype=np.int64)[None, :]
    return off + i * view.stride(0) + j * view.stride(1)


def inside_mask(view, buffer):
    idx = flat_index(view, buffer)
    assert idx.min(initial=0) >= 0 and idx.max(initial=0) < max(buffer.numel(), 1), "the view leaves its allocation"
    mask = np.zeros(buffer.numel(), dtype=bool)
    mask[idx.ravel()] = True
    assert int(mask.sum()) == idx.size, "the view names an element twice"
    return mask


def assert_layout_properties(view, buffer, layout):
    """What makes a layout the layout it is called: asserted of every view make_view returns, so that a change of the helper (or of
    the allocator's alignment) cannot quietly turn FP / CP into views the vector paths accept."""
    rows, cols = view.shape
    rs, cs = view.stride()
    esz = view.element_size()
    off = (view.data_ptr() - buffer.data_ptr()) // esz
    if layout == "C":
        assert off == 0 and (rs, cs) == (cols, 1) and buffer.numel() == rows * cols
    elif layout == "F":
        assert off == 0 and (rs, cs) == (1, rows) and buffer.numel() == rows * cols
    elif layout in ("FP", "CP"):
        unit, pitch, fast = (rs, cs, rows) if layout == "FP" else (cs, rs, cols)
        assert unit == 1, f"{layout}: unit stride expected along the fast dimension, got {unit}"
        assert pitch % 2 == 1, f"{layout}: the pitch {pitch} is even"
        assert pitch >= fast + 2 * GUARD, f"{layout}: no room for the guard band"
        assert off % 2 == 1, f"{layout}: the element offset {off} is even"
        assert buffer.data_ptr() % 16 == 0, "the allocation itself is not 16-byte aligned"
        if esz < 16:  # a 16-byte element (c64) is 16-byte aligned wherever it lies
            assert view.data_ptr() % 16 != 0, f"{layout}: the view's pointer is 16-byte aligned"
        lead, tail = off % pitch, pitch - fast - off % pitch
        assert lead >= GUARD and tail >= GUARD and off // pitch >= GUARD, f"{layout}: guard band thinner than {GUARD}"
    elif layout == "S":
        assert rs == 4 * cols and cs == 2 and off == 2 * cols + 1 and buffer.numel() == 4 * rows * cols
    else:
        raise ValueError(layout)


def make_view(rows, cols, dtype, layout, device="cuda"):
    """(view, buffer, inside): a rows x cols output view of layout `layout` in a sentinel-filled allocation (see the module text)."""
    count, offset, rs, cs = _geometry(rows, cols, layout)
    buffer = sentinel_buffer(count, dtype, device)
    view = torch.as_strided(buffer, (rows, cols), (rs, cs), offset)
    assert_layout_properties(view, buffer, layout)
    return view, buffer, inside_mask(view, buffer)


def untouched(buffer, inside):
    """Flat bool array: True where an element outside the mask still holds the sentinel bits (True under the mask)."""
    b = bits(buffer)
    same = b == SENTINEL_BITS[b.dtype.itemsize]
    if same.ndim == 2:
        same = same.all(axis=1)
    return same | inside


def assert_outside_untouched(buffer, inside, what="output"):
    ok = untouched(buffer, inside)
    if not ok.all():
        bad = np.nonzero(~ok)[0]
        raise AssertionError(f"{what}: {bad.size} element(s) outside the view were written, flat indices {bad[:8].tolist()} ...")


def written(view):
    """rows x cols bool array: False where an element of the view still holds the sentinel bits in any of its parts."""
    b = bits(view)
    hit = b == SENTINEL_BITS[b.dtype.itemsize]
    return ~(hit.any(axis=-1) if hit.ndim == 3 else hit)


def assert_inside_written(view, what="output"):
    w = written(view)
    if not w.all():
        bad = np.argwhere(~w)
        raise AssertionError(f"{what}: {len(bad)} element(s) of the view were never written, first {bad[:4].tolist()}")
