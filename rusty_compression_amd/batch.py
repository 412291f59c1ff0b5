"""Batches of independent matrices sharded over the GPUs of one node (BASELINE.json configs[4]).

The path shards by MATRIX: matrix i of N goes to rank i // (N / world) (8 per GPU for the
64-matrix config); nothing is exchanged while compressing.  The one exchange step is the
gather of the finished factor blocks (C: m x k, Z: k x n, col_ind: n) to rank 0, one packed,
equal-sized buffer per rank:

  * `Comm` + `gather_packed`: the library's own RCCL path (rc_comm_init / rc_comm_gather, grouped
    ncclSend / ncclRecv over xGMI) -- what a Rust / C++ host uses;
  * `torch.distributed.gather` when a torch process group is active (gloo in the CPU tests).

Per GPU the matrices run through rc_batch_column_id_* (include/rusty_compression_amd.h): spread over
`lanes` contexts / HIP streams and advanced in lock step, one host wait per pivoting panel for all of them.

reference call sequence per matrix (examples/interpolative_decomposition.rs:25-32):
    QR::compute_from(a) -> compress(RANK(k)) -> column_id()
"""
from __future__ import annotations

import ctypes
from typing import Callable, List, Optional, Sequence, Tuple

import numpy as np
import torch


def shard_range(n_items: int, world: int, rank: int) -> range:
    """Contiguous block partition: the first (n_items % world) ranks take one extra item (rc_batch_shard_range)."""
    base, extra = divmod(n_items, world)
    start = rank * base + min(rank, extra)
    return range(start, start + base + (1 if rank < extra else 0))


def column_id_rank(a: torch.Tensor, k: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Rank-k column ID of one matrix through the C ABI (rc_column_id_rank_*)."""
    from . import _lib
    from .types import as_device, empty

    a = as_device(a)
    m, n = a.shape
    k = min(int(k), m, n)
    c, z = empty(m, k, a), empty(k, n, a)
    ind = torch.empty(n, dtype=torch.int64, device=a.device)
    _lib.default_context().call(f"rc_column_id_rank_{_lib.suffix(a.dtype)}", _lib.mat(a), ctypes.c_int64(k), _lib.mat(c), _lib.mat(z), _lib.i64p(ind))
    return c, z, ind


def column_id_rank_batched(a: torch.Tensor, k: int, tol: float = 0.0) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """Column IDs of `count` small same-shaped matrices in one stream-ordered call (rc_column_id_rank_batched_*).

    a: [count, m, n] device tensor of float64, float32, complex128 or complex64, any strides (1 <= m, n <= 512).  k (<= 128) is
    clamped to min(m, n); the rank of each matrix is the first j < k with R_jj == 0 or |R_jj / R_00| < tol (tol = 0: fixed rank k),
    with R_jj real also for complex data (?geqp3's complex Householder QR).  Returns C [count, m, k], Z [count, k, n] (a's dtype),
    ind [count, n] (full permutations, pivots first) and ranks [count]; columns / rows of C / Z past a matrix's rank are zero."""
    from . import _lib
    from .types import as_device

    a = as_device(a).resolve_conj()  # a lazily conjugated complex view is materialised: the kernels read the stored values
    if a.dim() != 3:
        raise AssertionError("expected a [count, m, n] batch")
    count, m, n = a.shape
    kk = min(int(k), m, n)
    c = torch.empty((count, m, kk), dtype=a.dtype, device=a.device)
    z = torch.empty((count, kk, n), dtype=a.dtype, device=a.device)
    ind = torch.empty((count, n), dtype=torch.int64, device=a.device)
    ranks = torch.empty(count, dtype=torch.int64, device=a.device)
    view = _lib.rc_matrix(a.data_ptr(), m, n, a.stride(1), a.stride(2))
    _lib.default_context().call(f"rc_column_id_rank_batched_{_lib.suffix(a.dtype)}", view, ctypes.c_int64(a.stride(0)), ctypes.c_int32(count),
                                ctypes.c_int64(int(k)), ctypes.c_double(float(tol)), _lib.mat(c[0] if count else c.new_empty(m, kk)),
                                ctypes.c_int64(m * kk), _lib.mat(z[0] if count else z.new_empty(kk, n)), ctypes.c_int64(kk * n),
                                _lib.i64p(ind), _lib.i64p(ranks))
    return c, z, ind, ranks


def two_sided_id_rank_batched(a: torch.Tensor, k: int, tol: float = 0.0) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor,
                                                                                torch.Tensor]:
    """Two-sided IDs A ~ C X R of `count` small same-shaped matrices in one stream-ordered call (rc_two_sided_id_rank_batched_*).

    a: [count, m, n] device tensor, any strides (1 <= m, n <= 512).  k (<= 128) is clamped to min(m, n); the rank r of each matrix is
    that of column_id_rank_batched (R_jj == 0 or |R_jj / R_00| < tol; tol = 0: fixed rank k), whose Z and ind are R and col_ind here
    bit for bit.  The row side is the row ID of A[:, col_ind[:r]] (ColumnID::two_sided_id; for complex data the column ID of its
    conjugate transpose, C = Z2^H).  Float64, float32, complex128 and complex64.  Returns C [count, m, k], X [count, k, k],
    R [count, k, n], row_ind [count, m], col_ind [count, n] (full permutations, pivots first) and ranks [count];
    X[:r, :r] = A[row_ind[:r]][:, col_ind[:r]], and the columns of C, rows of R and rows and columns of X past a matrix's rank are zero."""
    from . import _lib
    from .types import as_device

    a = as_device(a).resolve_conj()  # a lazily conjugated complex view is materialised: the kernels read the stored values
    if a.dim() != 3:
        raise AssertionError("expected a [count, m, n] batch")
    count, m, n = a.shape
    kk = min(int(k), m, n)
    c = torch.empty((count, m, kk), dtype=a.dtype, device=a.device)
    x = torch.empty((count, kk, kk), dtype=a.dtype, device=a.device)
    r = torch.empty((count, kk, n), dtype=a.dtype, device=a.device)
    row_ind = torch.empty((count, m), dtype=torch.int64, device=a.device)
    col_ind = torch.empty((count, n), dtype=torch.int64, device=a.device)
    ranks = torch.empty(count, dtype=torch.int64, device=a.device)
    view = _lib.rc_matrix(a.data_ptr(), m, n, a.stride(1), a.stride(2))
    _lib.default_context().call(f"rc_two_sided_id_rank_batched_{_lib.suffix(a.dtype)}", view, ctypes.c_int64(a.stride(0)), ctypes.c_int32(count),
                                ctypes.c_int64(int(k)), ctypes.c_double(float(tol)), _lib.mat(c[0] if count else c.new_empty(m, kk)),
                                ctypes.c_int64(m * kk), _lib.mat(x[0] if count else x.new_empty(kk, kk)), ctypes.c_int64(kk * kk),
                                _lib.mat(r[0] if count else r.new_empty(kk, n)), ctypes.c_int64(kk * n), _lib.i64p(row_ind), _lib.i64p(col_ind),
                                _lib.i64p(ranks))
    return c, x, r, row_ind, col_ind, ranks


def _svd_rank_batched(who: str, complex_data: bool, a, k, tol):
    """The body of svd_rank_batched and svd_rank_batched_complex: the checks and the call; S comes back in the real dtype."""
    from . import _lib
    from .types import as_device

    a = as_device(a).resolve_conj()  # a lazily conjugated complex view is materialised: the kernels read the stored values
    if a.dim() != 3:
        raise AssertionError("expected a [count, m, n] batch")
    kinds = (torch.complex128, torch.complex64) if complex_data else (torch.float64, torch.float32)
    if a.dtype not in kinds:
        raise TypeError(f"{who}: {'complex128 or complex64' if complex_data else 'float64 or float32'} data expected, got {a.dtype}")
    count, m, n = a.shape
    p = min(m, n)
    kk = min(int(k), p)
    u = torch.empty((count, m, kk), dtype=a.dtype, device=a.device)
    s = torch.empty((count, p), dtype=_lib.real_dtype(a.dtype), device=a.device)
    vt = torch.empty((count, kk, n), dtype=a.dtype, device=a.device)
    ranks = torch.empty(count, dtype=torch.int64, device=a.device)
    view = _lib.rc_matrix(a.data_ptr(), m, n, a.stride(1), a.stride(2))
    _lib.default_context().call(f"rc_svd_rank_batched_{_lib.suffix(a.dtype)}", view, ctypes.c_int64(a.stride(0)), ctypes.c_int32(count),
                                ctypes.c_int64(int(k)), ctypes.c_double(float(tol)), _lib.mat(u[0] if count else u.new_empty(m, kk)),
                                ctypes.c_int64(m * kk), ctypes.c_void_p(s.data_ptr()), _lib.mat(vt[0] if count else vt.new_empty(kk, n)),
                                ctypes.c_int64(kk * n), _lib.i64p(ranks))
    return u, s, vt, ranks


def svd_rank_batched(a: torch.Tensor, k: int, tol: float = 0.0) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """Truncated SVDs of `count` small same-shaped matrices in one stream-ordered call (rc_svd_rank_batched_*).

    a: [count, m, n] device tensor of float64 or float32, any strides (1 <= m, n <= 512, min(m, n) <= 128).  k (<= 128) is clamped to
    p = min(m, n); the rank of each matrix is the first j < k with s_j == 0 or s_j / s_0 < tol (tol = 0: fixed rank k).  Returns
    U [count, m, k], S [count, p] (all singular values, descending), Vt [count, k, n] and ranks [count]; the columns of U and rows of
    Vt past a matrix's rank are zero, and the largest-|.| entry of each kept column of U is positive.  Complex data (complex128,
    complex64) goes to svd_rank_batched_complex; this function raises TypeError for it."""
    return _svd_rank_batched("svd_rank_batched", False, a, k, tol)


def svd_rank_batched_complex(a: torch.Tensor, k: int, tol: float = 0.0) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """Truncated SVDs of `count` small same-shaped complex matrices in one stream-ordered call (rc_svd_rank_batched_c64 / _c32).

    a: [count, m, n] device tensor of complex128 or complex64, any strides (1 <= m, n <= 512, min(m, n) <= 128); float64 and float32
    data goes to svd_rank_batched, and this function raises TypeError for it.  The domain, the rank rule and the zero tails are
    svd_rank_batched's.  Returns U [count, m, k] (complex), S [count, p] (the real dtype: float64 for complex128, float32 for
    complex64; all p = min(m, n) singular values, descending), Vt [count, k, n] (complex, the conjugate transpose of V, so that
    U[:, :, :r] S[:, :r] Vt[:, :r, :] is the rank-r truncation) and ranks [count].  Phase rule: in each kept column of U the first of
    its largest-modulus entries is real and positive, its imaginary part exactly 0; conj(a) gives the conjugated U and Vt bit for bit."""
    return _svd_rank_batched("svd_rank_batched_complex", True, a, k, tol)


def lowrank_apply_batched(left: torch.Tensor, right: torch.Tensor, b: Optional[torch.Tensor] = None, mid: Optional[torch.Tensor] = None,
                          s: Optional[torch.Tensor] = None, ranks: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Apply, or rebuild, every block of a batch from its factors in one stream-ordered call (rc_lowrank_apply_batched_*): the
    reference's Apply::dot and to_mat (src/col_interp_decomp.rs:63-65, :134-154, src/two_sided_interp_decomp.rs:62-65, :159-170,
    src/svd.rs:42-55) for the outputs of the batched IDs and SVDs.

    left: [count, m, k], right: [count, k, n], mid: [count, k, k] or None, s: [count, p >= k] of the real dtype or None, ranks:
    [count] int64 or None (every rank is k); device tensors of one scalar type (float64, float32, complex128, complex64), any strides
    (a stride-0 batch dimension shares one operand).  b: [count, n, nrhs], or [count, n] for vectors, or None to reconstruct.  With
    r = ranks[i] clamped to [0, k], block i of the result is left[i][:, :r] mid[i][:r, :r] diag(s[i][:r]) right[i][:r] b[i] (absent
    factors omitted, nothing conjugated); nothing at an index >= r is read.  Returns y: [count, m, nrhs], [count, m] or [count, m, n]."""
    from . import _lib
    from .types import as_device

    ops = {"left": left, "right": right, "b": b, "mid": mid}
    ops = {name: as_device(t).resolve_conj() for name, t in ops.items() if t is not None}  # the kernels read the stored values
    left, right, b, mid = ops["left"], ops["right"], ops.get("b"), ops.get("mid")
    for name, t in ops.items():
        if t.dtype != left.dtype:
            raise TypeError(f"lowrank_apply_batched: {name} is {t.dtype}, left is {left.dtype}")
    if left.dim() != 3 or right.dim() != 3 or (mid is not None and mid.dim() != 3) or (b is not None and b.dim() not in (2, 3)):
        raise AssertionError("expected left [count, m, k], right [count, k, n], mid [count, k, k] and b [count, n, nrhs] or [count, n]")
    count, m, k = left.shape
    n = right.shape[2]
    for name, t in ops.items():
        if t.shape[0] != count:
            raise AssertionError(f"lowrank_apply_batched: {name} holds {t.shape[0]} blocks, left {count}")
    if s is not None:
        s = as_device(s)
        if s.dtype != _lib.real_dtype(left.dtype):
            raise TypeError(f"lowrank_apply_batched: s is {s.dtype}, expected {_lib.real_dtype(left.dtype)}")
        if s.dim() != 2 or s.shape[0] != count or s.shape[1] < k:
            raise AssertionError(f"lowrank_apply_batched: s must be [count, p] with p >= k = {k}")
        if s.stride(1) != 1:
            s = s.contiguous()
    if ranks is not None:
        ranks = as_device(ranks)
        if ranks.dtype != torch.int64:
            raise TypeError(f"lowrank_apply_batched: ranks is {ranks.dtype}, expected torch.int64")
        if ranks.shape != (count,):
            raise AssertionError("lowrank_apply_batched: ranks must be [count]")
        ranks = ranks.contiguous()
    vector = b is not None and b.dim() == 2
    if vector:
        b = b.unsqueeze(2)
    ncols = n if b is None else b.shape[2]
    y = torch.empty((count, m, ncols), dtype=left.dtype, device=left.device)

    def view(t):  # block 0's view and the batch stride
        if t is None:
            return _lib.mat(None), ctypes.c_int64(0)
        return _lib.rc_matrix(t.data_ptr(), t.shape[1], t.shape[2], t.stride(1), t.stride(2)), ctypes.c_int64(t.stride(0))

    _lib.default_context().call(f"rc_lowrank_apply_batched_{_lib.suffix(left.dtype)}", *view(left), *view(mid),
                                ctypes.c_void_p(s.data_ptr() if s is not None else None), ctypes.c_int64(s.stride(0) if s is not None else 0),
                                *view(right), _lib.i64p(ranks), ctypes.c_int32(count), *view(b),
                                _lib.rc_matrix(y.data_ptr(), m, ncols, ncols, 1), ctypes.c_int64(m * ncols))
    return y[:, :, 0] if vector else y


def column_id_apply_batched(c: torch.Tensor, z: torch.Tensor, ranks: Optional[torch.Tensor], b: Optional[torch.Tensor] = None) -> torch.Tensor:
    """ColumnID dot / to_mat for the outputs of column_id_rank_batched: C[:, :r] Z[:r] b per block, or C[:, :r] Z[:r] with b = None."""
    return lowrank_apply_batched(c, z, b=b, ranks=ranks)


def two_sided_id_apply_batched(c: torch.Tensor, x: torch.Tensor, r: torch.Tensor, ranks: Optional[torch.Tensor],
                               b: Optional[torch.Tensor] = None) -> torch.Tensor:
    """TwoSidedID dot / to_mat for the outputs of two_sided_id_rank_batched: C X R b per block at its rank, or C X R with b = None."""
    return lowrank_apply_batched(c, r, b=b, mid=x, ranks=ranks)


def svd_apply_batched(u: torch.Tensor, s: torch.Tensor, vt: torch.Tensor, ranks: Optional[torch.Tensor], b: Optional[torch.Tensor] = None) -> torch.Tensor:
    """SVD dot / to_mat for the outputs of svd_rank_batched / svd_rank_batched_complex: U diag(s) Vt b per block at its rank, or U diag(s) Vt
    with b = None; s is the [count, p] tensor those calls return, read with row stride p."""
    return lowrank_apply_batched(u, vt, b=b, s=s, ranks=ranks)


def block_csr(rows, cols, block_ids, group_rows=None, group_cols=None):
    """The block-CSR pattern of rc_block_operator_apply_* and its transposed twin, built on the host with NumPy.

    Entry e of the input places block block_ids[e] with its first row at rows[e] (a row of y) and its first column at cols[e] (a row of
    x).  Returns (pattern, pattern_t), each a tuple (group_ptr, group_row, entry_block, entry_col) of int64 arrays.  pattern groups the
    entries by row: one group per distinct value of rows in ascending order, or one per element of group_rows when given (a value of
    group_rows that no entry has gives an empty group; every entry's row must be listed).  Within a group the entries keep the order
    of the input, which is the order the kernel sums them in.  pattern_t groups the same entries by column (group_cols likewise), its
    entry_col holding the rows: with the transposed views of the blocks it is the pattern of A^T x / A^H x."""
    import numpy as np

    rows, cols, ids = (np.asarray(v, dtype=np.int64).reshape(-1) for v in (rows, cols, block_ids))
    if not (rows.shape == cols.shape == ids.shape):
        raise AssertionError("block_csr: rows, cols and block_ids must have one value per entry")

    def grouped(first, other, listed):
        if listed is None:
            heads = np.unique(first)
        else:
            heads = np.asarray(listed, dtype=np.int64).reshape(-1)
            if np.unique(heads).size != heads.size:
                raise AssertionError("block_csr: a group is listed twice")
        order = np.argsort(heads, kind="stable")
        pos = np.searchsorted(heads[order], first)
        if first.size and (np.any(pos >= heads.size) or np.any(heads[order][np.minimum(pos, heads.size - 1)] != first)):
            raise AssertionError("block_csr: an entry belongs to no listed group")
        group_of = order[pos] if first.size else pos  # the group of every entry, in the order of `heads`
        perm = np.argsort(group_of, kind="stable")    # entries by group, input order inside a group
        ptr = np.zeros(heads.size + 1, dtype=np.int64)
        np.cumsum(np.bincount(group_of, minlength=heads.size), out=ptr[1:])
        return ptr, heads.copy(), ids[perm].copy(), other[perm].copy()

    return grouped(rows, cols, group_rows), grouped(cols, rows, group_cols)


class _BlockOperatorCall:
    """The checked operands of rc_block_operator_apply_* on the device, ready to be applied to any x and y (block_operator_apply, the
    products of operator.BlockLowRankOperator): keeps the tensors alive and builds the argument list of the C call."""

    def __init__(self, who, pattern, left=None, right=None, mid=None, s=None, ranks=None, dense=None):
        from . import _lib
        from .types import as_device, as_index

        ops = {"left": left, "right": right, "mid": mid, "dense": dense}
        ops = {name: as_device(t).resolve_conj() for name, t in ops.items() if t is not None}  # the kernels read the stored values
        if ("left" in ops) != ("right" in ops):
            raise AssertionError(f"{who}: left and right come together")
        if "left" not in ops and "dense" not in ops:
            raise AssertionError(f"{who}: needs a low-rank batch (left, right), a dense batch, or both")
        if "left" not in ops and (mid is not None or s is not None or ranks is not None):
            raise AssertionError(f"{who}: mid, s and ranks belong to a low-rank batch")
        first = ops["left"] if "left" in ops else ops["dense"]
        self.dtype = first.dtype
        for name, t in ops.items():
            if t.dtype != self.dtype:
                raise TypeError(f"{who}: {name} is {t.dtype}, expected {self.dtype}")
            if t.dim() != 3:
                raise AssertionError(f"{who}: {name} must be a [count, rows, cols] batch")
        self.left, self.right, self.mid, self.dense = ops.get("left"), ops.get("right"), ops.get("mid"), ops.get("dense")
        self.count = self.left.shape[0] if self.left is not None else 0
        for name in ("right", "mid"):
            if name in ops and ops[name].shape[0] != self.count:
                raise AssertionError(f"{who}: {name} holds {ops[name].shape[0]} blocks, left {self.count}")
        self.m, self.n = (self.left.shape[1], self.right.shape[2]) if self.left is not None else self.dense.shape[1:]
        self.s = self.ranks = None
        if s is not None:
            k = self.left.shape[2]
            s = as_device(s)
            if s.dtype != _lib.real_dtype(self.dtype):
                raise TypeError(f"{who}: s is {s.dtype}, expected {_lib.real_dtype(self.dtype)}")
            if s.dim() != 2 or s.shape[0] != self.count or s.shape[1] < k:
                raise AssertionError(f"{who}: s must be [count, p] with p >= k = {k}")
            self.s = s if s.stride(1) == 1 else s.contiguous()
        if ranks is not None:
            ranks = as_device(ranks)
            if ranks.dtype != torch.int64:
                raise TypeError(f"{who}: ranks is {ranks.dtype}, expected torch.int64")
            if ranks.shape != (self.count,):
                raise AssertionError(f"{who}: ranks must be [count]")
            self.ranks = ranks.contiguous()
        self.pattern = tuple(as_index(v) for v in pattern)
        group_ptr, group_row, entry_block, entry_col = self.pattern
        self.groups = int(group_row.numel())
        if group_ptr.numel() != self.groups + 1 or entry_block.numel() != entry_col.numel():
            raise AssertionError(f"{who}: group_ptr needs groups + 1 values, entry_block and entry_col one per entry")
        self.name = f"rc_block_operator_apply_{_lib.suffix(self.dtype)}"

    def args(self, xv, yv, accumulate=False, conj=False):
        """The arguments after ctx: xv and yv are rc_matrix views of x (N x nrhs) and y (M x nrhs)."""
        from . import _lib

        def view(t):  # block 0's view and the batch stride
            if t is None:
                return _lib.mat(None), ctypes.c_int64(0)
            return _lib.rc_matrix(t.data_ptr(), t.shape[1], t.shape[2], t.stride(1), t.stride(2)), ctypes.c_int64(t.stride(0))

        s = self.s
        group_ptr, group_row, entry_block, entry_col = self.pattern
        return (*view(self.left), *view(self.mid), ctypes.c_void_p(s.data_ptr() if s is not None else None),
                ctypes.c_int64(s.stride(0) if s is not None else 0), *view(self.right), _lib.i64p(self.ranks), ctypes.c_int32(self.count),
                *view(self.dense), ctypes.c_int32(self.dense.shape[0] if self.dense is not None else 0), _lib.i64p(group_ptr), _lib.i64p(group_row),
                ctypes.c_int32(self.groups), _lib.i64p(entry_block), _lib.i64p(entry_col), xv, yv, ctypes.c_int32(1 if accumulate else 0),
                ctypes.c_int32(1 if conj else 0))

    def apply(self, x, y=None, rows=None, accumulate=False, conj=False):
        from . import _lib
        from .types import as_device

        x = as_device(x).resolve_conj()
        if x.dtype != self.dtype:
            raise TypeError(f"{self.name}: x is {x.dtype}, expected {self.dtype}")
        vector = x.dim() == 1
        x2 = x.unsqueeze(1) if vector else x
        if y is None:
            if rows is None:
                raise AssertionError("block_operator_apply: give y, or rows (the number of rows of y)")
            y = torch.zeros((int(rows), x2.shape[1]), dtype=self.dtype, device=x.device)  # rows of no group stay zero
            out = y[:, 0] if vector else y
        else:
            if not (isinstance(y, torch.Tensor) and y.is_cuda and y.dtype == self.dtype and y.dim() == x.dim()):
                raise AssertionError("block_operator_apply: y must be a device tensor of x's dtype and rank")
            out = y
            y = y.unsqueeze(1) if vector else y
        _lib.default_context().call(self.name, *self.args(_lib.mat(x2), _lib.mat(y), accumulate, conj))
        return out


def block_operator_apply(x: torch.Tensor, group_ptr, group_row, entry_block, entry_col, left: Optional[torch.Tensor] = None,
                         right: Optional[torch.Tensor] = None, mid: Optional[torch.Tensor] = None, s: Optional[torch.Tensor] = None,
                         ranks: Optional[torch.Tensor] = None, dense: Optional[torch.Tensor] = None, y: Optional[torch.Tensor] = None,
                         rows: Optional[int] = None, accumulate: bool = False, conj: bool = False) -> torch.Tensor:
    """y = H x for the block-sparse operator whose blocks are a batch of low-rank factors and / or a batch of dense blocks, in one
    stream-ordered call (rc_block_operator_apply_*): the gather of x, lowrank_apply_batched and the scatter-add into y without
    atomics and without the two intermediate buffers.

    left [count, m, k], right [count, k, n], mid, s and ranks are the operands of lowrank_apply_batched; dense is [dense_count, m, n]
    or None.  Block ids 0 .. count - 1 are the low-rank blocks, count .. count + dense_count - 1 the dense ones.  (group_ptr,
    group_row, entry_block, entry_col) is the block-CSR pattern (block_csr builds it): group g owns rows group_row[g] .. + m - 1 of y
    and sums, in order, the entries group_ptr[g] .. group_ptr[g + 1] - 1; entry e is block entry_block[e] applied to rows
    entry_col[e] .. + n - 1 of x.  x is [N, nrhs] or [N].  y ([M, nrhs] or [M], any strides) is written in place when given, else a
    zero-filled [rows, nrhs] result is returned; rows of no group are not touched.  accumulate adds to y instead of overwriting the
    groups' rows; conj conjugates the blocks (not x) as they are loaded, a no-op for real data.  The row ranges of two groups must
    not overlap.  An out-of-range block id, entry_col or group_row is skipped on the device and sets bit 64 of the health word
    (Context.get_health)."""
    call = _BlockOperatorCall("block_operator_apply", (group_ptr, group_row, entry_block, entry_col), left, right, mid, s, ranks, dense)
    return call.apply(x, y=y, rows=rows, accumulate=accumulate, conj=conj)


# mixed-precision storage: the factors of a compressed batch in the narrow type, everything else in the wide one
_MIXED_WIDE = {torch.float32: torch.float64, torch.complex64: torch.complex128}
_MIXED_STORAGE = {wide: narrow for narrow, wide in _MIXED_WIDE.items()}


def _mixed_wide_dtype(who: str, same: str, factors: dict) -> torch.dtype:
    """The compute dtype of the storage dtype the factors of a mixed call share; TypeError for anything but float32 / complex64 factors."""
    first = next(iter(factors.values()))
    for name, t in factors.items():
        if t.dtype != first.dtype:
            raise TypeError(f"{who}: {name} is {t.dtype}, the other factors are {first.dtype}")
    if first.dtype not in _MIXED_WIDE:
        raise TypeError(f"{who}: the factors must be stored in float32 (with float64 vectors) or complex64 (with complex128 vectors), got "
                        f"{first.dtype}; use {same} when every operand has one dtype")
    return _MIXED_WIDE[first.dtype]


def _convert_batched(who: str, x: torch.Tensor, table: dict, stem: str, return_overflow: bool):
    from . import _lib
    from .types import as_device

    x = as_device(x).resolve_conj()
    if x.dtype not in table:
        raise TypeError(f"{who}: x is {x.dtype}, expected one of {sorted(str(d) for d in table)}")
    if x.dim() != 3:
        raise AssertionError(f"{who}: expected a [count, rows, cols] batch")
    count, rows, cols = x.shape
    out = torch.empty((count, rows, cols), dtype=table[x.dtype], device=x.device)
    overflow = torch.zeros(count, dtype=torch.int64, device=x.device) if return_overflow else None
    blank = x.new_empty(rows, cols)  # block 0 of an empty batch: the shapes are still checked
    args = [_lib.mat(x[0] if count else blank), ctypes.c_int64(x.stride(0)), ctypes.c_int32(count),
            _lib.mat(out[0] if count else out.new_empty(rows, cols)), ctypes.c_int64(rows * cols)]
    if stem == "rc_demote_batched":
        args.append(_lib.i64p(overflow))
    _lib.default_context().call(f"{stem}_{_lib.suffix(x.dtype)}", *args)
    return (out, overflow) if return_overflow else out


def demote_batched(x: torch.Tensor, return_overflow: bool = False):
    """The storage copy of a factor batch for the mixed calls (rc_demote_batched_f64 / _c64): x [count, rows, cols] of float64 or
    complex128, any strides, rounded to nearest even into a fresh contiguous float32 / complex64 tensor, the bits of NumPy's astype.  With
    return_overflow also an int64 [count] tensor: per block the finite elements that became infinite."""
    return _convert_batched("demote_batched", x, _MIXED_STORAGE, "rc_demote_batched", return_overflow)


def promote_batched(x: torch.Tensor) -> torch.Tensor:
    """The exact inverse direction (rc_promote_batched_f32 / _c32): x [count, rows, cols] of float32 or complex64 widened into a fresh
    contiguous float64 / complex128 tensor."""
    return _convert_batched("promote_batched", x, _MIXED_WIDE, "rc_promote_batched", False)


def lowrank_apply_batched_mixed(left: torch.Tensor, right: torch.Tensor, b: Optional[torch.Tensor] = None, mid: Optional[torch.Tensor] = None,
                                s: Optional[torch.Tensor] = None, ranks: Optional[torch.Tensor] = None) -> torch.Tensor:
    """lowrank_apply_batched for factors kept in storage precision (rc_lowrank_apply_mixed_batched_f64 / _c64): left, mid and right are
    float32 with b and s float64, or complex64 with b complex128 and s float64.  Every factor element is widened exactly as it is loaded
    and the arithmetic is the wide call's, so the result (float64 / complex128, also when reconstructing with b = None) has the bits of
    lowrank_apply_batched on promote_batched copies of the factors, while the launch reads half the factor bytes.  Shapes, strides, ranks
    and the returned shapes are lowrank_apply_batched's.  Any other combination of dtypes raises TypeError."""
    from . import _lib
    from .types import as_device

    who = "lowrank_apply_batched_mixed"
    fac = {"left": left, "right": right, "mid": mid}
    fac = {name: as_device(t).resolve_conj() for name, t in fac.items() if t is not None}  # the kernels read the stored values
    left, right, mid = fac["left"], fac["right"], fac.get("mid")
    wide = _mixed_wide_dtype(who, "lowrank_apply_batched", fac)
    if b is not None:
        b = as_device(b).resolve_conj()
        if b.dtype != wide:
            raise TypeError(f"{who}: b is {b.dtype}, expected {wide} beside {left.dtype} factors")
    if left.dim() != 3 or right.dim() != 3 or (mid is not None and mid.dim() != 3) or (b is not None and b.dim() not in (2, 3)):
        raise AssertionError("expected left [count, m, k], right [count, k, n], mid [count, k, k] and b [count, n, nrhs] or [count, n]")
    count, m, k = left.shape
    n = right.shape[2]
    for name, t in {**fac, **({"b": b} if b is not None else {})}.items():
        if t.shape[0] != count:
            raise AssertionError(f"{who}: {name} holds {t.shape[0]} blocks, left {count}")
    if s is not None:
        s = as_device(s)
        if s.dtype != torch.float64:
            raise TypeError(f"{who}: s is {s.dtype}, expected torch.float64")
        if s.dim() != 2 or s.shape[0] != count or s.shape[1] < k:
            raise AssertionError(f"{who}: s must be [count, p] with p >= k = {k}")
        if s.stride(1) != 1:
            s = s.contiguous()
    if ranks is not None:
        ranks = as_device(ranks)
        if ranks.dtype != torch.int64:
            raise TypeError(f"{who}: ranks is {ranks.dtype}, expected torch.int64")
        if ranks.shape != (count,):
            raise AssertionError(f"{who}: ranks must be [count]")
        ranks = ranks.contiguous()
    vector = b is not None and b.dim() == 2
    if vector:
        b = b.unsqueeze(2)
    ncols = n if b is None else b.shape[2]
    y = torch.empty((count, m, ncols), dtype=wide, device=left.device)

    def view(t):  # block 0's view and the batch stride
        if t is None:
            return _lib.mat(None), ctypes.c_int64(0)
        return _lib.rc_matrix(t.data_ptr(), t.shape[1], t.shape[2], t.stride(1), t.stride(2)), ctypes.c_int64(t.stride(0))

    _lib.default_context().call(f"rc_lowrank_apply_mixed_batched_{_lib.suffix(wide)}", *view(left), *view(mid),
                                ctypes.c_void_p(s.data_ptr() if s is not None else None), ctypes.c_int64(s.stride(0) if s is not None else 0),
                                *view(right), _lib.i64p(ranks), ctypes.c_int32(count), *view(b),
                                _lib.rc_matrix(y.data_ptr(), m, ncols, ncols, 1), ctypes.c_int64(m * ncols))
    return y[:, :, 0] if vector else y


class _MixedBlockOperatorCall(_BlockOperatorCall):
    """_BlockOperatorCall for rc_block_operator_apply_mixed_*: left, mid and right in the storage dtype, dense, x and y in the wide one (the
    call's dtype), s float64.  The argument list and apply are the base class's."""

    def __init__(self, who, pattern, left=None, right=None, mid=None, s=None, ranks=None, dense=None):
        from . import _lib
        from .types import as_device, as_index

        fac = {"left": left, "right": right, "mid": mid}
        fac = {name: as_device(t).resolve_conj() for name, t in fac.items() if t is not None}  # the kernels read the stored values
        if "left" not in fac or "right" not in fac:
            raise AssertionError(f"{who}: needs a low-rank batch (left, right) in storage precision; a dense-only operator has nothing to demote")
        self.dtype = _mixed_wide_dtype(who, "block_operator_apply", fac)
        if dense is not None:
            dense = as_device(dense).resolve_conj()
            if dense.dtype != self.dtype:
                raise TypeError(f"{who}: dense is {dense.dtype}, expected {self.dtype} (near-field blocks stay in full precision)")
        for name, t in {**fac, **({"dense": dense} if dense is not None else {})}.items():
            if t.dim() != 3:
                raise AssertionError(f"{who}: {name} must be a [count, rows, cols] batch")
        self.left, self.right, self.mid, self.dense = fac["left"], fac["right"], fac.get("mid"), dense
        self.count = self.left.shape[0]
        for name in ("right", "mid"):
            if name in fac and fac[name].shape[0] != self.count:
                raise AssertionError(f"{who}: {name} holds {fac[name].shape[0]} blocks, left {self.count}")
        self.m, self.n = self.left.shape[1], self.right.shape[2]
        self.s = self.ranks = None
        if s is not None:
            k = self.left.shape[2]
            s = as_device(s)
            if s.dtype != torch.float64:
                raise TypeError(f"{who}: s is {s.dtype}, expected torch.float64")
            if s.dim() != 2 or s.shape[0] != self.count or s.shape[1] < k:
                raise AssertionError(f"{who}: s must be [count, p] with p >= k = {k}")
            self.s = s if s.stride(1) == 1 else s.contiguous()
        if ranks is not None:
            ranks = as_device(ranks)
            if ranks.dtype != torch.int64:
                raise TypeError(f"{who}: ranks is {ranks.dtype}, expected torch.int64")
            if ranks.shape != (self.count,):
                raise AssertionError(f"{who}: ranks must be [count]")
            self.ranks = ranks.contiguous()
        self.pattern = tuple(as_index(v) for v in pattern)
        group_ptr, group_row, entry_block, entry_col = self.pattern
        self.groups = int(group_row.numel())
        if group_ptr.numel() != self.groups + 1 or entry_block.numel() != entry_col.numel():
            raise AssertionError(f"{who}: group_ptr needs groups + 1 values, entry_block and entry_col one per entry")
        self.name = f"rc_block_operator_apply_mixed_{_lib.suffix(self.dtype)}"


def block_operator_apply_mixed(x: torch.Tensor, group_ptr, group_row, entry_block, entry_col, left: Optional[torch.Tensor] = None,
                               right: Optional[torch.Tensor] = None, mid: Optional[torch.Tensor] = None, s: Optional[torch.Tensor] = None,
                               ranks: Optional[torch.Tensor] = None, dense: Optional[torch.Tensor] = None, y: Optional[torch.Tensor] = None,
                               rows: Optional[int] = None, accumulate: bool = False, conj: bool = False) -> torch.Tensor:
    """block_operator_apply for low-rank blocks kept in storage precision (rc_block_operator_apply_mixed_f64 / _c64): left, mid and right
    are float32 (complex64); dense, x and y are float64 (complex128) and s float64.  The result has the bits of block_operator_apply on
    promote_batched copies of the factors; every other argument and rule is block_operator_apply's."""
    call = _MixedBlockOperatorCall("block_operator_apply_mixed", (group_ptr, group_row, entry_block, entry_col), left, right, mid, s, ranks, dense)
    return call.apply(x, y=y, rows=rows, accumulate=accumulate, conj=conj)


def _lowrank_recompress_batched(who: str, complex_data: bool, left, right, k, tol, mid, s, ranks, tall=False):
    """The shared body of lowrank_recompress_batched, lowrank_recompress_tall_batched, lowrank_recompress_large_batched (real dtypes; tall:
    False, True for the entry points with m <= 65536, or "large" for those with m, n <= 65536), lowrank_recompress_batched_complex,
    lowrank_recompress_tall_batched_complex and lowrank_recompress_large_batched_complex (complex dtypes, real s and S, the same values of tall)."""
    from . import _lib
    from .types import as_device

    ops = {"left": left, "right": right, "mid": mid}
    ops = {name: as_device(t) for name, t in ops.items() if t is not None}
    if complex_data:
        ops = {name: t.resolve_conj() for name, t in ops.items()}  # the kernels read the stored values
    left, right, mid = ops["left"], ops["right"], ops.get("mid")
    kinds = (torch.complex128, torch.complex64) if complex_data else (torch.float64, torch.float32)
    if left.dtype not in kinds:
        raise TypeError(f"{who}: {' or '.join(str(t).replace('torch.', '') for t in kinds)} data expected, got {left.dtype}")
    for name, t in ops.items():
        if t.dtype != left.dtype:
            raise TypeError(f"{who}: {name} is {t.dtype}, left is {left.dtype}")
    real = _lib.real_dtype(left.dtype)
    if s is not None:
        s = as_device(s)
        if s.dtype != real:
            raise TypeError(f"{who}: s is {s.dtype}, expected {real}" if complex_data else f"{who}: s is {s.dtype}, left is {left.dtype}")
        ops["s"] = s
    if left.dim() != 3 or right.dim() != 3 or (mid is not None and mid.dim() != 3):
        raise AssertionError("expected left [count, m, K], right [count, K, n] and mid [count, K, K]")
    count, m, kin = left.shape
    n = right.shape[2]
    for name, t in ops.items():
        if t.shape[0] != count:
            raise AssertionError(f"{who}: {name} holds {t.shape[0]} blocks, left {count}")
    if s is not None:
        if s.dim() != 2 or s.shape[1] < kin:
            raise AssertionError(f"{who}: s must be [count, p] with p >= K = {kin}")
        if s.stride(1) != 1:
            s = s.contiguous()
    if ranks is not None:
        ranks = as_device(ranks)
        if ranks.dtype != torch.int64:
            raise TypeError(f"{who}: ranks is {ranks.dtype}, expected torch.int64")
        if ranks.shape != (count,):
            raise AssertionError(f"{who}: ranks must be [count]")
        ranks = ranks.contiguous()
    kk = max(min(int(k), kin), 0)
    u = torch.empty((count, m, kk), dtype=left.dtype, device=left.device)
    s_out = torch.empty((count, kin), dtype=real, device=left.device)
    vt = torch.empty((count, kk, n), dtype=left.dtype, device=left.device)
    out_ranks = torch.empty(count, dtype=torch.int64, device=left.device)

    def view(t):  # block 0's view and the batch stride
        if t is None:
            return _lib.mat(None), ctypes.c_int64(0)
        return _lib.rc_matrix(t.data_ptr(), t.shape[1], t.shape[2], t.stride(1), t.stride(2)), ctypes.c_int64(t.stride(0))

    # the complex entry points spell their stem differently (see the header) and take tol in the real type of the data
    stem = {(False, False): "rc_lowrank_recompress_batched_", (False, True): "rc_lowrank_recompress_tall_batched_",
            (False, "large"): "rc_lowrank_recompress_large_batched_", (True, False): "rc_lowrank_recompress_complex_batched_",
            (True, True): "rc_lowrank_recompress_tall_complex_batched_",
            (True, "large"): "rc_lowrank_recompress_complex_large_batched_"}[(complex_data, tall)]
    tol_arg = ctypes.c_float(float(tol)) if left.dtype == torch.complex64 else ctypes.c_double(float(tol))
    _lib.default_context().call(stem + _lib.suffix(left.dtype), *view(left), *view(mid),
                                ctypes.c_void_p(s.data_ptr() if s is not None else None), ctypes.c_int64(s.stride(0) if s is not None else 0),
                                *view(right), _lib.i64p(ranks), ctypes.c_int32(count), ctypes.c_int64(int(k)), tol_arg,
                                _lib.rc_matrix(u.data_ptr(), m, kk, kk, 1), ctypes.c_int64(m * kk), ctypes.c_void_p(s_out.data_ptr()),
                                _lib.rc_matrix(vt.data_ptr(), kk, n, n, 1), ctypes.c_int64(kk * n), _lib.i64p(out_ranks))
    return u, s_out, vt, out_ranks


def lowrank_recompress_batched(left: torch.Tensor, right: torch.Tensor, k: int, tol: float = 0.0, mid: Optional[torch.Tensor] = None,
                               s: Optional[torch.Tensor] = None,
                               ranks: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """Recompress every factor pair of a batch to a truncated SVD without forming the blocks, in one stream-ordered call
    (rc_lowrank_recompress_batched_*): the scheme of the reference's SVD::to_qr / compute_from_range_estimate (src/svd.rs:150-163, :171-)
    with compress's rank rule (src/svd.rs:60-101).

    left: [count, m, K], right: [count, K, n], mid: [count, K, K] or None, s: [count, p >= K] or None, ranks: [count] int64 or None
    (every inner rank is K); float64 or float32 device tensors, any strides (a stride-0 batch dimension shares one operand);
    K <= min(m, n), K <= 128, m, n <= 512.  With q = ranks[i] clamped to [0, K], block i is A_i = left[i][:, :q] mid[i][:q, :q]
    diag(s[i][:q]) right[i][:q] (absent factors omitted; nothing at an index >= q is read).  Returns U [count, m, kk], S [count, K]
    (the q singular values of A_i, descending, then zeros), Vt [count, kk, n] and the new ranks [count], kk = min(k, K): the rank of a
    block is the first j < min(kk, q) with s_j == 0 or s_j / s_0 < tol, else min(kk, q); columns of U and rows of Vt past it are zero
    and the largest-|.| entry of each kept column of U is positive.  Complex data raises TypeError (see lowrank_recompress_batched_complex).

    Input scale (this call and every other recompression of this module, real and complex): each operand present may have its largest
    component anywhere in [2^-100, 2^100] (float32 / complex64) or [2^-900, 2^900] (float64 / complex128), and so may the sum of the
    operands' exponents.  Every operand is normalised by an exact power of two on loading and S takes the product back: scaling an operand
    by 2^e scales S by 2^e and leaves U, Vt and the ranks unchanged bit for bit, so the C of a column ID, the X of a two-sided ID and the
    s of an SVD of a block at 2^e recompress as those of the unit-scale block."""
    return _lowrank_recompress_batched("lowrank_recompress_batched", False, left, right, k, tol, mid, s, ranks)


def lowrank_recompress_batched_complex(left: torch.Tensor, right: torch.Tensor, k: int, tol: float = 0.0, mid: Optional[torch.Tensor] = None,
                                       s: Optional[torch.Tensor] = None,
                                       ranks: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """lowrank_recompress_batched for complex factors (rc_lowrank_recompress_complex_batched_c64 / _c32): left, right and mid complex128 or
    complex64 device tensors of one dtype (lazily conjugated views are materialised), s of the matching real dtype; real data, mismatched
    dtypes and a complex s raise TypeError.  Nothing is conjugated: A_i = left[i][:, :q] mid[i][:q, :q] diag(s[i][:q]) right[i][:q].
    Returns U [count, m, kk] (complex), S [count, K] (the real dtype), Vt [count, kk, n] (complex, the conjugate transpose of V, so that
    U[:, :, :r] S[:, :r] Vt[:, :r, :] is the rank-r truncation) and the new ranks.  Phase rule of svd_rank_batched_complex: in each kept
    column of U the first of its largest-modulus entries is real and positive, its imaginary part exactly 0; conjugated inputs give the
    conjugated U and Vt bit for bit.  For complex64 data tol is rounded to float32."""
    return _lowrank_recompress_batched("lowrank_recompress_batched_complex", True, left, right, k, tol, mid, s, ranks)


def column_id_to_svd_batched(c: torch.Tensor, z: torch.Tensor, ranks: Optional[torch.Tensor], k: int,
                             tol: float = 0.0) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """Truncated SVDs of the blocks C[:, :r] Z[:r] held by the outputs of column_id_rank_batched, each at its own rank."""
    return lowrank_recompress_batched(c, z, k, tol, ranks=ranks)


def two_sided_id_to_svd_batched(c: torch.Tensor, x: torch.Tensor, r: torch.Tensor, ranks: Optional[torch.Tensor], k: int,
                                tol: float = 0.0) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """Truncated SVDs of the blocks C X R held by the outputs of two_sided_id_rank_batched, each at its own rank."""
    return lowrank_recompress_batched(c, r, k, tol, mid=x, ranks=ranks)


def svd_add_batched(u1: torch.Tensor, s1: torch.Tensor, vt1: torch.Tensor, u2: torch.Tensor, s2: torch.Tensor, vt2: torch.Tensor, k: int,
                    tol: float = 0.0) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """Rounded addition of two batches of truncated SVDs (the outputs of svd_rank_batched or of this module's recompressions):
    block i of the result is the SVD of U1 diag(s1) Vt1 + U2 diag(s2) Vt2, truncated to rank <= k by tol.  The factors are concatenated
    to inner width K = k1 + k2 (K <= min(m, n), K <= 128) and recompressed; columns of U1, U2 past a block's rank are zero, as the
    batched SVD writes them, and come out as exactly zero singular values."""
    k1, k2 = u1.shape[2], u2.shape[2]
    left = torch.cat([u1, u2], dim=2)
    right = torch.cat([vt1, vt2], dim=1)
    s = torch.cat([s1[:, :k1], s2[:, :k2]], dim=1)
    return lowrank_recompress_batched(left, right, k, tol, s=s)


def lowrank_recompress_tall_batched(left: torch.Tensor, right: torch.Tensor, k: int, tol: float = 0.0, mid: Optional[torch.Tensor] = None,
                                    s: Optional[torch.Tensor] = None,
                                    ranks: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """Recompress every factor pair of a batch whose left factor is tall to a truncated SVD without forming the blocks, in one
    stream-ordered call (rc_lowrank_recompress_tall_batched_*): lowrank_recompress_batched's scheme with the left factor taken through a
    flat Householder TSQR in stages of 512 rows inside the launch.

    left: [count, m, K], right: [count, K, n], mid: [count, K, K] or None, s: [count, p >= K] or None, ranks: [count] int64 or None
    (every inner rank is K); float64 or float32 device tensors, any strides (a stride-0 batch dimension shares one operand);
    K <= min(m, n), K <= 128, m <= 65536, n <= 512.  With q = ranks[i] clamped to [0, K], block i is A_i = left[i][:, :q] mid[i][:q, :q]
    diag(s[i][:q]) right[i][:q] (absent factors omitted; nothing at an index >= q is read).  Returns U [count, m, kk], S [count, K]
    (the q singular values of A_i, descending, then zeros), Vt [count, kk, n] and the new ranks [count], kk = min(k, K): the rank of a
    block is the first j < min(kk, q) with s_j == 0 or s_j / s_0 < tol, else min(kk, q); columns of U and rows of Vt past it are zero
    and the largest-|.| entry of each kept column of U, over all m rows, is positive.  For m <= 512 the outputs are
    lowrank_recompress_batched's bit for bit.  A wide pair (tall right) is the transpose: pass right.mT, mid.mT, left.mT and swap
    U.mT / Vt.mT.  Complex data raises TypeError (see lowrank_recompress_tall_batched_complex)."""
    return _lowrank_recompress_batched("lowrank_recompress_tall_batched", False, left, right, k, tol, mid, s, ranks, tall=True)


def column_id_to_svd_tall_batched(c: torch.Tensor, z: torch.Tensor, ranks: Optional[torch.Tensor], k: int,
                                  tol: float = 0.0) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """Truncated SVDs of the tall blocks C[:, :r] Z[:r] held by the outputs of sketch_column_id_rank_batched, each at its own rank."""
    return lowrank_recompress_tall_batched(c, z, k, tol, ranks=ranks)


def svd_add_tall_batched(u1: torch.Tensor, s1: torch.Tensor, vt1: torch.Tensor, u2: torch.Tensor, s2: torch.Tensor, vt2: torch.Tensor, k: int,
                         tol: float = 0.0) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """svd_add_batched for tall blocks (m <= 65536): the rounded sum of two batches of truncated SVDs through lowrank_recompress_tall_batched."""
    k1, k2 = u1.shape[2], u2.shape[2]
    left = torch.cat([u1, u2], dim=2)
    right = torch.cat([vt1, vt2], dim=1)
    s = torch.cat([s1[:, :k1], s2[:, :k2]], dim=1)
    return lowrank_recompress_tall_batched(left, right, k, tol, s=s)


def lowrank_recompress_large_batched(left: torch.Tensor, right: torch.Tensor, k: int, tol: float = 0.0, mid: Optional[torch.Tensor] = None,
                                     s: Optional[torch.Tensor] = None,
                                     ranks: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """Recompress every factor pair of a batch whose factors are both tall (blocks large on both sides) to a truncated SVD without forming
    the blocks, in one stream-ordered call (rc_lowrank_recompress_large_batched_*): lowrank_recompress_tall_batched's scheme with right^T
    taken through the same flat Householder TSQR in stages of 512 rows as left.

    The arguments and results are lowrank_recompress_tall_batched's with m, n <= 65536 (K <= min(m, n), K <= 128): U [count, m, kk],
    S [count, K], Vt [count, kk, n] and the new ranks; the largest-|.| entry of each kept column of U, over all m rows, is positive and Vt
    takes U's signs.  For n <= 512 the outputs are lowrank_recompress_tall_batched's bit for bit; a block's bits are those of its truncated
    factors passed at inner width q.  No transposition symmetry is promised.  Real dtypes only: complex data raises TypeError (see
    lowrank_recompress_large_batched_complex)."""
    return _lowrank_recompress_batched("lowrank_recompress_large_batched", False, left, right, k, tol, mid, s, ranks, tall="large")


def svd_add_large_batched(u1: torch.Tensor, s1: torch.Tensor, vt1: torch.Tensor, u2: torch.Tensor, s2: torch.Tensor, vt2: torch.Tensor, k: int,
                          tol: float = 0.0, ranks1: Optional[torch.Tensor] = None,
                          ranks2: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """svd_add_batched for blocks large on both sides (m, n <= 65536): the rounded sum of two batches of truncated SVDs through
    lowrank_recompress_large_batched.  ranks1 / ranks2 ([count] int64, optional): the ranks of the two addends; columns of U1, U2, entries of
    s1, s2 and rows of Vt1, Vt2 past them are zeroed before the concatenation (without them the zero tails the batched calls write are relied
    on, as in svd_add_batched)."""
    left, right, s = _svd_add_large_operands(u1, s1, vt1, u2, s2, vt2, ranks1, ranks2)
    return lowrank_recompress_large_batched(left, right, k, tol, s=s)


def _svd_add_large_operands(u1, s1, vt1, u2, s2, vt2, ranks1, ranks2):
    """The concatenated factors of svd_add_large_batched and its complex twin, cut at ranks1 / ranks2 where given."""
    k1, k2 = u1.shape[2], u2.shape[2]

    def cut(u, s, vt, ranks, kx):  # on the device, no host synchronisation; what lies past a rank may be anything, NaN included
        if ranks is None:
            return u, s, vt
        keep = torch.arange(kx, device=s.device)[None, :] < ranks[:, None]
        zero = torch.zeros((), dtype=u.dtype, device=u.device)
        szero = torch.zeros((), dtype=s.dtype, device=s.device)  # s is real where u is complex
        return torch.where(keep[:, None, :], u, zero), torch.where(keep, s[:, :kx], szero), torch.where(keep[:, :, None], vt, zero)

    u1, s1, vt1 = cut(u1, s1, vt1, ranks1, k1)
    u2, s2, vt2 = cut(u2, s2, vt2, ranks2, k2)
    left = torch.cat([u1, u2], dim=2)
    right = torch.cat([vt1, vt2], dim=1)
    s = torch.cat([s1[:, :k1], s2[:, :k2]], dim=1)
    return left, right, s


def lowrank_recompress_tall_batched_complex(left: torch.Tensor, right: torch.Tensor, k: int, tol: float = 0.0, mid: Optional[torch.Tensor] = None,
                                            s: Optional[torch.Tensor] = None,
                                            ranks: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """lowrank_recompress_tall_batched for complex factors (rc_lowrank_recompress_tall_complex_batched_c64 / _c32): the arguments, dtypes and
    results of lowrank_recompress_batched_complex (left, right and mid complex128 or complex64 of one dtype, lazily conjugated views
    materialised, s and S real, Vt the conjugate transpose of V, nothing conjugated in the product; real data and mismatched dtypes raise
    TypeError) with m <= 65536: the left factor goes through the staged Householder TSQR of lowrank_recompress_tall_batched.  In each kept
    column of U the first of its largest-modulus entries over all m rows is real and positive, its imaginary part exactly 0; conjugated
    inputs give the conjugated U and Vt bit for bit.  For m <= 512 the outputs are lowrank_recompress_batched_complex's bit for bit.
    A wide pair (tall right) is the transpose, and because Vt = V^H with nothing conjugated in U S Vt, the recipe is the plain transpose of
    all three factors: pass right.mT, mid.mT, left.mT and read the block's U as Vt_out.mT and its Vt as U_out.mT (no .conj() anywhere);
    the phase rule then holds on the rows of the block's Vt."""
    return _lowrank_recompress_batched("lowrank_recompress_tall_batched_complex", True, left, right, k, tol, mid, s, ranks, tall=True)


def lowrank_recompress_large_batched_complex(left: torch.Tensor, right: torch.Tensor, k: int, tol: float = 0.0, mid: Optional[torch.Tensor] = None,
                                             s: Optional[torch.Tensor] = None,
                                             ranks: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """lowrank_recompress_large_batched for complex factors (rc_lowrank_recompress_complex_large_batched_c64 / _c32): the arguments, dtypes and
    results of lowrank_recompress_tall_batched_complex (left, right and mid complex128 or complex64 of one dtype, lazily conjugated views
    materialised, s and S real, Vt the conjugate transpose of V, nothing conjugated in the product; real data and mismatched dtypes raise
    TypeError) with m, n <= 65536: the plain transpose of right goes through the same staged Householder TSQR as left.  In each kept column
    of U the first of its largest-modulus entries over all m rows is real and positive, its imaginary part exactly 0, and the matching row
    of Vt carries the conjugate phase; conjugated inputs give the conjugated U and Vt bit for bit.  For n <= 512 the outputs are
    lowrank_recompress_tall_batched_complex's bit for bit; a block's bits are those of its truncated factors passed at inner width q."""
    return _lowrank_recompress_batched("lowrank_recompress_large_batched_complex", True, left, right, k, tol, mid, s, ranks, tall="large")


def svd_add_large_batched_complex(u1: torch.Tensor, s1: torch.Tensor, vt1: torch.Tensor, u2: torch.Tensor, s2: torch.Tensor, vt2: torch.Tensor, k: int,
                                  tol: float = 0.0, ranks1: Optional[torch.Tensor] = None,
                                  ranks2: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """svd_add_large_batched for complex truncated SVDs (U, Vt complex, s real; Vt = V^H, nothing conjugated in U diag(s) Vt), through
    lowrank_recompress_large_batched_complex, with the same ranks1 / ranks2 cut."""
    left, right, s = _svd_add_large_operands(u1, s1, vt1, u2, s2, vt2, ranks1, ranks2)
    return lowrank_recompress_large_batched_complex(left, right, k, tol, s=s)


def column_id_to_svd_tall_batched_complex(c: torch.Tensor, z: torch.Tensor, ranks: Optional[torch.Tensor], k: int,
                                          tol: float = 0.0) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """column_id_to_svd_tall_batched for the complex outputs of sketch_column_id_rank_batched_complex."""
    return lowrank_recompress_tall_batched_complex(c, z, k, tol, ranks=ranks)


def svd_add_tall_batched_complex(u1: torch.Tensor, s1: torch.Tensor, vt1: torch.Tensor, u2: torch.Tensor, s2: torch.Tensor, vt2: torch.Tensor, k: int,
                                 tol: float = 0.0) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """svd_add_batched_complex for tall blocks (m <= 65536): the rounded sum of two batches of complex truncated SVDs through
    lowrank_recompress_tall_batched_complex."""
    k1, k2 = u1.shape[2], u2.shape[2]
    left = torch.cat([u1, u2], dim=2)
    right = torch.cat([vt1, vt2], dim=1)
    s = torch.cat([s1[:, :k1], s2[:, :k2]], dim=1)
    return lowrank_recompress_tall_batched_complex(left, right, k, tol, s=s)


def column_id_to_svd_batched_complex(c: torch.Tensor, z: torch.Tensor, ranks: Optional[torch.Tensor], k: int,
                                     tol: float = 0.0) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """column_id_to_svd_batched for the complex outputs of column_id_rank_batched."""
    return lowrank_recompress_batched_complex(c, z, k, tol, ranks=ranks)


def two_sided_id_to_svd_batched_complex(c: torch.Tensor, x: torch.Tensor, r: torch.Tensor, ranks: Optional[torch.Tensor], k: int,
                                        tol: float = 0.0) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """two_sided_id_to_svd_batched for the complex outputs of two_sided_id_rank_batched."""
    return lowrank_recompress_batched_complex(c, r, k, tol, mid=x, ranks=ranks)


def svd_add_batched_complex(u1: torch.Tensor, s1: torch.Tensor, vt1: torch.Tensor, u2: torch.Tensor, s2: torch.Tensor, vt2: torch.Tensor, k: int,
                            tol: float = 0.0) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """svd_add_batched for the outputs of svd_rank_batched_complex or of the complex recompressions: u and vt (= V^H) complex, s real.
    Block i of the result is the SVD of U1 diag(s1) Vt1 + U2 diag(s2) Vt2; zero columns of U1, U2 come out as exactly zero singular values."""
    k1, k2 = u1.shape[2], u2.shape[2]
    left = torch.cat([u1, u2], dim=2)
    right = torch.cat([vt1, vt2], dim=1)
    s = torch.cat([s1[:, :k1], s2[:, :k2]], dim=1)
    return lowrank_recompress_batched_complex(left, right, k, tol, s=s)


def _lowrank_residual_batched(who: str, complex_data: bool, a, left, right, mid, s, ranks, want_residual: bool):
    """The shared body of lowrank_residual_batched (real dtypes) and lowrank_residual_batched_complex (complex dtypes, real s)."""
    from . import _lib
    from .types import as_device

    ops = {"a": a, "left": left, "right": right, "mid": mid}
    ops = {name: as_device(t) for name, t in ops.items() if t is not None}
    if complex_data:
        ops = {name: t.resolve_conj() for name, t in ops.items()}  # the kernels read the stored values
    a, left, right, mid = ops["a"], ops["left"], ops["right"], ops.get("mid")
    kinds = (torch.complex128, torch.complex64) if complex_data else (torch.float64, torch.float32)
    if a.dtype not in kinds:
        raise TypeError(f"{who}: {' or '.join(str(k).replace('torch.', '') for k in kinds)} data expected, got {a.dtype}")
    for name, t in ops.items():
        if t.dtype != a.dtype:
            raise TypeError(f"{who}: {name} is {t.dtype}, a is {a.dtype}")
    real = _lib.real_dtype(a.dtype)
    if s is not None:
        s = as_device(s)
        if s.dtype != real:
            raise TypeError(f"{who}: s is {s.dtype}, expected {real}")
        ops["s"] = s
    if a.dim() != 3 or left.dim() != 3 or right.dim() != 3 or (mid is not None and mid.dim() != 3):
        raise AssertionError("expected a [count, m, n], left [count, m, K], right [count, K, n] and mid [count, K, K]")
    count, m, n = a.shape
    kin = left.shape[2]
    for name, t in ops.items():
        if t.shape[0] != count:
            raise AssertionError(f"{who}: {name} holds {t.shape[0]} blocks, a {count}")
    if s is not None:
        if s.dim() != 2 or s.shape[1] < kin:
            raise AssertionError(f"{who}: s must be [count, p] with p >= K = {kin}")
        if s.stride(1) != 1:
            s = s.contiguous()
    if ranks is not None:
        ranks = as_device(ranks)
        if ranks.dtype != torch.int64:
            raise TypeError(f"{who}: ranks is {ranks.dtype}, expected torch.int64")
        if ranks.shape != (count,):
            raise AssertionError(f"{who}: ranks must be [count]")
        ranks = ranks.contiguous()
    err = torch.empty(count, dtype=real, device=a.device)
    nrm = torch.empty(count, dtype=real, device=a.device)
    e = torch.empty((count, m, n), dtype=a.dtype, device=a.device) if want_residual else None

    def view(t):  # block 0's view and the batch stride
        if t is None:
            return _lib.mat(None), ctypes.c_int64(0)
        return _lib.rc_matrix(t.data_ptr(), t.shape[1], t.shape[2], t.stride(1), t.stride(2)), ctypes.c_int64(t.stride(0))

    _lib.default_context().call(f"rc_lowrank_residual_batched_{_lib.suffix(a.dtype)}", *view(a), *view(left), *view(mid),
                                ctypes.c_void_p(s.data_ptr() if s is not None else None), ctypes.c_int64(s.stride(0) if s is not None else 0),
                                *view(right), _lib.i64p(ranks), ctypes.c_int32(count), *view(e), ctypes.c_void_p(err.data_ptr()),
                                ctypes.c_void_p(nrm.data_ptr()))
    return (err, nrm, e) if want_residual else (err, nrm)


def lowrank_residual_batched(a: torch.Tensor, left: torch.Tensor, right: torch.Tensor, mid: Optional[torch.Tensor] = None, s: Optional[torch.Tensor] = None,
                             ranks: Optional[torch.Tensor] = None, want_residual: bool = False):
    """Residual norms of every block of a batch against its low-rank factors in one stream-ordered call (rc_lowrank_residual_batched_*):
    the reference's rel_diff_fro(x.to_mat(), a) per block (src/lib.rs) without the rebuilt blocks, for the outputs of every batched compressor.

    a: [count, m, n], left: [count, m, K], right: [count, K, n], mid: [count, K, K] or None, s: [count, p >= K] or None, ranks: [count] int64
    or None (every rank is K); float64 or float32 device tensors of one dtype, any strides (a stride-0 batch dimension shares one operand);
    m <= 65536, n <= 512, K <= 128.  With r = ranks[i] clamped to [0, K] and Ah_i = left[i][:, :r] mid[i][:r, :r] diag(s[i][:r]) right[i][:r]
    (absent factors omitted; nothing at an index >= r is read), returns err [count] = ||a_i - Ah_i||_F and nrm [count] = ||a_i||_F, and with
    want_residual also e [count, m, n] = a_i - Ah_i.  Complex data (see lowrank_residual_batched_complex) and mismatched dtypes raise TypeError.

    Input scale: err and nrm neither overflow nor vanish for blocks with entries anywhere in the range of the batched compressors (2^+-900
    in float64 / complex128: the squares are binned as LAPACK's ?lassq bins them; float32 / complex64 squares are taken in float64).  The
    rebuild's intermediate products diag(s) right and mid (diag(s) right) are formed as the operands stand: a factor set whose
    intermediates leave the range although its product does not stays the caller's to rescale."""
    return _lowrank_residual_batched("lowrank_residual_batched", False, a, left, right, mid, s, ranks, want_residual)


def lowrank_residual_batched_complex(a: torch.Tensor, left: torch.Tensor, right: torch.Tensor, mid: Optional[torch.Tensor] = None,
                                     s: Optional[torch.Tensor] = None, ranks: Optional[torch.Tensor] = None, want_residual: bool = False):
    """lowrank_residual_batched for complex blocks and factors (rc_lowrank_residual_batched_c64 / _c32): a, left, right and mid complex128 or
    complex64 device tensors of one dtype (lazily conjugated views are materialised), s of the matching real dtype (float64 / float32);
    real data, mismatched dtypes and a complex s raise TypeError.  Nothing is conjugated: Ah_i = left[i][:, :r] mid[i][:r, :r]
    diag(s[i][:r]) right[i][:r], so vt is the V^H svd_rank_batched_complex returns.  err and nrm come back in the real dtype, e complex."""
    return _lowrank_residual_batched("lowrank_residual_batched_complex", True, a, left, right, mid, s, ranks, want_residual)


def column_id_residual_batched(a: torch.Tensor, c: torch.Tensor, z: torch.Tensor, ranks: Optional[torch.Tensor], want_residual: bool = False):
    """||a_i - C[:, :r] Z[:r]||_F and ||a_i||_F per block for the outputs of column_id_rank_batched / sketch_column_id_rank_batched."""
    return lowrank_residual_batched(a, c, z, ranks=ranks, want_residual=want_residual)


def two_sided_id_residual_batched(a: torch.Tensor, c: torch.Tensor, x: torch.Tensor, r: torch.Tensor, ranks: Optional[torch.Tensor],
                                  want_residual: bool = False):
    """||a_i - C X R||_F at the block's rank and ||a_i||_F per block for the outputs of two_sided_id_rank_batched."""
    return lowrank_residual_batched(a, c, r, mid=x, ranks=ranks, want_residual=want_residual)


def svd_residual_batched(a: torch.Tensor, u: torch.Tensor, s: torch.Tensor, vt: torch.Tensor, ranks: Optional[torch.Tensor], want_residual: bool = False):
    """||a_i - U diag(s) Vt||_F at the block's rank and ||a_i||_F per block for the outputs of svd_rank_batched and of the recompressions; s is
    the [count, p] tensor those calls return, read with row stride p."""
    return lowrank_residual_batched(a, u, vt, s=s, ranks=ranks, want_residual=want_residual)


def column_id_residual_batched_complex(a: torch.Tensor, c: torch.Tensor, z: torch.Tensor, ranks: Optional[torch.Tensor], want_residual: bool = False):
    """column_id_residual_batched for the complex outputs of column_id_rank_batched."""
    return lowrank_residual_batched_complex(a, c, z, ranks=ranks, want_residual=want_residual)


def two_sided_id_residual_batched_complex(a: torch.Tensor, c: torch.Tensor, x: torch.Tensor, r: torch.Tensor, ranks: Optional[torch.Tensor],
                                          want_residual: bool = False):
    """two_sided_id_residual_batched for the complex outputs of two_sided_id_rank_batched."""
    return lowrank_residual_batched_complex(a, c, r, mid=x, ranks=ranks, want_residual=want_residual)


def svd_residual_batched_complex(a: torch.Tensor, u: torch.Tensor, s: torch.Tensor, vt: torch.Tensor, ranks: Optional[torch.Tensor],
                                 want_residual: bool = False):
    """svd_residual_batched for the outputs of svd_rank_batched_complex: u and vt (= V^H) complex, s the real [count, p] tensor it returns."""
    return lowrank_residual_batched_complex(a, u, vt, s=s, ranks=ranks, want_residual=want_residual)


def _default_omega(a, k, oversampling, seed, who):
    """The shared Gaussian omega every sketched call draws when none is given: l = min(k + oversampling, 128) rows (at least one) of
    rc_random_gaussian_* at (seed, offset 0), in a's dtype."""
    from .random_matrix import Rng, random_gaussian

    if k is None:
        raise AssertionError(f"{who}: k is needed to draw the default omega")
    return random_gaussian((max(min(int(k) + int(oversampling), 128), 1), a.shape[-2]), Rng(int(seed)), a.dtype)


def _sketch_column_id_rank_batched(who: str, complex_data: bool, a, k, tol, omega, oversampling, seed, return_sketch: bool):
    """The body of sketch_column_id_rank_batched and sketch_column_id_rank_batched_complex: the checks, the default omega and the call."""
    from . import _lib
    from .types import as_device

    a = as_device(a)
    kinds = (torch.complex128, torch.complex64) if complex_data else (torch.float64, torch.float32)
    if a.dtype not in kinds:
        raise TypeError(f"{who}: {'complex128 or complex64' if complex_data else 'float64 or float32'} data expected, got {a.dtype}")
    if a.dim() != 3:
        raise AssertionError("expected a [count, m, n] batch")
    a = a.resolve_conj()  # a lazily conjugated complex view is materialised: the kernels read the stored values
    count, m, n = a.shape
    if omega is None:
        omega = _default_omega(a, k, oversampling, seed, who)
    omega = as_device(omega)
    if omega.dtype != a.dtype:
        raise TypeError(f"{who}: omega is {omega.dtype}, a is {a.dtype}")
    omega = omega.resolve_conj()
    if omega.dim() not in (2, 3) or (omega.dim() == 3 and omega.shape[0] != count):
        raise AssertionError("expected omega [l, m] or [count, l, m]")
    l = omega.shape[-2]
    obs = omega.stride(0) if omega.dim() == 3 else 0
    kk = max(min(int(k), l, n), 0)
    c = torch.empty((count, m, kk), dtype=a.dtype, device=a.device)
    z = torch.empty((count, kk, n), dtype=a.dtype, device=a.device)
    ind = torch.empty((count, n), dtype=torch.int64, device=a.device)
    ranks = torch.empty(count, dtype=torch.int64, device=a.device)
    y = torch.empty((count, l, n), dtype=a.dtype, device=a.device) if return_sketch else None
    stem = "rc_sketch_column_id_rank_complex_batched_" if complex_data else "rc_sketch_column_id_rank_batched_"
    _lib.default_context().call(stem + _lib.suffix(a.dtype),
                                _lib.rc_matrix(a.data_ptr(), m, n, a.stride(1), a.stride(2)), ctypes.c_int64(a.stride(0)),
                                _lib.rc_matrix(omega.data_ptr(), l, omega.shape[-1], omega.stride(-2), omega.stride(-1)), ctypes.c_int64(obs),
                                ctypes.c_int32(count), ctypes.c_int64(int(k)), ctypes.c_double(float(tol)),
                                _lib.rc_matrix(y.data_ptr(), l, n, n, 1) if return_sketch else _lib.mat(None), ctypes.c_int64(l * n),
                                _lib.rc_matrix(c.data_ptr(), m, kk, kk, 1), ctypes.c_int64(m * kk),
                                _lib.rc_matrix(z.data_ptr(), kk, n, n, 1), ctypes.c_int64(kk * n), _lib.i64p(ind), _lib.i64p(ranks))
    return (c, z, ind, ranks, y) if return_sketch else (c, z, ind, ranks)


def sketch_column_id_rank_batched(a: torch.Tensor, k: int, tol: float = 0.0, omega: Optional[torch.Tensor] = None, oversampling: int = 8, seed: int = 0,
                                  return_sketch: bool = False):
    """One-pass randomized column IDs of `count` tall same-shaped blocks in one stream-ordered call (rc_sketch_column_id_rank_batched_*):
    per block the sketch Y = omega a (l x n) and the column ID of Y, C gathered from a; the reference's sample_range_by_rank projection
    (src/random_sampling.rs) followed by QR::compute_from_range_estimate + column_id (src/qr.rs:311-323).

    a: [count, m, n] device tensor of float64 or float32, any strides (m <= 65536, n <= 512).  omega: [l, m] (shared by the batch) or
    [count, l, m], l <= 128, a's dtype, any strides; None draws one shared Gaussian omega of l = min(k + oversampling, 128) rows with
    rc_random_gaussian_* at (seed, offset 0), so the result is that of the explicit call with random_gaussian((l, m), Rng(seed)).
    k (<= 128) is clamped to kk = min(k, l, n).  Returns C [count, m, kk], Z [count, kk, n], ind [count, n], ranks [count] and, with
    return_sketch, Y [count, l, n]: Z, ind and ranks are column_id_rank_batched(Y, k, tol)'s bit for bit, C[:, :, j] = a[:, :, ind[j]]
    for j below the block's rank, the rest of C and Z zero.  Complex data (see sketch_column_id_rank_batched_complex) and mismatched
    dtypes raise TypeError."""
    return _sketch_column_id_rank_batched("sketch_column_id_rank_batched", False, a, k, tol, omega, oversampling, seed, return_sketch)


def sketch_svd_rank_batched(a: torch.Tensor, k: int, tol: float = 0.0, omega: Optional[torch.Tensor] = None, oversampling: int = 8,
                            seed: int = 0) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """Batched randomized SVDs of `count` tall same-shaped blocks (m <= 65536, n <= 512): the reference's sketch -> factor the small matrix ->
    SVD path in two launches with no host synchronisation between them, sketch_column_id_rank_batched(a, k, tol, omega, oversampling, seed)
    followed by column_id_to_svd_tall_batched on its (C, Z, ranks).  Returns (U [count, m, kk], S [count, kk], Vt [count, kk, n], ranks),
    kk = min(k, l, n): the truncated SVD of each block's one-pass column ID C Z, bit for bit that of the two calls made by hand.
    Complex data raises TypeError (see sketch_svd_rank_batched_complex)."""
    c, z, _, ranks = sketch_column_id_rank_batched(a, k, tol, omega, oversampling, seed)
    return column_id_to_svd_tall_batched(c, z, ranks, k, tol)


def sketch_column_id_rank_batched_complex(a: torch.Tensor, k: int, tol: float = 0.0, omega: Optional[torch.Tensor] = None, oversampling: int = 8,
                                          seed: int = 0, return_sketch: bool = False):
    """sketch_column_id_rank_batched for complex tall blocks (rc_sketch_column_id_rank_complex_batched_c64 / _c32): a and omega complex128 or
    complex64 device tensors of one dtype (lazily conjugated views are materialised); real data and mismatched dtypes raise TypeError.
    Y = omega a with nothing conjugated: a caller who wants Q^H a passes Q^H.  omega=None draws one shared complex Gaussian of
    l = min(k + oversampling, 128) rows with rc_random_gaussian_c64 / _c32 at (seed, offset 0): random_gaussian((l, m), Rng(seed), a.dtype).
    Z, ind and ranks are column_id_rank_batched(Y, k, tol)'s on the complex sketch bit for bit."""
    return _sketch_column_id_rank_batched("sketch_column_id_rank_batched_complex", True, a, k, tol, omega, oversampling, seed, return_sketch)


def sketch_svd_rank_batched_complex(a: torch.Tensor, k: int, tol: float = 0.0, omega: Optional[torch.Tensor] = None, oversampling: int = 8,
                                    seed: int = 0) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """sketch_svd_rank_batched for complex tall blocks: sketch_column_id_rank_batched_complex(a, k, tol, omega, oversampling, seed) followed by
    column_id_to_svd_tall_batched_complex on its (C, Z, ranks), two launches with no host synchronisation between them.  Returns
    (U, S real, Vt = V^H, ranks), bit for bit the result of the two calls made by hand."""
    c, z, _, ranks = sketch_column_id_rank_batched_complex(a, k, tol, omega, oversampling, seed)
    return column_id_to_svd_tall_batched_complex(c, z, ranks, k, tol)


def _require_dtype(who: str, complex_data: bool, a) -> None:
    """TypeError for anything but complex128 / complex64 (complex_data) or float64 / float32 data, raised before a device is asked for."""
    dtype = a.dtype if isinstance(a, torch.Tensor) else torch.from_numpy(np.asarray(a)).dtype
    if dtype not in ((torch.complex128, torch.complex64) if complex_data else (torch.float64, torch.float32)):
        raise TypeError(f"{who}: {'complex128 or complex64' if complex_data else 'float64 or float32'} data expected, got {dtype}")


def _sketch_range_step_batched(who: str, complex_data: bool, a, omega, oversampling, k, seed, return_sketch: bool, conj_p: bool):
    """The body of sketch_range_step_batched and sketch_range_step_batched_complex: the checks, the default omega and the call; only the
    complex entry points take conj_p."""
    from . import _lib
    from .types import as_device

    _require_dtype(who, complex_data, a)
    a = as_device(a)
    if a.dim() != 3:
        raise AssertionError("expected a [count, m, n] batch")
    a = a.resolve_conj()  # a lazily conjugated complex view is materialised: the kernels read the stored values
    count, m, n = a.shape
    if omega is None:
        omega = _default_omega(a, k, oversampling, seed, who)
    omega = as_device(omega)
    if omega.dtype != a.dtype:
        raise TypeError(f"{who}: omega is {omega.dtype}, a is {a.dtype}")
    omega = omega.resolve_conj()
    if omega.dim() not in (2, 3) or (omega.dim() == 3 and omega.shape[0] != count):
        raise AssertionError("expected omega [l, m] or [count, l, m]")
    l = omega.shape[-2]
    obs = omega.stride(0) if omega.dim() == 3 else 0
    q = torch.empty((count, l, n), dtype=a.dtype, device=a.device)
    p = torch.empty((count, m, l), dtype=a.dtype, device=a.device)
    ranks = torch.empty(count, dtype=torch.int64, device=a.device)
    y = torch.empty((count, l, n), dtype=a.dtype, device=a.device) if return_sketch else None
    stem = "rc_sketch_range_step_complex_batched_" if complex_data else "rc_sketch_range_step_batched_"
    _lib.default_context().call(stem + _lib.suffix(a.dtype),
                                _lib.rc_matrix(a.data_ptr(), m, n, a.stride(1), a.stride(2)), ctypes.c_int64(a.stride(0)),
                                _lib.rc_matrix(omega.data_ptr(), l, omega.shape[-1], omega.stride(-2), omega.stride(-1)), ctypes.c_int64(obs),
                                ctypes.c_int32(count),
                                _lib.rc_matrix(y.data_ptr(), l, n, n, 1) if return_sketch else _lib.mat(None), ctypes.c_int64(l * n),
                                _lib.rc_matrix(q.data_ptr(), l, n, n, 1), ctypes.c_int64(l * n),
                                _lib.rc_matrix(p.data_ptr(), m, l, l, 1), ctypes.c_int64(m * l), _lib.i64p(ranks),
                                *([ctypes.c_int32(1 if conj_p else 0)] if complex_data else []))
    return (q, p, ranks, y) if return_sketch else (q, p, ranks)


def _power_iteration_batched(complex_data: bool, a, omega, k, oversampling, seed) -> torch.Tensor:
    """One full power iteration: the range step, then P orthonormalised by the tall recompression with right = I at the step's ranks (zero
    singular values give exactly zero columns); U^T, a strided view, is the next omega.  On complex blocks the step runs with conj_p: the
    recompression of conj(P) gives conj of P's basis, so U^T is that basis' conjugate transpose and nothing is conjugated by a kernel of
    its own.  Two launches, nothing on the host between them."""
    sfx = "_complex" if complex_data else ""
    _, p, ranks = _sketch_range_step_batched("sketch_range_step_batched" + sfx, complex_data, a, omega, oversampling, k, seed, False, complex_data)
    l = p.shape[2]
    eye = torch.eye(l, dtype=p.dtype, device=p.device).expand(p.shape[0], l, l)
    u, _, _, _ = _lowrank_recompress_batched("lowrank_recompress_tall_batched" + sfx, complex_data, p, eye, l, 0.0, None, None, ranks, tall=True)
    return u.mT


def _sketch_power_omega_batched(who: str, complex_data: bool, a, k, power_iterations, omega, oversampling, seed) -> torch.Tensor:
    """The body of sketch_power_omega_batched and sketch_power_omega_batched_complex."""
    from .types import as_device

    _require_dtype(who, complex_data, a)
    a = as_device(a)
    if int(power_iterations) < 0:
        raise AssertionError(f"{who}: power_iterations must be >= 0")
    if omega is None:
        omega = _default_omega(a, k, oversampling, seed, who)
    for _ in range(int(power_iterations)):
        omega = _power_iteration_batched(complex_data, a, omega, k, oversampling, seed)
    return omega


def _sketch_column_id_rank_power_batched(who: str, complex_data: bool, a, k, tol, power_iterations, omega, oversampling, seed, return_sketch: bool):
    """The body of sketch_column_id_rank_power_batched and its _complex twin: the power rounds on omega, then the one-pass call.  The complex
    name refuses real data itself; the real one leaves complex data to the calls below, which refuse it under their own names."""
    sfx = "_complex" if complex_data else ""
    if complex_data:
        _require_dtype(who, True, a)
    if int(power_iterations) != 0:
        omega = _sketch_power_omega_batched("sketch_power_omega_batched" + sfx, complex_data, a, k, power_iterations, omega, oversampling, seed)
    return _sketch_column_id_rank_batched("sketch_column_id_rank_batched" + sfx, complex_data, a, k, tol, omega, oversampling, seed, return_sketch)


def _sketch_svd_rank_power_batched(who: str, complex_data: bool, a, k, tol, power_iterations, omega, oversampling, seed):
    """The body of sketch_svd_rank_power_batched and its _complex twin: all but the last power round on omega, one more range step (P not
    conjugated), then the tall recompression of (P, Q).  Who refuses data of the other kind: as in _sketch_column_id_rank_power_batched."""
    sfx = "_complex" if complex_data else ""
    if complex_data:
        _require_dtype(who, True, a)
    if int(power_iterations) == 0:
        return (sketch_svd_rank_batched_complex if complex_data else sketch_svd_rank_batched)(a, k, tol, omega, oversampling, seed)
    omega_q = _sketch_power_omega_batched("sketch_power_omega_batched" + sfx, complex_data, a, k, int(power_iterations) - 1, omega, oversampling, seed)
    q, p, ranks = _sketch_range_step_batched("sketch_range_step_batched" + sfx, complex_data, a, omega_q, oversampling, k, seed, False, False)
    return _lowrank_recompress_batched("lowrank_recompress_tall_batched" + sfx, complex_data, p, q, k, tol, None, None, ranks, tall=True)


def sketch_range_step_batched(a: torch.Tensor, omega: Optional[torch.Tensor] = None, oversampling: int = 8, k: Optional[int] = None, seed: int = 0,
                              return_sketch: bool = False):
    """One range step of a power iteration on `count` tall same-shaped blocks in one stream-ordered call (rc_sketch_range_step_batched_*):
    per block the sketch Y = omega a (l x n, sketch_column_id_rank_batched's bit for bit), an orthonormal basis Q (l x n) of Y's rows from a
    column-pivoted Householder QR of Y^T, and the projection P = a Q^T (m x l); the two products of one round of the reference's
    sample_range_power_iteration (src/random_sampling.rs:131-158) with the orthonormalisation between them.

    a: [count, m, n] device tensor of float64 or float32, any strides (m <= 65536, n <= 512).  omega: [l, m] (shared by the batch) or
    [count, l, m], l <= min(128, m, n), a's dtype, any strides; None draws the shared Gaussian omega of sketch_column_id_rank_batched(a, k,
    oversampling=oversampling, seed=seed), l = min(k + oversampling, 128) rows.  Returns Q [count, l, n], P [count, m, l], ranks [count] and,
    with return_sketch, Y [count, l, n]: rows of Q below a block's rank r are orthonormal, rows of Q and columns of P from r on are exactly
    zero; r is the first step whose R_jj is exactly zero or not finite, else l (no tolerance: truncation belongs to the call that ends the
    chain).  Complex data and mismatched dtypes raise TypeError."""
    return _sketch_range_step_batched("sketch_range_step_batched", False, a, omega, oversampling, k, seed, return_sketch, False)


def sketch_power_omega_batched(a: torch.Tensor, k: int, power_iterations: int, omega: Optional[torch.Tensor] = None, oversampling: int = 8,
                               seed: int = 0) -> torch.Tensor:
    """The test matrix after `power_iterations` rounds of the reference's sample_range_power_iteration (src/random_sampling.rs:131-158) on every
    block of a batch, both half-steps orthonormalised: per round sketch_range_step_batched, then lowrank_recompress_tall_batched(p, I, k=l,
    tol=0, ranks=the step's ranks), whose U^T (a strided view, no copy) is the next omega.  Two launches per round and no host
    synchronisation.  a, omega, k, oversampling and seed as sketch_range_step_batched.  Returns omega_q [count, l, m], whose rows are
    orthonormal (exactly zero past a block's rank); with power_iterations = 0 the omega given or drawn is returned unchanged ([l, m] when
    shared).  Complex data raises TypeError."""
    return _sketch_power_omega_batched("sketch_power_omega_batched", False, a, k, power_iterations, omega, oversampling, seed)


def sketch_column_id_rank_power_batched(a: torch.Tensor, k: int, tol: float = 0.0, power_iterations: int = 1, omega: Optional[torch.Tensor] = None,
                                        oversampling: int = 8, seed: int = 0, return_sketch: bool = False):
    """sketch_column_id_rank_batched after `power_iterations` rounds of power iteration on the test matrix: sketch_power_omega_batched(a, k,
    power_iterations, omega, oversampling, seed), then sketch_column_id_rank_batched(a, k, tol, that omega).  On slowly decaying spectra
    one round roughly halves the error of the one-pass call; more add little.  The return tuple is sketch_column_id_rank_batched's;
    power_iterations = 0 is that function on the same arguments, bit for bit.  2 q + 1 launches, no host synchronisation.  The power
    rounds need l <= min(128, m, n).  Complex data raises TypeError."""
    return _sketch_column_id_rank_power_batched("sketch_column_id_rank_power_batched", False, a, k, tol, power_iterations, omega, oversampling, seed,
                                                return_sketch)


def sketch_svd_rank_power_batched(a: torch.Tensor, k: int, tol: float = 0.0, power_iterations: int = 1, omega: Optional[torch.Tensor] = None,
                                  oversampling: int = 8, seed: int = 0) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """Batched randomized SVDs of tall blocks with power iteration: power_iterations - 1 full rounds (sketch_power_omega_batched), one more
    range step (Q, P = a Q^T, ranks), then lowrank_recompress_tall_batched(left=P, right=Q, ranks=the step's ranks, k, tol): the
    reference's svd_from_range_estimate on a ~ (a Q^T) Q.  Returns (U [count, m, kk], S [count, l], Vt [count, kk, n], ranks), kk = min(k, l).
    power_iterations = 0 delegates to sketch_svd_rank_batched on the same arguments.  2 q launches, no host synchronisation.  Complex data
    raises TypeError."""
    return _sketch_svd_rank_power_batched("sketch_svd_rank_power_batched", False, a, k, tol, power_iterations, omega, oversampling, seed)


def sketch_product_batched(a: torch.Tensor, omega: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The sketch Y = omega a of every block of a batch and nothing else, in one stream-ordered call (rc_sketch_product_batched_*): the
    product sketch_column_id_rank_batched and sketch_range_step_batched form inside their launch, for blocks of any width.

    a: [count, m, n] device tensor of float64 or float32, any strides (m, n <= 65536; a stride-0 batch dimension shares one block).
    omega: [l, m] (shared by the batch) or [count, l, m], l <= 128, a's dtype, any strides.  out: None, or a [count, l, n] device tensor
    of a's dtype that receives Y (any strides, for instance the transposed view of a [count, n, l] tensor; it must not overlap a or
    omega).  Returns Y [count, l, n] (out when given).  An element of Y is one MFMA accumulator chain from zero over ascending rows of
    a: for n <= 512 Y is sketch_column_id_rank_batched(..., return_sketch=True)'s bit for bit, and for any n a column of Y depends on
    that column of a, on omega and on m alone.  P = a Q^T is the call on transposed views: sketch_product_batched(a.mT, q, out=p.mT).
    Complex data and mismatched dtypes raise TypeError."""
    from . import _lib
    from .types import as_device

    who = "sketch_product_batched"
    _require_dtype(who, False, a)
    a, omega = as_device(a), as_device(omega)
    if omega.dtype != a.dtype:
        raise TypeError(f"{who}: omega is {omega.dtype}, a is {a.dtype}")
    if a.dim() != 3:
        raise AssertionError("expected a [count, m, n] batch")
    if omega.dim() not in (2, 3) or (omega.dim() == 3 and omega.shape[0] != a.shape[0]):
        raise AssertionError("expected omega [l, m] or [count, l, m]")
    count, m, n = a.shape
    l = omega.shape[-2]
    obs = omega.stride(0) if omega.dim() == 3 else 0
    if out is None:
        out = torch.empty((count, l, n), dtype=a.dtype, device=a.device)
    else:
        if not isinstance(out, torch.Tensor) or not out.is_cuda or out.dtype != a.dtype:
            raise TypeError(f"{who}: out must be a device tensor of a's dtype {a.dtype}")
        if tuple(out.shape) != (count, l, n):
            raise AssertionError(f"{who}: out must be [{count}, {l}, {n}], got {list(out.shape)}")
    _lib.default_context().call("rc_sketch_product_batched_" + _lib.suffix(a.dtype),
                                _lib.rc_matrix(a.data_ptr(), m, n, a.stride(1), a.stride(2)), ctypes.c_int64(a.stride(0)),
                                _lib.rc_matrix(omega.data_ptr(), l, omega.shape[-1], omega.stride(-2), omega.stride(-1)), ctypes.c_int64(obs),
                                ctypes.c_int32(count), _lib.rc_matrix(out.data_ptr(), l, n, out.stride(1), out.stride(2)),
                                ctypes.c_int64(out.stride(0)))
    return out


_SMALL_N = 512  # the widest block the one-launch range step and sketched ID take


def sketch_range_step_large_batched(a: torch.Tensor, omega: Optional[torch.Tensor] = None, oversampling: int = 8, k: Optional[int] = None,
                                    seed: int = 0) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """sketch_range_step_batched for blocks of any width (m, n <= 65536, l <= min(128, m, n)): Q [count, l, n] with orthonormal rows
    spanning the rows of Y = omega a, P = a Q^T [count, m, l] and the ranks [count]; rows of Q and columns of P from a block's rank on
    are exactly zero.  a, omega, oversampling, k and seed as sketch_range_step_batched.

    n <= 512 returns sketch_range_step_batched's outputs by calling it.  Above that, three launches with nothing on the host between them:
    Y = sketch_product_batched(a, omega); the row basis by lowrank_recompress_tall_batched(Y^T, I, k=l, tol=0), whose U^T (a strided
    view) is Q and whose ranks are the step's (a singular value that is exactly zero ends the rank, where the one-launch step tests the
    diagonal of R); and P by sketch_product_batched(a^T, Q) into P^T.  Complex data raises TypeError."""
    who = "sketch_range_step_large_batched"
    _require_dtype(who, False, a)
    if a.dim() != 3:
        raise AssertionError("expected a [count, m, n] batch")
    if a.shape[2] <= _SMALL_N:
        return sketch_range_step_batched(a, omega, oversampling, k, seed)
    from .types import as_device

    a = as_device(a)
    if omega is None:
        omega = _default_omega(a, k, oversampling, seed, who)
    omega = as_device(omega)
    count, m, n = a.shape
    l = omega.shape[-2]
    if l > min(128, m, n):
        raise AssertionError(f"{who}: needs 1 <= l <= min(128, m, n) (got a {m} x {n}, omega {l} x {omega.shape[-1]})")
    y = sketch_product_batched(a, omega)
    eye = torch.eye(l, dtype=a.dtype, device=a.device).expand(count, l, l)
    u, _, _, ranks = lowrank_recompress_tall_batched(y.mT, eye, l, 0.0)
    q = u.mT
    p = torch.empty((count, m, l), dtype=a.dtype, device=a.device)
    sketch_product_batched(a.mT, q, out=p.mT)
    return q, p, ranks


def sketch_svd_rank_large_batched(a: torch.Tensor, k: int, tol: float = 0.0, power_iterations: int = 1, omega: Optional[torch.Tensor] = None,
                                  oversampling: int = 8, seed: int = 0) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """Batched randomized SVDs of blocks of any width (m, n <= 65536): sketch_svd_rank_power_batched's chain with
    sketch_range_step_large_batched as the step and lowrank_recompress_large_batched at the end.  power_iterations counts range steps as
    sketch_svd_rank_power_batched counts them and must be >= 1: between steps P is orthonormalised by lowrank_recompress_tall_batched(p, I,
    k=l, tol=0, ranks=the step's ranks), whose U^T is the next omega; after the last step lowrank_recompress_large_batched(p, q, k, tol,
    ranks=ranks) gives (U [count, m, kk], S [count, l], Vt [count, kk, n], ranks), kk = min(k, l).  n <= 512 returns
    sketch_svd_rank_power_batched's result by calling it.  3 q + (q - 1) + 1 launches above that, no host synchronisation.  Complex data
    raises TypeError."""
    who = "sketch_svd_rank_large_batched"
    _require_dtype(who, False, a)
    if int(power_iterations) < 1:
        raise AssertionError(f"{who}: power_iterations must be >= 1: without a range step the SVD goes through the one-pass column ID, which needs "
                             f"n <= {_SMALL_N} (sketch_svd_rank_batched)")
    if a.dim() != 3:
        raise AssertionError("expected a [count, m, n] batch")
    if a.shape[2] <= _SMALL_N:
        return sketch_svd_rank_power_batched(a, k, tol, power_iterations, omega, oversampling, seed)
    from .types import as_device

    a = as_device(a)
    if omega is None:
        omega = _default_omega(a, k, oversampling, seed, who)
    for step in range(int(power_iterations)):
        q, p, ranks = sketch_range_step_large_batched(a, omega)
        if step + 1 < int(power_iterations):
            l = p.shape[2]
            eye = torch.eye(l, dtype=p.dtype, device=p.device).expand(p.shape[0], l, l)
            omega = lowrank_recompress_tall_batched(p, eye, l, 0.0, ranks=ranks)[0].mT
    return lowrank_recompress_large_batched(p, q, k, tol, ranks=ranks)


def sketch_range_step_batched_complex(a: torch.Tensor, omega: Optional[torch.Tensor] = None, oversampling: int = 8, k: Optional[int] = None,
                                      seed: int = 0, return_sketch: bool = False, conj_p: bool = False):
    """sketch_range_step_batched for complex tall blocks (rc_sketch_range_step_complex_batched_c64 / _c32): a and omega complex128 or complex64
    device tensors of one dtype (lazily conjugated views are materialised); real data and mismatched dtypes raise TypeError.  Per block
    Y = omega a (l x n, nothing conjugated, sketch_column_id_rank_batched_complex's bit for bit), Q (l x n) with Q Q^H = I on its first r
    rows, which span Y's rows, from the column-pivoted complex Householder QR of the plain transpose Y^T, and P = a Q^H (m x l), so
    a ~ P Q with nothing conjugated.  conj_p=True returns conj(P) instead, the same bits with the sign of every imaginary part flipped at
    the store: the tall complex recompression of conj(P) gives conj(U), whose plain transpose U^H is the next test matrix of a power
    iteration, so no conjugation kernel runs anywhere.  omega=None draws the shared complex Gaussian of
    sketch_column_id_rank_batched_complex(a, k, oversampling=oversampling, seed=seed).  Returns Q [count, l, n], P [count, m, l],
    ranks [count] and, with return_sketch, Y [count, l, n]; rows of Q and columns of P from a block's rank r on are exactly zero; r is the
    first step whose real R_jj is exactly zero or not finite, else l."""
    return _sketch_range_step_batched("sketch_range_step_batched_complex", True, a, omega, oversampling, k, seed, return_sketch, conj_p)


def sketch_power_omega_batched_complex(a: torch.Tensor, k: int, power_iterations: int, omega: Optional[torch.Tensor] = None, oversampling: int = 8,
                                       seed: int = 0) -> torch.Tensor:
    """sketch_power_omega_batched for complex tall blocks: the test matrix after `power_iterations` rounds of the reference's
    sample_range_power_iteration (src/random_sampling.rs:128-168, c64 / c32).  Per round sketch_range_step_batched_complex(conj_p=True), then
    lowrank_recompress_tall_batched_complex(p, I, k=l, tol=0, ranks=the step's ranks), whose u.mT (a strided view, no copy, no conjugation) is
    U^H of the basis of a Q^H's columns and the next omega.  Two launches per round and no host synchronisation.  Returns omega_q
    [count, l, m] with orthonormal rows (exactly zero past a block's rank); with power_iterations = 0 the omega given or drawn is returned
    unchanged ([l, m] when shared).  Real data raises TypeError."""
    return _sketch_power_omega_batched("sketch_power_omega_batched_complex", True, a, k, power_iterations, omega, oversampling, seed)


def sketch_column_id_rank_power_batched_complex(a: torch.Tensor, k: int, tol: float = 0.0, power_iterations: int = 1,
                                                omega: Optional[torch.Tensor] = None, oversampling: int = 8, seed: int = 0,
                                                return_sketch: bool = False):
    """sketch_column_id_rank_power_batched for complex tall blocks: sketch_power_omega_batched_complex(a, k, power_iterations, omega,
    oversampling, seed), then sketch_column_id_rank_batched_complex(a, k, tol, that omega).  The return tuple is
    sketch_column_id_rank_batched_complex's; power_iterations = 0 is that function on the same arguments, bit for bit.  2 q + 1 launches,
    no host synchronisation.  The power rounds need l <= min(128, m, n).  Real data raises TypeError."""
    return _sketch_column_id_rank_power_batched("sketch_column_id_rank_power_batched_complex", True, a, k, tol, power_iterations, omega, oversampling,
                                                seed, return_sketch)


def sketch_svd_rank_power_batched_complex(a: torch.Tensor, k: int, tol: float = 0.0, power_iterations: int = 1, omega: Optional[torch.Tensor] = None,
                                          oversampling: int = 8, seed: int = 0) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """sketch_svd_rank_power_batched for complex tall blocks: power_iterations - 1 full rounds (sketch_power_omega_batched_complex), one more
    range step with conj_p=False (Q, P = a Q^H, ranks), then lowrank_recompress_tall_batched_complex(left=P, right=Q, ranks=the step's ranks,
    k, tol): the reference's svd_from_range_estimate on a ~ (a Q^H) Q.  Returns (U [count, m, kk], S real [count, l], Vt = V^H
    [count, kk, n], ranks), kk = min(k, l).  power_iterations = 0 delegates to sketch_svd_rank_batched_complex on the same arguments.
    2 q launches, no host synchronisation.  Real data raises TypeError."""
    return _sketch_svd_rank_power_batched("sketch_svd_rank_power_batched_complex", True, a, k, tol, power_iterations, omega, oversampling, seed)


def packed_bytes(m: int, n: int, k: int, elem_size: int) -> int:
    """Bytes one matrix's factors take in the packed buffer: C (m x k) | Z (k x n) | pad to 8 | col_ind (n int64)
    (rc_batch_packed_bytes)."""
    return ((m * k + k * n) * elem_size + 7) // 8 * 8 + n * 8


def pack_factors(factors: Sequence[Tuple[torch.Tensor, torch.Tensor, torch.Tensor]]) -> torch.Tensor:
    """[(C, Z, col_ind), ...] -> one flat uint8 buffer in the layout of rc_batch_column_id_* (indices bit-cast, exact)."""
    parts = []
    for c, z, ind in factors:
        body = torch.cat([c.contiguous().reshape(-1), z.contiguous().reshape(-1)]).view(torch.uint8)
        pad = (-body.numel()) % 8
        if pad:
            body = torch.cat([body, torch.zeros(pad, dtype=torch.uint8, device=body.device)])
        parts += [body, ind.to(torch.int64).contiguous().view(torch.uint8)]
    return torch.cat(parts) if parts else torch.empty(0, dtype=torch.uint8)


def unpack_factors(buf: torch.Tensor, count: int, m: int, n: int, k: int, dtype: Optional[torch.dtype] = None):
    """Inverse of pack_factors / view of the buffer rc_batch_column_id_* fills: [(C, Z, col_ind), ...]."""
    if buf.dtype != torch.uint8:  # older callers packed in the factors' dtype
        dtype = dtype or buf.dtype
        buf = buf.contiguous().view(torch.uint8)
    if dtype is None:  # infer the scalar type from the buffer size
        dtype = next((d for d in (torch.float32, torch.float64) if packed_bytes(m, n, k, torch.empty(0, dtype=d).element_size()) * count == buf.numel()), None)
        assert dtype is not None, "unpack_factors: buffer size matches neither f32 nor f64 factors"
    es = torch.empty(0, dtype=dtype).element_size()
    per = packed_bytes(m, n, k, es)
    out = []
    for i in range(count):
        b = buf[i * per:(i + 1) * per]
        c = b[: m * k * es].view(dtype).reshape(m, k)
        z = b[m * k * es: (m * k + k * n) * es].view(dtype).reshape(k, n)
        ind = b[per - n * 8:].view(torch.int64)
        out.append((c, z, ind))
    return out


class _LanePool:
    """Contexts + HIP streams for the lock-step batch (created once per device, reused)."""

    _pools = {}

    @classmethod
    def get(cls, device: int, lanes: int):
        from . import _lib

        pool = cls._pools.setdefault(device, [])
        while len(pool) < lanes:
            raw = ctypes.c_void_p()
            st = _lib.lib().rc_stream_create(ctypes.c_int32(device), ctypes.byref(raw))
            if st != 0:
                raise _lib.HipRuntimeError("rc_stream_create failed")
            pool.append(_lib.Context(device, raw.value))
        return pool[:lanes]


def batch_column_id_packed(matrices: Sequence[torch.Tensor], k: int, lanes: int = 8) -> torch.Tensor:
    """rc_batch_column_id_*: rank-k column ID of same-shaped device matrices -> packed uint8 device buffer."""
    from . import _lib
    from .types import as_device

    mats = [as_device(a) for a in matrices]
    if not mats:
        return torch.empty(0, dtype=torch.uint8, device="cuda")
    m, n = mats[0].shape
    k = min(int(k), m, n)
    dev = mats[0].device.index if mats[0].device.index is not None else torch.cuda.current_device()
    es = mats[0].element_size()
    per = packed_bytes(m, n, k, es)
    out = torch.empty(len(mats) * per, dtype=torch.uint8, device=mats[0].device)
    ctxs = _LanePool.get(dev, max(1, min(lanes, len(mats))))
    arr = (ctypes.c_void_p * len(ctxs))(*[c._h.value for c in ctxs])
    marr = (_lib.rc_matrix * len(mats))(*[_lib.mat(a) for a in mats])
    torch.cuda.current_stream(dev).synchronize()  # the inputs were produced on torch's stream, the lanes have their own
    fn = getattr(_lib.lib(), f"rc_batch_column_id_{_lib.suffix(mats[0].dtype)}")
    ctxs[0].check(fn(arr, ctypes.c_int32(len(ctxs)), marr, ctypes.c_int32(len(mats)), ctypes.c_int64(k), ctypes.c_void_p(out.data_ptr())))
    return out


class Comm:
    """rc_comm_*: the library's RCCL communicator for the factor gather (one process per GPU)."""

    def __init__(self, world: int, rank: int, unique_id: bytes, device: Optional[int] = None):
        from . import _lib

        self.world, self.rank = int(world), int(rank)
        self.device = torch.cuda.current_device() if device is None else int(device)
        self._h = ctypes.c_void_p()
        st = _lib.lib().rc_comm_init(ctypes.byref(self._h), ctypes.c_int32(world), ctypes.c_int32(rank), ctypes.c_char_p(unique_id), ctypes.c_int32(self.device))
        if st != 0:
            raise _lib.HipRuntimeError(f"rc_comm_init failed with status {st}")

    @classmethod
    def from_process_group(cls, group=None, device: Optional[int] = None) -> "Comm":
        """The library's RCCL communicator for the ranks of a torch.distributed group: rank 0 draws the unique id
        (rc_comm_unique_id) and the group carries its 128 bytes to the others once; every later byte moves through rc_comm_gather."""
        import torch.distributed as dist

        world, rank = dist.get_world_size(group), dist.get_rank(group)
        dev = torch.cuda.current_device() if device is None else int(device)
        ident = torch.zeros(128, dtype=torch.uint8)
        if rank == 0:
            ident = torch.frombuffer(bytearray(cls.unique_id()), dtype=torch.uint8).clone()
        if dist.get_backend(group) == "nccl":
            ident = ident.cuda(dev)
        dist.broadcast(ident, src=dist.get_global_rank(group, 0) if group is not None else 0, group=group)
        return cls(world, rank, bytes(ident.cpu().numpy().tobytes()), dev)

    @staticmethod
    def unique_id() -> bytes:
        from . import _lib

        buf = ctypes.create_string_buffer(128)
        st = _lib.lib().rc_comm_unique_id(buf)
        if st != 0:
            raise _lib.HipRuntimeError(f"rc_comm_unique_id failed with status {st} (librccl not available?)")
        return buf.raw

    def gather(self, send: torch.Tensor, root: int = 0) -> Optional[torch.Tensor]:
        """Gather equal-sized uint8 device buffers to `root` (returns the concatenation there, None elsewhere)."""
        from . import _lib

        send = send.contiguous()
        nbytes = send.numel() * send.element_size()
        recv = torch.empty(self.world * nbytes, dtype=torch.uint8, device=send.device) if self.rank == root else None
        ctx = _lib.default_context()
        st = _lib.lib().rc_comm_gather(self._h, ctx._h, ctypes.c_void_p(send.data_ptr()), ctypes.c_void_p(recv.data_ptr() if recv is not None else None),
                                       ctypes.c_size_t(nbytes), ctypes.c_int32(root))
        ctx.check(st)
        ctx.synchronize()
        return recv

    def close(self):
        from . import _lib

        if self._h.value:
            _lib.lib().rc_comm_destroy(self._h)
            self._h = ctypes.c_void_p()


def batch_column_id(matrices: Sequence[torch.Tensor], k: int, compute: Optional[Callable] = None,
                    group=None, dst: int = 0, comm: Optional[Comm] = None, lanes: int = 8) -> Optional[List[Tuple[torch.Tensor, torch.Tensor, torch.Tensor]]]:
    """Compress the local shard `matrices` (this rank's block of the global batch) and gather every
    rank's factors on `dst` in global matrix order.  Returns the full list on `dst`, None elsewhere.
    All ranks must hold the same number of same-shaped matrices (8 per GPU in configs[4]).

    compute: optional per-matrix function (a, k) -> (C, Z, col_ind) replacing the device path (the gloo tests inject the CPU
    oracle); comm: the library's RCCL communicator (otherwise torch.distributed when a process group is active)."""
    import torch.distributed as dist

    if not matrices:
        return []
    m, n = matrices[0].shape
    if compute is None:
        packed = batch_column_id_packed(matrices, k, lanes)
        kk = min(int(k), m, n)
        dtype = matrices[0].dtype
    else:
        local = [compute(a, k) for a in matrices]
        kk = local[0][0].shape[1]
        dtype = local[0][0].dtype
        packed = pack_factors(local)
    nloc = len(matrices)
    if comm is not None and comm.world > 1:
        got = comm.gather(packed, dst)
        if comm.rank != dst:
            return None
        return unpack_factors(got, comm.world * nloc, m, n, kk, dtype)
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(group) == 1:
        return unpack_factors(packed, nloc, m, n, kk, dtype)
    world, rank = dist.get_world_size(group), dist.get_rank(group)
    gathered = [torch.empty_like(packed) for _ in range(world)] if rank == dst else None
    dist.gather(packed, gathered, dst=dst, group=group)   # the ONLY collective on this path
    if rank != dst:
        return None
    out = []
    for r in range(world):
        out += unpack_factors(gathered[r], nloc, m, n, kk, dtype)
    return out
