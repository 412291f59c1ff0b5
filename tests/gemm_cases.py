"""Shared pieces of the GEMM tests (tests/test_gpu_parity.py, tests/test_gpu_complex_edges.py, tests/test_gpu_gemm_arms.py):
the dispatch table, device operands of a chosen layout and staging width, C views, the rc_gemm_* call and what it launched."""
import ctypes
import re

import numpy as np
import torch

TORCH = {np.dtype(np.complex128): torch.complex128, np.dtype(np.complex64): torch.complex64,
         np.dtype(np.float64): torch.float64, np.dtype(np.float32): torch.float32}


def tdt(dtype):
    return TORCH[np.dtype(dtype)]


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def view(x, kind, fill=None):
    """x (m x n) as a device view: "C" row-major, "T" the transpose of a contiguous n x m (column-major), "P" a column-major
    sub-view of a larger buffer with an odd leading dimension.  Returns (view, buffer); the buffer's border holds `fill`."""
    m, n = x.shape
    dt = tdt(x.dtype)
    if kind == "C":
        t = dev(x)
        return t, t
    if kind == "T":
        t = dev(x.T)
        return t.t(), t
    ld = m + 3 if (m + 3) % 2 else m + 4
    fill = complex(7.0, -3.0) if fill is None else fill
    buf = torch.full((n + 2, ld), fill if dt.is_complex else fill.real, dtype=dt, device="cuda")
    buf[1:n + 1, 2:m + 2] = torch.from_numpy(np.ascontiguousarray(x.T)).cuda()
    v = buf[1:n + 1, 2:m + 2].t()
    assert v.stride() == (1, ld) and ld % 2 == 1
    return v, buf


def gemm(opa, opb, alpha, a, b, beta, c):
    """c <- alpha op(a) op(b) + beta c through rc_gemm_* of c's scalar type, on the default context."""
    from rusty_compression_amd import _lib

    dt = c.dtype
    _lib.default_context().call(f"rc_gemm_{_lib.suffix(dt)}", ctypes.c_int32(opa), ctypes.c_int32(opb), _lib.scalar_arg(dt, alpha),
                                _lib.mat(a), _lib.mat(b), _lib.scalar_arg(dt, beta), _lib.mat(c))
    torch.cuda.synchronize()


def last_gemm_kernel():
    """The instantiation of the most recent GEMM launch on the default context, as rocprofv3 names it."""
    from rusty_compression_amd import _lib

    fn = _lib.lib().rc_last_gemm_kernel_name
    fn.restype = ctypes.c_char_p
    fn.argtypes = [ctypes.c_void_p]
    return fn(_lib.default_context()._h).decode()


_PRODUCT = re.compile(r"kernel:k_gemm_mfma<f(?:64|32)> M=(\d+) N=(\d+) K=(\d+)")
_REDUCE = re.compile(r"kernel:k_splitk_reduce M=(\d+) N=(\d+) splits=(\d+)")


def gemm_traced(alpha, a, b, beta, c):
    """One real rc_gemm_* call (no op flags) with the event profile of the default context switched on.  Returns
    (instantiation launched, (M, N) of the problem as dispatched -- (n, m) when it ran as the transposed problem --, number of
    K slabs: 1 when no kernel:k_splitk_reduce label was recorded).  The caller orders its reads of c on the same stream."""
    from rusty_compression_amd import _lib

    ctx = _lib.default_context()
    lib = _lib.lib()
    dt = c.dtype
    ctx.check(lib.rc_profile_enable(ctx._h, 1))
    try:
        ctx.check(lib.rc_profile_reset(ctx._h))
        ctx.call(f"rc_gemm_{_lib.suffix(dt)}", ctypes.c_int32(0), ctypes.c_int32(0), _lib.scalar_arg(dt, alpha),
                 _lib.mat(a), _lib.mat(b), _lib.scalar_arg(dt, beta), _lib.mat(c))
        name = last_gemm_kernel()
        cnt = ctypes.c_int32(0)
        ctx.check(lib.rc_profile_count(ctx._h, ctypes.byref(cnt)))
        shape, splits = None, 1
        for i in range(cnt.value):
            label = ctypes.create_string_buffer(192)
            ms, calls = ctypes.c_double(0), ctypes.c_int64(0)
            ctx.check(lib.rc_profile_get(ctx._h, i, label, 192, ctypes.byref(ms), ctypes.byref(calls)))
            text = label.value.decode()
            mt = _PRODUCT.match(text)
            if mt:
                assert shape is None and calls.value == 1, text
                shape = (int(mt.group(1)), int(mt.group(2)))
            mt = _REDUCE.match(text)
            if mt:
                assert splits == 1 and calls.value == 1, text
                splits = int(mt.group(3))
                assert splits > 1, text
    finally:
        lib.rc_profile_enable(ctx._h, 0)
        lib.rc_profile_reset(ctx._h)
    assert shape is not None, "no kernel:k_gemm_mfma label was recorded"
    return name, shape, splits


def gemm_operand(x, layout):
    """`x` on the device: "C" row-major / "F" column-major with an even leading dimension (16-byte vector staging),
    "c" row-major with an odd leading dimension (scalar staging)."""
    r, c = x.shape
    if layout == "F":
        t = torch.zeros((c, r + (r & 1)), dtype=torch.from_numpy(x).dtype, device="cuda")[:, :r]
        t.copy_(torch.from_numpy(np.ascontiguousarray(x.T)))
        return t.t()
    ld = c + (c & 1) if layout == "C" else c + 1 - (c & 1)
    t = torch.zeros((r, ld), dtype=torch.from_numpy(x).dtype, device="cuda")[:, :c]
    t.copy_(torch.from_numpy(x))
    return t


# Every arm of the GEMM dispatch (kernels_gemm.hip launch_shape_f64q / launch_shape, kernels_gemm_pipe.hip gemm_f64p_launch) with
# the instantiation it launches: (dtype, layout of A, layout of B, M, N, K, kernel).  "C" A / "F" B: K-contiguous; "F" A: M-contiguous;
# "C" B: N-contiguous.  f64 products with N <= 144 under M > 144 run as the transposed problem.
GEMM_DISPATCH = [
    # f64: the n x n Gram products (pipelined loop for the two CholeskyQR layouts), 144 x 144 tiles otherwise
    ("f64", "C", "F", 100, 100, 512, "k_gemm_f64p<0,1,144,144,16,3,3,0>"),
    ("f64", "F", "C", 100, 100, 512, "k_gemm_f64p<1,0,144,144,16,3,3,0>"),
    ("f64", "C", "C", 100, 100, 512, "k_gemm_f64q<0,0,144,144,16,3,3,2,0,0>"),
    ("f64", "C", "F", 100, 100, 40, "k_gemm_f64q<0,1,144,144,16,3,3,2,0,0>"),
    ("f64", "c", "C", 100, 100, 97, "k_gemm_f64q<0,0,144,144,16,3,3,1,0,0>"),
    # f64 skinny N
    ("f64", "C", "C", 100, 64, 256, "k_gemm_f64q<0,0,256,80,16,8,1,2,0,0>"),
    ("f64", "C", "C", 60, 128, 256, "k_gemm_f64q<0,0,256,128,16,8,1,2,0,0>"),
    ("f64", "C", "C", 60, 136, 256, "k_gemm_f64q<0,0,256,144,16,8,1,2,0,0>"),
    # f64 skinny M: 32-row panel products, <= 80 rows, shallow K over a wide N
    ("f64", "C", "C", 32, 512, 1024, "k_gemm_f64q<0,0,32,256,16,1,8,2,1,0>"),
    ("f64", "C", "C", 64, 512, 256, "k_gemm_f64q<0,0,80,256,16,1,8,2,1,0>"),
    ("f64", "C", "C", 128, 2048, 128, "k_gemm_f64q<0,0,128,128,16,1,8,2,1,0>"),
    ("f64", "F", "F", 136, 2048, 128, "k_gemm_f64q<1,1,136,128,16,2,4,2,0,0>"),
    # f64 <= 128 rows: the projection on the ring kernel; direct-to-LDS B tile; register staging
    ("f64", "F", "C", 128, 512, 256, "k_gemm_f64r<0,1,128,256,1,8,false,0>"),
    ("f64", "F", "C", 100, 300, 256, "k_gemm_f64r<0,1,128,256,1,8,false,0>"),
    ("f64", "C", "C", 128, 512, 256, "k_gemm_f64q<0,0,128,256,16,1,8,2,1,1>"),
    ("f64", "F", "C", 100, 300, 40, "k_gemm_f64q<1,0,128,256,16,1,8,2,1,0>"),
    ("f64", "C", "C", 1000, 100, 256, "k_gemm_f64q<1,1,128,256,16,1,8,2,1,0>"),
    # f64 129 .. 136 rows: the sketch on the ring kernel, the pipelined loop, the plain loop
    ("f64", "F", "F", 133, 512, 256, "k_gemm_f64r<1,0,136,256,2,4,true,0>"),
    ("f64", "F", "F", 133, 300, 256, "k_gemm_f64p<1,1,136,256,16,2,4,0>"),
    ("f64", "F", "F", 133, 512, 40, "k_gemm_f64q<1,1,136,256,16,2,4,2,0,0>"),
    ("f64", "F", "C", 133, 512, 256, "k_gemm_f64q<1,0,136,256,16,2,4,2,0,0>"),
    # f64 137 .. 144 rows, and everything larger
    ("f64", "F", "F", 140, 512, 256, "k_gemm_f64q<1,1,144,256,16,1,8,2,1,0>"),
    ("f64", "C", "C", 300, 300, 256, "k_gemm_f64q<0,0,128,128,16,2,2,2,0,0>"),
    # f32
    ("f32", "C", "C", 100, 100, 256, "k_gemm_mfma<float,0,0,144,144,16,3,3,2,2>"),
    ("f32", "C", "C", 300, 64, 256, "k_gemm_mfma<float,0,0,128,80,16,4,1,2,2>"),
    ("f32", "C", "C", 300, 136, 256, "k_gemm_mfma<float,0,0,256,144,16,8,1,2,2>"),
    ("f32", "C", "F", 32, 512, 1024, "k_gemm_mfma<float,0,1,32,128,16,1,4,2,2>"),
    ("f32", "C", "C", 32, 512, 1024, "k_gemm_mfma<float,0,0,80,128,16,1,4,2,2>"),
    ("f32", "C", "C", 64, 512, 256, "k_gemm_mfma<float,0,0,80,128,16,1,4,2,2>"),
    ("f32", "C", "C", 128, 512, 256, "k_gemm_mfma<float,0,0,144,256,16,1,8,2,2>"),
    ("f32", "C", "C", 300, 300, 256, "k_gemm_mfma<float,0,0,128,128,16,2,2,2,2>"),
    ("f32", "c", "C", 300, 300, 255, "k_gemm_mfma<float,0,0,128,128,16,2,2,1,2>"),
]
