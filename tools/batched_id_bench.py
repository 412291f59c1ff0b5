#!/usr/bin/env python3
"""Throughput of the batched small-matrix column ID (rc_column_id_rank_batched_*) against a loop of rc_column_id_rank_* calls.

For each shape: one batched call timed with device events after warm-up (median of --repeats), the same matrices through a
loop of lone calls on the same stream (the first --loop-count of them: the loop is host-bound and slow, so a subset is timed
and scaled per matrix), a check that both take the same pivots on the agreed prefix, and the algorithmic bytes (A read once;
C, Z, col_ind written) over the batched time as a share of HBM bandwidth.  Not used by the tests or by bench.py.

--two-sided times, on the same shapes and matrices, the batched column ID, the batched two-sided ID
(rc_two_sided_id_rank_batched_*) and a loop of lone rc_column_id_rank_* + rc_column_id_two_sided_* calls on a subset, and writes
profiles/batched_two_sided_bench.json unless --out names another file.

--complex runs the same shapes with complex scalars (c64 / c32 / c64 in place of f64 / f32 / f64): the batched complex calls
(rc_column_id_rank_batched_c*, with --two-sided rc_two_sided_id_rank_batched_c*) against a loop of lone rc_column_id_rank_c* (+
rc_column_id_two_sided_c*) calls, next to the real batched call of the same shape timed in the same process; the results go to
profiles/batched_id_complex_bench.json / profiles/batched_id_complex_two_sided_bench.json unless --out names another file.

    python tools/batched_id_bench.py [--two-sided] [--complex] [--repeats 5] [--loop-count 64] [--shapes 0,1,2] [--out path.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import rusty_compression_amd as rc  # noqa: E402
from rusty_compression_amd.batch import column_id_rank  # noqa: E402
from tests.helpers import agreed_pivot_prefix  # noqa: E402

HBM_BYTES_PER_S = 8.0e12  # MI355X HBM3E peak (spec); measured copy ceiling 6.29 TB/s
SHAPES = [  # (count, m, n, k, tol, dtype)
    (2048, 512, 256, 32, 0.0, torch.float64),
    (8192, 256, 256, 32, 0.0, torch.float32),
    (16384, 128, 128, 64, 1e-8, torch.float64),
]
COMPLEX_OF = {torch.float64: torch.complex128, torch.float32: torch.complex64}


def timed(fn, repeats):
    ts = []
    for _ in range(repeats):
        b, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        b.record()
        fn()
        e.record()
        e.synchronize()
        ts.append(b.elapsed_time(e) * 1e-3)
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def decaying_batch(count, m, n, dtype, seed):
    """A = U diag(logspace(0, -10)) V^H per matrix with Gaussian U, V scaled to unit expected column norms (a decaying spectrum,
    generated on the device without a batched QR); complex Gaussian U, V for a complex dtype."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    r = min(m, n)
    wide = torch.complex128 if dtype.is_complex else torch.float64
    u = torch.randn(count, m, r, generator=g, device="cuda", dtype=wide) / m ** 0.5
    v = torch.randn(count, n, r, generator=g, device="cuda", dtype=wide) / n ** 0.5
    s = torch.logspace(0, -10, r, device="cuda", dtype=torch.float64)
    return ((u * s) @ v.transpose(1, 2).conj()).to(dtype).contiguous()


def shape_of(args, si):
    """SHAPES[si], with the complex scalar of the same precision under --complex."""
    count, m, n, k, tol, dtype = SHAPES[si]
    return count, m, n, k, tol, COMPLEX_OF[dtype] if args.complex else dtype


def real_batched_s(args, si, two_sided):
    """Under --complex: the real batched call of the same shape (the input of the real run), timed here for the comparison."""
    if not args.complex:
        return {}
    count, m, n, k, tol, dtype = SHAPES[si]
    a = decaying_batch(count, m, n, dtype, 1234 + si)
    fn = (lambda: rc.two_sided_id_rank_batched(a, k, tol)) if two_sided else (lambda: rc.column_id_rank_batched(a, k, tol))
    fn()
    torch.cuda.synchronize()
    med = timed(fn, args.repeats)[0]
    del a
    torch.cuda.empty_cache()
    return dict(real_dtype=str(dtype).replace("torch.", ""), real_batched_s=med)


def real_dtype_np(dtype):
    return np.dtype(np.float64 if dtype in (torch.float64, torch.complex128) else np.float32)


def two_sided_rows(args):
    """Batched column ID, batched two-sided ID and the loop of lone column ID + two-sided calls, per shape."""
    results = []
    for si in [int(x) for x in args.shapes.split(",")]:
        count, m, n, k, tol, dtype = shape_of(args, si)
        real = real_batched_s(args, si, True)
        a = decaying_batch(count, m, n, dtype, 1234 + si)
        kk = min(k, m, n)
        rc.column_id_rank_batched(a, k, tol)  # warm-up (code objects, workspace)
        c, x, r, row_ind, col_ind, ranks = rc.two_sided_id_rank_batched(a, k, tol)
        torch.cuda.synchronize()
        b_med, b_min, b_max = timed(lambda: rc.column_id_rank_batched(a, k, tol), args.repeats)
        t_med, t_min, t_max = timed(lambda: rc.two_sided_id_rank_batched(a, k, tol), args.repeats)
        nl = min(args.loop_count, count)
        ranks_h = ranks.cpu().numpy()

        def loop():  # the lone chain at each matrix's own rank, as a user of the lone calls would run it
            for i in range(nl):
                ci, zi, ind = column_id_rank(a[i], int(ranks_h[i]) or 1)
                rc.ColumnID(ci, zi, ind).two_sided_id()

        loop()
        l_med, l_min, l_max = timed(loop, max(1, args.repeats // 2))
        # row pivots against the lone chain started from the batch's own column ID (identical bits on both sides)
        agree = []
        for i in range(min(nl, 8)):
            ri = int(ranks_h[i])
            cols = col_ind[i, :ri]
            lone = rc.ColumnID(a[i][:, cols].contiguous(), r[i, :ri].contiguous(), col_ind[i].clone()).two_sided_id()
            mine, lrow = row_ind[i].cpu().numpy(), lone.row_ind.cpu().numpy()
            ct = a[i][:, cols].to(torch.complex128 if dtype.is_complex else torch.float64).cpu().numpy().conj().T
            agree.append(int(agreed_pivot_prefix(mine, np.linalg.qr(ct[:, mine], mode="r")[:ri], lrow, np.linalg.qr(ct[:, lrow], mode="r")[:ri],
                                                 real_dtype_np(dtype))))
        row = dict(count=count, m=m, n=n, k=k, tol=tol, dtype=str(dtype).replace("torch.", ""),
                   column_id_s=b_med, column_id_matrices_per_s=count / b_med,
                   two_sided_s=t_med, two_sided_s_min=t_min, two_sided_s_max=t_max, two_sided_matrices_per_s=count / t_med,
                   two_sided_over_column_id=b_med / t_med,
                   loop_matrices=nl, loop_s=l_med, loop_matrices_per_s=nl / l_med, speedup=(count / t_med) / (nl / l_med),
                   ranks_min=int(ranks_h.min()), ranks_max=int(ranks_h.max()), row_pivots_agreed_prefix=agree, kk=kk)
        if real:
            row.update(real, two_sided_over_real=t_med / real["real_batched_s"])
        results.append(row)
        print(json.dumps(row), flush=True)
        del a, c, x, r, row_ind, col_ind, ranks
        torch.cuda.empty_cache()
    return results


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--loop-count", type=int, default=64)
    ap.add_argument("--shapes", default="0,1,2")
    ap.add_argument("--out", default="")
    ap.add_argument("--two-sided", action="store_true")
    ap.add_argument("--complex", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("batched_id_bench: no GPU visible (this tool only measures on the device)")
    torch.cuda.set_device(0)
    if args.two_sided:
        results = two_sided_rows(args)
        default = "batched_id_complex_two_sided_bench.json" if args.complex else "batched_two_sided_bench.json"
        with open(args.out or os.path.join(ROOT, "profiles", default), "w") as f:
            json.dump(results, f, indent=1)
        return
    results = []
    for si in [int(x) for x in args.shapes.split(",")]:
        count, m, n, k, tol, dtype = shape_of(args, si)
        real = real_batched_s(args, si, False)
        a = decaying_batch(count, m, n, dtype, 1234 + si)
        es = a.element_size()
        c, z, ind, ranks = rc.column_id_rank_batched(a, k, tol)  # warm-up (code objects, workspace)
        torch.cuda.synchronize()
        t_med, t_min, t_max = timed(lambda: rc.column_id_rank_batched(a, k, tol), args.repeats)
        nl = min(args.loop_count, count)
        kk = min(k, m, n)
        column_id_rank(a[0], kk)  # warm-up of the lone path

        def loop():
            for i in range(nl):
                column_id_rank(a[i], kk)

        l_med, l_min, l_max = timed(loop, max(1, args.repeats // 2))
        # pivots: the lone call runs at fixed rank k; compare on the prefix both determine
        agree = []
        ind_h, ranks_h = ind.cpu().numpy(), ranks.cpu().numpy()
        for i in range(min(nl, 8)):
            _, _, lind = column_id_rank(a[i], kk)
            an = a[i].to(torch.complex128 if dtype.is_complex else torch.float64).cpu().numpy()
            r = int(ranks_h[i])
            mine = np.linalg.qr(an[:, ind_h[i]], mode="r")[:r]
            ref = np.linalg.qr(an[:, lind.cpu().numpy()], mode="r")[:r]
            agree.append(int(agreed_pivot_prefix(ind_h[i], mine, lind.cpu().numpy(), ref, real_dtype_np(dtype))))
        bytes_alg = count * ((m * n + m * kk + kk * n) * es + n * 8 + 8)
        row = dict(count=count, m=m, n=n, k=k, tol=tol, dtype=str(dtype).replace("torch.", ""),
                   batched_s=t_med, batched_s_min=t_min, batched_s_max=t_max, batched_matrices_per_s=count / t_med,
                   loop_matrices=nl, loop_s=l_med, loop_matrices_per_s=nl / l_med, speedup=(count / t_med) / (nl / l_med),
                   ranks_min=int(ranks_h.min()), ranks_max=int(ranks_h.max()), pivots_agreed_prefix=agree,
                   algorithmic_bytes=bytes_alg, hbm_share=bytes_alg / t_med / HBM_BYTES_PER_S,
                   bound="not HBM: %.1f %% of the 8 TB/s peak; the k serial Householder steps of each matrix inside its workgroup"
                   % (100 * bytes_alg / t_med / HBM_BYTES_PER_S))
        if real:
            row.update(real, complex_over_real=t_med / real["real_batched_s"])
        results.append(row)
        print(json.dumps(row), flush=True)
        del a, c, z, ind, ranks
        torch.cuda.empty_cache()
    if args.out or args.complex:
        with open(args.out or os.path.join(ROOT, "profiles", "batched_id_complex_bench.json"), "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
