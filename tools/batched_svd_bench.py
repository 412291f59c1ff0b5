#!/usr/bin/env python3
"""Throughput of the batched truncated SVD (rc_svd_rank_batched_*) against a loop of lone rc_compute_svd_* calls.

For each shape: one batched call timed with device events after warm-up (median of --repeats); the same matrices through a loop
of lone rc_compute_svd_* + rc_svd_rank_by_tolerance_* calls (SVD.compute_from + compress_svd_tolerance, a synchronous round trip
per matrix) on the first --loop-count of them, scaled per matrix; the largest singular-value difference between the two on that
subset (relative to s_0); and on the 128 x 128 shape the batched column ID (rc_column_id_rank_batched_*) of the same matrices.
Writes profiles/batched_svd_bench.json unless --out names another file.  Not used by the tests or by bench.py.

--complex runs COMPLEX_SHAPES through rc_svd_rank_batched_c64 / _c32 (svd_rank_batched_complex) instead; the lone loop is then
rc_compute_svd_c* + rc_svd_rank_by_tolerance_* (slow: keep --loop-count small), and each row also times the real batched call
(rc_svd_rank_batched_f64 / _f32) on a real batch of the same shape.  Writes profiles/batched_svd_complex_bench.json by default.

    python tools/batched_svd_bench.py [--complex] [--repeats 5] [--loop-count 32] [--shapes 0,1,2,3] [--out path.json]
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
from tools.batched_id_bench import decaying_batch, timed  # noqa: E402

SHAPES = [  # (count, m, n, k, tol, dtype)
    (16384, 128, 128, 64, 1e-8, torch.float64),
    (4096, 512, 128, 32, 0.0, torch.float64),
    (4096, 128, 512, 32, 0.0, torch.float64),
    (16384, 64, 64, 16, 0.0, torch.float32),
]
COMPLEX_SHAPES = [  # the 128 x 128 c64 core lives in the workspace, the 96 x 96 one in LDS: the two sides of the plan boundary
    (16384, 128, 128, 64, 1e-8, torch.complex128),
    (16384, 96, 96, 48, 0.0, torch.complex128),
    (4096, 512, 128, 32, 0.0, torch.complex128),
    (4096, 128, 512, 32, 0.0, torch.complex128),
    (16384, 64, 64, 16, 0.0, torch.complex64),
]
REAL_OF = {torch.complex128: torch.float64, torch.complex64: torch.float32}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--loop-count", type=int, default=32)
    ap.add_argument("--shapes", default=None)
    ap.add_argument("--complex", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs an MI355X")
    shapes = COMPLEX_SHAPES if args.complex else SHAPES
    call = rc.svd_rank_batched_complex if args.complex else rc.svd_rank_batched
    out_path = args.out or os.path.join(ROOT, "profiles", "batched_svd_complex_bench.json" if args.complex else "batched_svd_bench.json")
    results = []
    for si in [int(x) for x in (args.shapes or ",".join(str(i) for i in range(len(shapes)))).split(",")]:
        count, m, n, k, tol, dtype = shapes[si]
        a = decaying_batch(count, m, n, dtype, 4321 + si)
        u, s, vt, ranks = call(a, k, tol)  # warm-up (code objects, workspace)
        torch.cuda.synchronize()
        b_med, b_min, b_max = timed(lambda: call(a, k, tol), args.repeats)
        nl = min(args.loop_count, count)

        def loop():  # the lone path as a user runs it: compute_svd, then the rank from the tolerance (a host round trip)
            for i in range(nl):
                svd = rc.SVD.compute_from(a[i])
                svd.compress_svd_tolerance(tol) if tol > 0 else svd.compress_svd_rank(k)

        loop()
        torch.cuda.synchronize()
        l_med, l_min, l_max = timed(loop, max(1, args.repeats // 2))
        sdiff = 0.0
        for i in range(min(nl, 8)):
            ls = rc.SVD.compute_from(a[i]).s.double()
            sdiff = max(sdiff, float((s[i].double() - ls).abs().max() / ls[0]))
        rh = ranks.cpu().numpy()
        row = dict(count=count, m=m, n=n, k=k, tol=tol, dtype=str(dtype).replace("torch.", ""),
                   batched_s=b_med, batched_s_min=b_min, batched_s_max=b_max, batched_matrices_per_s=count / b_med,
                   loop_matrices=nl, loop_s=l_med, loop_matrices_per_s=nl / l_med, speedup=(count / b_med) / (nl / l_med),
                   ranks_min=int(rh.min()), ranks_max=int(rh.max()), s_max_rel_diff_vs_lone=sdiff)
        if args.complex:  # the real batched call of the same shape
            ar = decaying_batch(count, m, n, REAL_OF[dtype], 4321 + si)
            rc.svd_rank_batched(ar, k, tol)
            torch.cuda.synchronize()
            r_med = timed(lambda: rc.svd_rank_batched(ar, k, tol), args.repeats)[0]
            row.update(real_batched_s=r_med, real_matrices_per_s=count / r_med, complex_over_real=b_med / r_med)
            del ar
        elif (m, n) == (128, 128):
            rc.column_id_rank_batched(a, k, tol)
            torch.cuda.synchronize()
            c_med = timed(lambda: rc.column_id_rank_batched(a, k, tol), args.repeats)[0]
            row.update(column_id_batched_s=c_med, column_id_matrices_per_s=count / c_med)
        results.append(row)
        print(json.dumps(row), flush=True)
        del a, u, s, vt, ranks
        torch.cuda.empty_cache()
    health = rc.default_context().get_health()
    out = dict(tool="tools/batched_svd_bench.py", device=torch.cuda.get_device_name(0), health_word=health, results=results)
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", out_path)


if __name__ == "__main__":
    main()
