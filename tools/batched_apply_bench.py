#!/usr/bin/env python3
"""Throughput of the batched apply / to_mat (rc_lowrank_apply_batched_*) against a loop of lone rc_gemm_* calls and a torch.bmm chain.

For each shape the factors come from the real batched calls (column ID everywhere; two-sided ID and SVD on the 128 x 128 f64 shape),
so the ranks are the tolerance's.  Each run -- one right-hand side, 16 right-hand sides, reconstruction -- is one batched call timed
with device events after warm-up (median of --repeats).  Baselines: the same product as two or three lone rc_gemm_* calls per block on
the first --loop-count blocks (rank-aware through host-side slices of the factors), scaled per block; and a torch.bmm chain over the
full batch, which ignores the ranks and relies on the zero tails.  Bytes are algorithmic: the first r columns / rows of each factor,
b and y, once each; the fraction is of the 6.29 TB/s a float4 copy reaches on the MI355X.
Writes profiles/batched_apply_bench.json unless --out names another file.  Not used by the tests or by bench.py.

--mixed measures the mixed-storage call instead (rc_lowrank_apply_mixed_batched_f64 / _c64: factors kept in f32 / c32): on the f64 and
c128 shapes, the column-ID factors are demoted (rc_demote_batched_*) and promoted back, and each run times, in the same process and by
the same method, the full-precision call on the promoted factors (the yardstick: this library's unchanged kernel) and the mixed call on
the stored ones; the two results are checked to be the same bits.  Bytes are counted as above with the factor elements at their stored
size, so bytes_ratio is the ceiling of the speed-up.  Writes profiles/batched_apply_mixed_bench.json.

    python tools/batched_apply_bench.py [--repeats 5] [--loop-count 64] [--shapes 0,1,2,3] [--out path.json] [--mixed]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import rusty_compression_amd as rc  # noqa: E402
from tools.batched_id_bench import decaying_batch, timed  # noqa: E402

SHAPES = [  # (count, m, n, k, tol, dtype): the README's batched shapes and one c64 shape
    (16384, 128, 128, 64, 1e-8, torch.float64),
    (2048, 512, 256, 32, 0.0, torch.float64),
    (8192, 256, 256, 32, 0.0, torch.float32),
    (8192, 128, 128, 64, 1e-8, torch.complex128),
]
COPY_BW = 6.29e12  # bytes/s, measured float4 copy


def factor(form, a, k, tol):
    """(left, mid, s, right, ranks) of the batch through the real batched call of `form`."""
    if form == "column_id":
        c, z, _, ranks = rc.column_id_rank_batched(a, k, tol)
        return c, None, None, z, ranks
    if form == "two_sided_id":
        c, x, r, _, _, ranks = rc.two_sided_id_rank_batched(a, k, tol)
        return c, x, None, r, ranks
    u, s, vt, ranks = (rc.svd_rank_batched_complex if a.dtype.is_complex else rc.svd_rank_batched)(a, k, tol)
    return u, None, s, vt, ranks


def main_mixed(args):
    out_path = args.out or os.path.join(ROOT, "profiles", "batched_apply_mixed_bench.json")
    results = []
    for si in [int(x) for x in (args.shapes or "0,1,3").split(",")]:
        count, m, n, k, tol, dtype = SHAPES[si]
        if dtype not in (torch.float64, torch.complex128):
            raise SystemExit(f"--mixed: shape {si} is {dtype}; the mixed calls compute in float64 / complex128")
        a = decaying_batch(count, m, n, dtype, 2468 + si)
        g = torch.Generator(device="cuda").manual_seed(97 + si)
        b16 = torch.randn(count, n, 16, generator=g, device="cuda", dtype=torch.float64).to(dtype)
        c, _, _, z, ranks = factor("column_id", a, k, tol)
        del a
        low = [rc.demote_batched(c), rc.demote_batched(z)]
        up = [rc.promote_batched(v) for v in low]
        del c, z
        torch.cuda.synchronize()
        rh = ranks.cpu()
        rsum = int(rh.sum())
        es, ss = up[0].element_size(), low[0].element_size()
        for mode, b in (("nrhs=1", b16[:, :, :1].contiguous()), ("nrhs=16", b16), ("to_mat", None)):
            ncols = n if b is None else b.shape[2]
            full = lambda: rc.lowrank_apply_batched(up[0], up[1], b=b, ranks=ranks)  # noqa: E731
            mixed = lambda: rc.lowrank_apply_batched_mixed(low[0], low[1], b=b, ranks=ranks)  # noqa: E731
            same = bool(torch.equal(full(), mixed()))  # warm-up of both code objects, and the contract
            torch.cuda.synchronize()
            # full, mixed, full again: the second full run shows how far the yardstick itself moves between two measurements
            t_full, t_mixed, t_again = timed(full, args.repeats), timed(mixed, args.repeats), timed(full, args.repeats)
            other = count * (m * ncols + (0 if b is None else n * ncols)) * es  # b and y, full precision in both calls
            bytes_full, bytes_mixed = rsum * (m + n) * es + other, rsum * (m + n) * ss + other
            row = dict(form="column_id", mode=mode, count=count, m=m, n=n, k=k, tol=tol, dtype=str(dtype).replace("torch.", ""),
                       storage=str(low[0].dtype).replace("torch.", ""), ranks_mean=rsum / count, bit_equal=same,
                       full_s=t_full[0], full_s_min=t_full[1], full_s_max=t_full[2], full_again_s=t_again[0],
                       mixed_s=t_mixed[0], mixed_s_min=t_mixed[1], mixed_s_max=t_mixed[2],
                       full_bytes=bytes_full, mixed_bytes=bytes_mixed, bytes_ratio=bytes_full / bytes_mixed,
                       full_bytes_per_block=bytes_full / count, mixed_bytes_per_block=bytes_mixed / count,
                       full_blocks_per_s=count / t_full[0], mixed_blocks_per_s=count / t_mixed[0], speedup=t_full[0] / t_mixed[0],
                       full_fraction_of_copy_bw=bytes_full / t_full[0] / COPY_BW, mixed_fraction_of_copy_bw=bytes_mixed / t_mixed[0] / COPY_BW)
            results.append(row)
            print(json.dumps(row), flush=True)
        del low, up, b16
        torch.cuda.empty_cache()
    out = dict(tool="tools/batched_apply_bench.py --mixed", device=torch.cuda.get_device_name(0), repeats=args.repeats,
               copy_bandwidth_bytes_per_s=COPY_BW, results=results)
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", out_path)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--loop-count", type=int, default=64)
    ap.add_argument("--shapes", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--mixed", action="store_true", help="time the mixed-storage call against the full-precision call on promoted factors")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs an MI355X")
    if args.mixed:
        return main_mixed(args)
    out_path = args.out or os.path.join(ROOT, "profiles", "batched_apply_bench.json")
    results = []
    for si in [int(x) for x in (args.shapes or ",".join(str(i) for i in range(len(SHAPES)))).split(",")]:
        count, m, n, k, tol, dtype = SHAPES[si]
        a = decaying_batch(count, m, n, dtype, 2468 + si)
        es = a.element_size()
        g = torch.Generator(device="cuda").manual_seed(97 + si)
        b16 = torch.randn(count, n, 16, generator=g, device="cuda", dtype=torch.float64).to(dtype)
        forms = ["column_id", "two_sided_id", "svd"] if (si == 0) else ["column_id"]
        for form in forms:
            left, mid, s, right, ranks = factor(form, a, k, tol)
            torch.cuda.synchronize()
            rh = ranks.cpu()
            rsum = int(rh.sum())
            nl = min(args.loop_count, count)
            for mode, b in (("nrhs=1", b16[:, :, :1].contiguous()), ("nrhs=16", b16), ("to_mat", None)):
                ncols = n if b is None else b.shape[2]
                fn = lambda: rc.lowrank_apply_batched(left, right, b=b, mid=mid, s=s, ranks=ranks)  # noqa: E731
                y = fn()  # warm-up (code objects)
                torch.cuda.synchronize()
                t_med, t_min, t_max = timed(fn, args.repeats)
                nbytes = rsum * (m + n) * es + (0 if mid is None else int((rh * rh).sum()) * es) + (0 if s is None else rsum * s.element_size())
                nbytes += count * (m * ncols + (0 if b is None else n * ncols)) * es

                def loop():  # what a caller without the batched call does: two or three lone GEMMs per block at its rank
                    for i in range(nl):
                        r = int(rh[i])
                        if r == 0:
                            continue
                        w = right[i, :r] if b is None else rc.dot(right[i, :r], b[i])
                        if s is not None:
                            w = s[i, :r, None] * w
                        if mid is not None:
                            w = rc.dot(mid[i, :r, :r], w)
                        rc.dot(left[i, :, :r], w)

                loop()
                torch.cuda.synchronize()
                l_med = timed(loop, max(1, args.repeats // 2))[0]

                def bmm():  # the generic batched GEMM chain: full k, intermediates through HBM
                    w = right if b is None else torch.bmm(right, b)
                    if s is not None:
                        w = s[:, :k, None] * w
                    if mid is not None:
                        w = torch.bmm(mid, w)
                    return torch.bmm(left, w)

                row = dict(form=form, mode=mode, count=count, m=m, n=n, k=k, tol=tol, dtype=str(dtype).replace("torch.", ""), ranks_min=int(rh.min()),
                           ranks_max=int(rh.max()), ranks_mean=rsum / count, batched_s=t_med, batched_s_min=t_min, batched_s_max=t_max,
                           blocks_per_s=count / t_med, algorithmic_bytes=nbytes, bytes_per_s=nbytes / t_med, fraction_of_copy_bw=nbytes / t_med / COPY_BW,
                           loop_blocks=nl, loop_s=l_med, loop_blocks_per_s=nl / l_med, speedup_vs_loop=(count / t_med) / (nl / l_med))
                try:
                    yb = bmm()
                    torch.cuda.synchronize()
                    b_med = timed(bmm, args.repeats)[0]
                    row.update(bmm_s=b_med, bmm_blocks_per_s=count / b_med, speedup_vs_bmm=b_med / t_med,
                               max_abs_diff_vs_bmm=float((y - yb).abs().max()), max_abs_y=float(yb.abs().max()))
                    del yb
                except RuntimeError as e:  # torch has no bmm for this dtype on this build
                    row.update(bmm_error=str(e).splitlines()[0])
                results.append(row)
                print(json.dumps(row), flush=True)
                del y
            del left, mid, s, right, ranks
        del a, b16
        torch.cuda.empty_cache()
    out = dict(tool="tools/batched_apply_bench.py", device=torch.cuda.get_device_name(0), copy_bandwidth_bytes_per_s=COPY_BW, results=results)
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", out_path)


if __name__ == "__main__":
    main()
