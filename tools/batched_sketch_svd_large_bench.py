#!/usr/bin/env python3
"""Throughput of the batched sketch product (rc_sketch_product_batched_*) and of the randomized SVD of wide blocks built on it
(batch.sketch_svd_rank_large_batched) beside what a caller had before them.

Blocks are Gaussian (the product's time does not depend on the values) with one shared Gaussian omega; every figure is timed with device
events after warm-up (median of --repeats, with the smallest and largest time as the spread).

  product    rc_sketch_product_batched_* alone: blocks/s, bytes of a per second as a share of the 6.29 TB/s copy bandwidth, and its time
             against torch.matmul(omega, a) on the same inputs.  At 2048 x 256 and 8192 x 128 the share stands beside the 0.10 and 0.29
             the whole sketched ID reached at those shapes, whose sketch is this product made by one workgroup per block.
  chain      sketch_svd_rank_large_batched at one and two range steps against the same chain with both products of every step made by
             torch.matmul (y = omega a, p = a q^T), which is what a caller of the parent commit had for n > 512.  The last, delegating
             shape (n <= 512) runs sketch_svd_rank_power_batched on both sides of the ratio, so it stands at 1 by construction and is
             recorded as a check.

Writes profiles/batched_sketch_svd_large_bench.json unless --out names another file.  Not used by the tests or by bench.py.

    python tools/batched_sketch_svd_large_bench.py [--repeats 5] [--shapes 0,1,2,3] [--out path.json]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import rusty_compression_amd as rc  # noqa: E402
from tools.batched_id_bench import timed  # noqa: E402

COPY_BW = 6.29e12
SHAPES = [  # (count, m, n, l, k, dtype)
    (512, 2048, 2048, 40, 32, torch.float64),
    (1024, 1024, 1024, 72, 64, torch.float64),
    (256, 4096, 4096, 72, 64, torch.float32),
    (2048, 2048, 256, 40, 32, torch.float64),
]
# the product alone at the two tall shapes of 7g's table that name a share of the copy bandwidth: (count, m, n, l, dtype, 7g's share)
SKETCH_ID_SHAPES = [(2048, 2048, 256, 40, torch.float64, 0.10), (512, 8192, 128, 24, torch.float64, 0.29)]


def spread(prefix, t):
    med, lo, hi = t
    return {prefix + "_s": med, prefix + "_s_min": lo, prefix + "_s_max": hi, prefix + "_spread": (hi - lo) / med}


def eye(l, count, dtype):
    return torch.eye(l, dtype=dtype, device="cuda").expand(count, l, l)


def matmul_step(a, omega):
    """The large range step with both products by torch.matmul."""
    count, l = a.shape[0], omega.shape[-2]
    y = torch.matmul(omega, a)
    u, _, _, ranks = rc.lowrank_recompress_tall_batched(y.mT, eye(l, count, a.dtype), l, 0.0)
    q = u.mT
    return q, torch.matmul(a, u), ranks


def matmul_chain(a, omega, k, steps):
    for step in range(steps):
        q, p, ranks = matmul_step(a, omega)
        if step + 1 < steps:
            l = p.shape[2]
            omega = rc.lowrank_recompress_tall_batched(p, eye(l, a.shape[0], a.dtype), l, 0.0, ranks=ranks)[0].mT
    return rc.lowrank_recompress_large_batched(p, q, k, 0.0, ranks=ranks)


def product_row(a, omega, repeats):
    count, m, n = a.shape
    fn = lambda: rc.sketch_product_batched(a, omega)  # noqa: E731
    ref = lambda: torch.matmul(omega, a)  # noqa: E731
    y, yr = fn(), ref()  # warm-up
    torch.cuda.synchronize()
    scale = float((omega.abs().double() @ a[0].abs().double()).max())
    agree = float((y - yr).abs().max()) / scale
    t, tm = timed(fn, repeats), timed(ref, repeats)
    return dict(**spread("product", t), **spread("matmul", tm), product_blocks_per_s=count / t[0],
                product_share_of_copy_bw=count * m * n * a.element_size() / t[0] / COPY_BW, matmul_over_product=tm[0] / t[0],
                max_abs_diff_over_abs_product=agree)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--shapes", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs an MI355X")
    out_path = args.out or os.path.join(ROOT, "profiles", "batched_sketch_svd_large_bench.json")
    results = []
    for si in [int(x) for x in (args.shapes or ",".join(str(i) for i in range(len(SHAPES)))).split(",")]:
        count, m, n, l, k, dtype = SHAPES[si]
        g = torch.Generator(device="cuda").manual_seed(97530 + si)
        a = torch.randn(count, m, n, generator=g, device="cuda", dtype=dtype)
        omega = torch.randn(l, m, generator=g, device="cuda", dtype=dtype)
        row = dict(kind="chain", count=count, m=m, n=n, l=l, k=k, dtype=str(dtype).replace("torch.", ""), delegating=n <= 512)
        row.update(product_row(a, omega, args.repeats))
        for steps in (1, 2):
            new = lambda: rc.sketch_svd_rank_large_batched(a, k, 0.0, steps, omega=omega)  # noqa: E731
            old = (lambda: rc.sketch_svd_rank_power_batched(a, k, 0.0, steps, omega=omega)) if n <= 512 else (lambda: matmul_chain(a, omega, k, steps))  # noqa: E731
            s_new, s_old = new()[1], old()[1]  # warm-up; the singular values of the two routes
            torch.cuda.synchronize()
            t_new, t_old = timed(new, args.repeats), timed(old, args.repeats)
            row.update(**spread(f"chain{steps}", t_new), **spread(f"matmul_chain{steps}", t_old))
            row[f"chain{steps}_blocks_per_s"] = count / t_new[0]
            row[f"matmul_chain{steps}_over_chain{steps}"] = t_old[0] / t_new[0]
            row[f"chain{steps}_max_rel_s_diff"] = float(((s_new - s_old).abs().max(dim=1).values / s_old[:, 0]).max())
        print(json.dumps(row), flush=True)
        results.append(row)
        del a
        torch.cuda.empty_cache()
    for count, m, n, l, dtype, share in SKETCH_ID_SHAPES:
        g = torch.Generator(device="cuda").manual_seed(13579 + m)
        a = torch.randn(count, m, n, generator=g, device="cuda", dtype=dtype)
        omega = torch.randn(l, m, generator=g, device="cuda", dtype=dtype)
        row = dict(kind="product_beside_7g", count=count, m=m, n=n, l=l, dtype=str(dtype).replace("torch.", ""), sketched_id_share_7g=share)
        row.update(product_row(a, omega, args.repeats))
        row["share_over_7g"] = row["product_share_of_copy_bw"] / share
        print(json.dumps(row), flush=True)
        results.append(row)
        del a
        torch.cuda.empty_cache()
    with open(out_path, "w") as f:
        json.dump(dict(device=torch.cuda.get_device_name(0), repeats=args.repeats, copy_bandwidth_bytes_per_s=COPY_BW, results=results), f, indent=1)
        f.write("\n")
    print("wrote", out_path)


if __name__ == "__main__":
    main()
