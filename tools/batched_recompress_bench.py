#!/usr/bin/env python3
"""Throughput of the batched recompression (rc_lowrank_recompress_batched_*) against the only other route through the library:
rc_lowrank_apply_batched_* rebuilding every block (to_mat) followed by rc_svd_rank_batched_* of the blocks.

Each block is a rounded addition: left = [U1 U2] (m x K), right = [V1^T; V2^T] (K x n) with Gaussian columns of unit expected norm and
s = two copies of logspace(0, -6, K / 2), recompressed to rank k.  One batched call, timed with device events after warm-up (median
of --repeats).  The baseline runs where rc_svd_rank_batched_* accepts the block (min(m, n) <= 128); elsewhere the row records that
it cannot.  The plan label of the launch is read from the event profile.
Writes profiles/batched_recompress_bench.json unless --out names another file.  Not used by the tests or by bench.py.

--complex: the same measurement for complex factors (rc_lowrank_recompress_complex_batched_c64 / _c32; complex Gaussian columns, the
same real s) on the complex shapes below, beside (a) the only other route, the complex to_mat + rc_svd_rank_batched_c*, where it
accepts the block, and (b) the real recompression of real factors of the same shape and precision; the ratios to both are recorded.
Writes profiles/batched_recompress_complex_bench.json.

    python tools/batched_recompress_bench.py [--complex] [--repeats 5] [--shapes 0,1,2,3] [--out path.json]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import rusty_compression_amd as rc  # noqa: E402
from tests.helpers import batched_launch  # noqa: E402
from tools.batched_id_bench import timed  # noqa: E402

SHAPES = [  # (count, m, n, K, k, dtype)
    (16384, 128, 128, 64, 32, torch.float64),
    (4096, 512, 128, 64, 32, torch.float64),
    (8192, 256, 256, 64, 32, torch.float32),
    (2048, 512, 512, 128, 64, torch.float64),
]
COMPLEX_SHAPES = [  # the last count keeps one run of the all-workspace plan under a few seconds
    (16384, 128, 128, 64, 32, torch.complex128),
    (4096, 512, 128, 64, 32, torch.complex128),
    (8192, 256, 256, 64, 32, torch.complex64),
    (1024, 512, 512, 128, 64, torch.complex128),
]


def complex_main(args):
    out_path = args.out or os.path.join(ROOT, "profiles", "batched_recompress_complex_bench.json")
    results = []
    for si in [int(x) for x in (args.shapes or ",".join(str(i) for i in range(len(COMPLEX_SHAPES)))).split(",")]:
        count, m, n, kin, k, dtype = COMPLEX_SHAPES[si]
        real = torch.float64 if dtype == torch.complex128 else torch.float32
        g = torch.Generator(device="cuda").manual_seed(2468 + si)

        def gauss(rows, cols, scale):  # real and imaginary parts of variance 1 / (2 scale): columns of unit expected norm
            return torch.randn(count, rows, cols, generator=g, device="cuda", dtype=torch.float64) / (2 * scale) ** 0.5

        left = torch.complex(gauss(m, kin, m), gauss(m, kin, m)).to(dtype)
        right = torch.complex(gauss(kin, n, n), gauss(kin, n, n)).to(dtype)
        s = torch.logspace(0, -6, kin // 2, device="cuda", dtype=torch.float64).repeat(2).to(real).expand(count, kin).contiguous()
        fn = lambda: rc.lowrank_recompress_batched_complex(left, right, k, 0.0, s=s)  # noqa: E731
        (u, sv, vt, ranks), label = batched_launch(fn)  # warm-up (code objects, workspace) and the plan
        torch.cuda.synchronize()
        t_med, t_min, t_max = timed(fn, args.repeats)
        row = dict(count=count, m=m, n=n, K=kin, k=k, dtype=str(dtype).replace("torch.", ""), plan=label["plan"], grid=label["grid"],
                   slots=label["slots"], recompress_s=t_med, recompress_s_min=t_min, recompress_s_max=t_max, blocks_per_s=count / t_med)
        if min(m, n) <= 128:
            def baseline():
                return rc.svd_rank_batched_complex(rc.lowrank_apply_batched(left, right, s=s), k, 0.0)

            bu, bs, bvt, _ = baseline()
            torch.cuda.synchronize()
            b_med, b_min, b_max = timed(baseline, args.repeats)
            row.update(baseline="to_mat + svd_rank_batched_complex", baseline_s=b_med, baseline_s_min=b_min, baseline_s_max=b_max,
                       baseline_blocks_per_s=count / b_med, speedup_vs_baseline=b_med / t_med,
                       max_abs_sval_diff_vs_baseline=float((sv[:, :k] - bs[:, :k]).abs().max()), max_sval=float(bs[:, 0].max()))
            del bu, bs, bvt
        else:
            row.update(baseline="impossible: rc_svd_rank_batched_c* rejects min(m, n) > 128")
        del u, sv, vt, ranks
        # (b) the real recompression of real factors of the same shape and precision
        rl, rr = left.real.contiguous(), right.real.contiguous()
        del left, right
        torch.cuda.empty_cache()
        rfn = lambda: rc.lowrank_recompress_batched(rl, rr, k, 0.0, s=s)  # noqa: E731
        _, rlabel = batched_launch(rfn)
        torch.cuda.synchronize()
        r_med, r_min, r_max = timed(rfn, args.repeats)
        row.update(real_twin_plan=rlabel["plan"], real_twin_s=r_med, real_twin_s_min=r_min, real_twin_s_max=r_max,
                   real_twin_blocks_per_s=count / r_med, time_vs_real_twin=t_med / r_med)
        results.append(row)
        print(json.dumps(row), flush=True)
        del rl, rr, s
        torch.cuda.empty_cache()
    out = dict(tool="tools/batched_recompress_bench.py --complex", device=torch.cuda.get_device_name(0), results=results)
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", out_path)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--complex", action="store_true", help="measure the complex recompression (c64, c32) instead of the real one")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--shapes", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs an MI355X")
    if args.complex:
        return complex_main(args)
    out_path = args.out or os.path.join(ROOT, "profiles", "batched_recompress_bench.json")
    results = []
    for si in [int(x) for x in (args.shapes or ",".join(str(i) for i in range(len(SHAPES)))).split(",")]:
        count, m, n, kin, k, dtype = SHAPES[si]
        g = torch.Generator(device="cuda").manual_seed(1357 + si)
        left = (torch.randn(count, m, kin, generator=g, device="cuda", dtype=torch.float64) / m ** 0.5).to(dtype)
        right = (torch.randn(count, kin, n, generator=g, device="cuda", dtype=torch.float64) / n ** 0.5).to(dtype)
        s = torch.logspace(0, -6, kin // 2, device="cuda", dtype=torch.float64).repeat(2).to(dtype).expand(count, kin).contiguous()
        fn = lambda: rc.lowrank_recompress_batched(left, right, k, 0.0, s=s)  # noqa: E731
        (u, sv, vt, ranks), label = batched_launch(fn)  # warm-up (code objects, workspace) and the plan
        torch.cuda.synchronize()
        t_med, t_min, t_max = timed(fn, args.repeats)
        row = dict(count=count, m=m, n=n, K=kin, k=k, dtype=str(dtype).replace("torch.", ""), plan=label["plan"], grid=label["grid"],
                   slots=label["slots"], recompress_s=t_med, recompress_s_min=t_min, recompress_s_max=t_max, blocks_per_s=count / t_med,
                   flop_model_gain=m * n * min(m, n) / ((m + n) * kin ** 2))
        if min(m, n) <= 128:
            def baseline():
                return rc.svd_rank_batched(rc.lowrank_apply_batched(left, right, s=s), k, 0.0)

            bu, bs, bvt, _ = baseline()
            torch.cuda.synchronize()
            b_med, b_min, b_max = timed(baseline, args.repeats)
            scale = float(bs[:, 0].max())
            row.update(baseline="to_mat + svd_rank_batched", baseline_s=b_med, baseline_s_min=b_min, baseline_s_max=b_max,
                       baseline_blocks_per_s=count / b_med, speedup_vs_baseline=b_med / t_med,
                       max_abs_sval_diff_vs_baseline=float((sv[:, :k] - bs[:, :k]).abs().max()), max_sval=scale)
            del bu, bs, bvt
        else:
            row.update(baseline="impossible: rc_svd_rank_batched_* rejects min(m, n) > 128")
        results.append(row)
        print(json.dumps(row), flush=True)
        del left, right, s, u, sv, vt, ranks
        torch.cuda.empty_cache()
    out = dict(tool="tools/batched_recompress_bench.py", device=torch.cuda.get_device_name(0), results=results)
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", out_path)


if __name__ == "__main__":
    main()
