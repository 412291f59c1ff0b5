#!/usr/bin/env python3
"""Throughput of the tall batched recompression (rc_lowrank_recompress_tall_batched_*) beside the composition a caller had before it:
torch.linalg.qr(left) (reduced, batched), rc_lowrank_recompress_batched_* on (R, right), and torch.bmm(Q, u) to bring the left vectors
back to m rows.

Each block is a rounded addition: left = [U1 U2] (m x K), right = [V1^T; V2^T] (K x n) with Gaussian columns of unit expected norm and
s = two copies of logspace(0, -6, K / 2), recompressed to rank k.  One batched call, timed with device events after warm-up (median
of --repeats).  The stages and the plan of the launch are read from the event profile.  At m <= 512 the same arguments also go through
rc_lowrank_recompress_batched_*: the same work per block, so the ratio of the two times is recorded, with a check that the bits agree.
Writes profiles/batched_recompress_tall_bench.json unless --out names another file.  Not used by the tests or by bench.py.

--complex measures rc_lowrank_recompress_tall_complex_batched_* at the same shapes in c64 / c32 (complex Gaussian factors, the same real s)
against the complex composition (torch.linalg.qr on complex left, rc_lowrank_recompress_complex_batched_*, torch.bmm), against the real tall
call at the same shape and precision (the real parts of the same factors), and at m <= 512 against the existing complex call on the same
arguments; it writes profiles/batched_recompress_tall_complex_bench.json.

    python tools/batched_recompress_tall_bench.py [--complex] [--repeats 5] [--shapes 0,1,2,3] [--out path.json]
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
    (2048, 2048, 256, 32, 16, torch.float64),
    (8192, 512, 256, 32, 16, torch.float64),
    (2048, 1024, 512, 64, 32, torch.float32),
    (512, 8192, 128, 16, 8, torch.float64),
]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--shapes", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--complex", action="store_true", dest="complex_data")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs an MI355X")
    cx = args.complex_data
    out_path = args.out or os.path.join(ROOT, "profiles", "batched_recompress_tall_complex_bench.json" if cx else "batched_recompress_tall_bench.json")
    tall = rc.lowrank_recompress_tall_batched_complex if cx else rc.lowrank_recompress_tall_batched
    existing = rc.lowrank_recompress_batched_complex if cx else rc.lowrank_recompress_batched
    results = []
    for si in [int(x) for x in (args.shapes or ",".join(str(i) for i in range(len(SHAPES)))).split(",")]:
        count, m, n, kin, k, dtype = SHAPES[si]
        g = torch.Generator(device="cuda").manual_seed(97531 + si)
        real_dtype = dtype
        if cx:  # complex Gaussian columns of unit expected norm; s stays real
            dtype = torch.complex128 if dtype == torch.float64 else torch.complex64
        gen = torch.complex128 if cx else torch.float64
        left = (torch.randn(count, m, kin, generator=g, device="cuda", dtype=gen) / m ** 0.5).to(dtype)
        right = (torch.randn(count, kin, n, generator=g, device="cuda", dtype=gen) / n ** 0.5).to(dtype)
        s = torch.logspace(0, -6, kin // 2, device="cuda", dtype=torch.float64).repeat(2).to(real_dtype).expand(count, kin).contiguous()
        fn = lambda: tall(left, right, k, 0.0, s=s)  # noqa: E731
        (u, sv, vt, ranks), label = batched_launch(fn)  # warm-up (code objects, workspace) and the plan
        torch.cuda.synchronize()
        t_med, t_min, t_max = timed(fn, args.repeats)
        plan = label["plan"].split(",")
        row = dict(count=count, m=m, n=n, K=kin, k=k, dtype=str(dtype).replace("torch.", ""), stages=int(plan[0].split("=")[1]), plan=",".join(plan[1:]),
                   grid=label["grid"], slots=label["slots"], recompress_tall_s=t_med, recompress_tall_s_min=t_min, recompress_tall_s_max=t_max,
                   blocks_per_s=count / t_med)

        def composition():
            q, r = torch.linalg.qr(left)
            cu, cs, cvt, cr = existing(r, right, k, 0.0, s=s)
            return torch.bmm(q, cu), cs, cvt, cr

        cu, cs, cvt, _ = composition()
        torch.cuda.synchronize()
        c_med, c_min, c_max = timed(composition, args.repeats)
        row.update(composition="torch.linalg.qr + lowrank_recompress_batched%s + torch.bmm" % ("_complex" if cx else ""), composition_s=c_med, composition_s_min=c_min, composition_s_max=c_max,
                   composition_blocks_per_s=count / c_med, speedup_vs_composition=c_med / t_med,
                   max_abs_sval_diff_vs_composition=float((sv[:, :k] - cs[:, :k]).abs().max()), max_sval=float(cs[:, 0].max()))
        del cu, cs, cvt
        if cx:  # the real tall call at the same shape and precision
            rl, rr = left.real.contiguous(), right.real.contiguous()
            rfn = lambda: rc.lowrank_recompress_tall_batched(rl, rr, k, 0.0, s=s)  # noqa: E731
            rfn()
            torch.cuda.synchronize()
            r_med, r_min, r_max = timed(rfn, args.repeats)
            row.update(real_tall_s=r_med, real_tall_s_min=r_min, real_tall_s_max=r_max, time_vs_real_tall=t_med / r_med)
            del rl, rr
        if m <= 512:
            pfn = lambda: existing(left, right, k, 0.0, s=s)  # noqa: E731
            (pu, ps, pvt, pr), plabel = batched_launch(pfn)
            torch.cuda.synchronize()
            p_med, p_min, p_max = timed(pfn, args.repeats)
            t2_med, t2_min, t2_max = timed(fn, args.repeats)  # the tall call again, after the existing one: the same cache state on both sides
            same = all(torch.equal(a, b) for a, b in zip((u, sv, vt, ranks), (pu, ps, pvt, pr)))
            row.update(existing_call_plan=plabel["plan"], existing_call_s=p_med, existing_call_s_min=p_min, existing_call_s_max=p_max,
                       recompress_tall_again_s=t2_med, recompress_tall_again_s_min=t2_min, recompress_tall_again_s_max=t2_max,
                       rate_vs_existing_call=p_med / t2_med, same_bits_as_existing_call=bool(same))
            del pu, ps, pvt, pr
        results.append(row)
        print(json.dumps(row), flush=True)
        del left, right, s, u, sv, vt, ranks
        torch.cuda.empty_cache()
    out = dict(tool="tools/batched_recompress_tall_bench.py" + (" --complex" if cx else ""), device=torch.cuda.get_device_name(0), results=results)
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", out_path)


if __name__ == "__main__":
    main()
