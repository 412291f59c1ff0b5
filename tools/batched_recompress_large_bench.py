#!/usr/bin/env python3
"""Throughput of the batched recompression with both factors tall (rc_lowrank_recompress_large_batched_*) beside what a caller had before it.

Each block is a rounded addition: left = [U1 U2] (m x K), right = [V1^T; V2^T] (K x n) with Gaussian columns of unit expected norm and
s = two copies of logspace(0, -6, K / 2), recompressed to rank k.  One batched call, timed with device events after warm-up (median of
--repeats, with the smallest and largest time as the spread).  The stages of both sides and the plan of the launch are read from the event
profile.  Per both-tall shape (n > 512):

  in-library composition   rc_lowrank_recompress_tall_batched_* with right = I on left and on right^T, the K x K core by torch.bmm,
                           rc_svd_rank_batched_* on the core, two torch.bmm to bring both bases back: three launches of the library's
                           (three Jacobi SVDs) and three products, two m x K / n x K bases written and re-read
  qr composition           torch.linalg.qr (reduced, batched) on left and on right^T, the core, rc_svd_rank_batched_*, two torch.bmm;
                           dropped (and recorded as dropped) at a shape where its first call takes more than a minute
  tall calls               rc_lowrank_recompress_tall_batched_* at m x 256 and at n x 256 with the same K: the new call factors one tall
                           side of each, so its time per block is expected near their sum minus one Jacobi; the ratio is recorded

At n <= 512 the same arguments also go through rc_lowrank_recompress_tall_batched_*: the same work per block, so the ratio of the two times
is recorded, with a check that the bits agree.  Writes profiles/batched_recompress_large_bench.json unless --out names another file.  Not used
by the tests or by bench.py.

--complex measures rc_lowrank_recompress_complex_large_batched_c64 / _c32 at the same shapes with complex factors (c64 where the real rows
are f64, c32 where f32) and writes profiles/batched_recompress_large_complex_bench.json.  Per both-tall shape: the in-library composition in
its complex form (two rc_lowrank_recompress_tall_complex_batched_* calls with right = I, rc_svd_rank_batched_c64 / _c32 on the core, three
torch.bmm) and the real large call on the real parts of the same factors, in the same process, with the ratio of the two times.  At n <= 512:
the ratio to rc_lowrank_recompress_tall_complex_batched_*, with the check of the bits.

    python tools/batched_recompress_large_bench.py [--complex] [--repeats 5] [--shapes 0,1,2,3] [--out path.json]
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import rusty_compression_amd as rc  # noqa: E402
from tests.helpers import batched_launch  # noqa: E402
from tools.batched_id_bench import timed  # noqa: E402

SHAPES = [  # (count, m, n, K, k, dtype)
    (512, 2048, 2048, 32, 16, torch.float64),
    (1024, 1024, 1024, 64, 32, torch.float64),
    (256, 4096, 4096, 64, 32, torch.float32),
    (2048, 2048, 256, 32, 16, torch.float64),
]
QR_LIMIT_S = 60.0
COMPLEX_OF = {torch.float64: torch.complex128, torch.float32: torch.complex64}


def spread(prefix, t):
    med, lo, hi = t
    return {prefix + "_s": med, prefix + "_s_min": lo, prefix + "_s_max": hi}


def main_complex(args):
    """The rows of --complex (see the module docstring)."""
    out_path = args.out or os.path.join(ROOT, "profiles", "batched_recompress_large_complex_bench.json")
    results = []
    for si in [int(x) for x in (args.shapes or ",".join(str(i) for i in range(len(SHAPES)))).split(",")]:
        count, m, n, kin, k, rdtype = SHAPES[si]
        dtype = COMPLEX_OF[rdtype]
        g = torch.Generator(device="cuda").manual_seed(86420 + si)
        left = (torch.randn(count, m, kin, generator=g, device="cuda", dtype=torch.complex128) / m ** 0.5).to(dtype)
        right = (torch.randn(count, kin, n, generator=g, device="cuda", dtype=torch.complex128) / n ** 0.5).to(dtype)
        s = torch.logspace(0, -6, kin // 2, device="cuda", dtype=torch.float64).repeat(2).to(rdtype).expand(count, kin).contiguous()
        fn = lambda: rc.lowrank_recompress_large_batched_complex(left, right, k, 0.0, s=s)  # noqa: E731
        (u, sv, vt, ranks), label = batched_launch(fn)  # warm-up (code objects, workspace) and the plan
        torch.cuda.synchronize()
        t_large = timed(fn, args.repeats)
        plan = label["plan"].split(",")
        row = dict(count=count, m=m, n=n, K=kin, k=k, dtype=str(dtype).replace("torch.", ""), stages=int(plan[0].split("=")[1]),
                   rstages=int(plan[1].split("=")[1]), plan=",".join(plan[2:]), grid=label["grid"], slots=label["slots"],
                   **spread("recompress_large", t_large), blocks_per_s=count / t_large[0])
        print(json.dumps(row), flush=True)

        # the real large call on the real parts of the same factors, from the same process
        rl, rr = left.real.contiguous(), right.real.contiguous()
        rfn = lambda: rc.lowrank_recompress_large_batched(rl, rr, k, 0.0, s=s)  # noqa: E731
        rfn()
        torch.cuda.synchronize()
        t_real = timed(rfn, args.repeats)
        row.update(**spread("real_large_call", t_real), real_large_call_blocks_per_s=count / t_real[0], time_vs_real_large_call=t_large[0] / t_real[0])
        del rl, rr

        if n > 512:
            eye = torch.eye(kin, device="cuda", dtype=dtype).expand(count, kin, kin)
            right_t = right.mT  # n x K as a strided view, the plain transpose: no copy, nothing conjugated

            def in_library():
                ul, sl, vl, _ = rc.lowrank_recompress_tall_batched_complex(left, eye, kin)       # left = ul diag(sl) vl
                ur, sr, vr, _ = rc.lowrank_recompress_tall_batched_complex(right_t, eye, kin)    # right = vr^T diag(sr) ur^T
                core = torch.bmm(sl[:, :, None] * vl * s[:, None, :], vr.mT * sr[:, None, :])
                cu, cs, cvt, cr = rc.svd_rank_batched_complex(core, k)
                return torch.bmm(ul, cu), cs, torch.bmm(cvt, ur.mT), cr

            _, cs, _, _ = in_library()
            torch.cuda.synchronize()
            t_lib = timed(in_library, args.repeats)
            row.update(in_library_composition="2 x lowrank_recompress_tall_batched_complex (right = I) + svd_rank_batched_complex + 3 x torch.bmm",
                       **spread("in_library", t_lib), in_library_blocks_per_s=count / t_lib[0], speedup_vs_in_library=t_lib[0] / t_large[0],
                       faster_than_in_library_beyond_spread=bool(t_lib[0] - t_large[0] > (t_lib[2] - t_lib[1]) + (t_large[2] - t_large[1])),
                       max_abs_sval_diff_vs_in_library=float((sv[:, :k] - cs[:, :k]).abs().max()), max_sval=float(cs[:, 0].max()))
            del cs, eye
        else:
            pfn = lambda: rc.lowrank_recompress_tall_batched_complex(left, right, k, 0.0, s=s)  # noqa: E731
            (pu, ps, pvt, pr), plabel = batched_launch(pfn)
            torch.cuda.synchronize()
            t_tall = timed(pfn, args.repeats)
            t_again = timed(fn, args.repeats)  # the large call again, after the tall one: the same cache state on both sides
            same = all(torch.equal(a, b) for a, b in zip((u, sv, vt, ranks), (pu, ps, pvt, pr)))
            row.update(tall_call_plan=plabel["plan"], **spread("tall_call", t_tall), **spread("recompress_large_again", t_again),
                       rate_vs_tall_call=t_tall[0] / t_again[0], same_bits_as_tall_call=bool(same))
            if not same:
                raise SystemExit("the bits differ from rc_lowrank_recompress_tall_complex_batched_*'s at n <= 512")
            del pu, ps, pvt, pr
        results.append(row)
        print(json.dumps(row), flush=True)
        del left, right, s, u, sv, vt, ranks
        torch.cuda.empty_cache()
    out = dict(tool="tools/batched_recompress_large_bench.py --complex", device=torch.cuda.get_device_name(0), repeats=args.repeats, results=results)
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", out_path)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--complex", action="store_true", help="the complex twin, rc_lowrank_recompress_complex_large_batched_*")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--shapes", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs an MI355X")
    if args.complex:
        return main_complex(args)
    out_path = args.out or os.path.join(ROOT, "profiles", "batched_recompress_large_bench.json")
    results = []
    for si in [int(x) for x in (args.shapes or ",".join(str(i) for i in range(len(SHAPES)))).split(",")]:
        count, m, n, kin, k, dtype = SHAPES[si]
        g = torch.Generator(device="cuda").manual_seed(86420 + si)
        left = (torch.randn(count, m, kin, generator=g, device="cuda", dtype=torch.float64) / m ** 0.5).to(dtype)
        right = (torch.randn(count, kin, n, generator=g, device="cuda", dtype=torch.float64) / n ** 0.5).to(dtype)
        s = torch.logspace(0, -6, kin // 2, device="cuda", dtype=torch.float64).repeat(2).to(dtype).expand(count, kin).contiguous()
        fn = lambda: rc.lowrank_recompress_large_batched(left, right, k, 0.0, s=s)  # noqa: E731
        (u, sv, vt, ranks), label = batched_launch(fn)  # warm-up (code objects, workspace) and the plan
        torch.cuda.synchronize()
        t_large = timed(fn, args.repeats)
        plan = label["plan"].split(",")
        row = dict(count=count, m=m, n=n, K=kin, k=k, dtype=str(dtype).replace("torch.", ""), stages=int(plan[0].split("=")[1]),
                   rstages=int(plan[1].split("=")[1]), plan=",".join(plan[2:]), grid=label["grid"], slots=label["slots"],
                   **spread("recompress_large", t_large), blocks_per_s=count / t_large[0])
        print(json.dumps(row), flush=True)

        if n > 512:
            eye = torch.eye(kin, device="cuda", dtype=dtype).expand(count, kin, kin)
            right_t = right.mT  # n x K as a strided view: no copy

            def in_library():
                ul, sl, vl, _ = rc.lowrank_recompress_tall_batched(left, eye, kin)       # left = ul diag(sl) vl
                ur, sr, vr, _ = rc.lowrank_recompress_tall_batched(right_t, eye, kin)    # right = vr^T diag(sr) ur^T
                core = torch.bmm(sl[:, :, None] * vl * s[:, None, :], vr.mT * sr[:, None, :])
                cu, cs, cvt, cr = rc.svd_rank_batched(core, k)
                return torch.bmm(ul, cu), cs, torch.bmm(cvt, ur.mT), cr

            _, cs, _, _ = in_library()
            torch.cuda.synchronize()
            t_lib = timed(in_library, args.repeats)
            row.update(in_library_composition="2 x lowrank_recompress_tall_batched (right = I) + svd_rank_batched + 3 x torch.bmm",
                       **spread("in_library", t_lib), in_library_blocks_per_s=count / t_lib[0], speedup_vs_in_library=t_lib[0] / t_large[0],
                       faster_than_in_library_beyond_spread=bool(t_large[2] < t_lib[1]),
                       max_abs_sval_diff_vs_in_library=float((sv[:, :k] - cs[:, :k]).abs().max()), max_sval=float(cs[:, 0].max()))
            print(json.dumps({"in_library_s": t_lib[0]}), flush=True)

            def qr_composition():
                ql, rl = torch.linalg.qr(left)
                qr, rr = torch.linalg.qr(right_t)
                core = torch.bmm(rl * s[:, None, :], rr.mT)
                cu, cs, cvt, cr = rc.svd_rank_batched(core, k)
                return torch.bmm(ql, cu), cs, torch.bmm(cvt, qr.mT), cr

            t0 = time.perf_counter()
            _, cs, _, _ = qr_composition()
            torch.cuda.synchronize()
            first = time.perf_counter() - t0
            row.update(qr_composition="2 x torch.linalg.qr + svd_rank_batched + 3 x torch.bmm", qr_composition_first_call_s=first)
            if first > QR_LIMIT_S:
                row.update(qr_composition_dropped=True)
            else:
                t_qr = timed(qr_composition, args.repeats)
                row.update(qr_composition_dropped=False, **spread("qr_composition", t_qr), qr_composition_blocks_per_s=count / t_qr[0],
                           speedup_vs_qr_composition=t_qr[0] / t_large[0], max_abs_sval_diff_vs_qr_composition=float((sv[:, :k] - cs[:, :k]).abs().max()))
            del cs

            # the tall call on each tall side beside a 256-column factor of the same inner width
            thin = (torch.randn(count, kin, 256, generator=g, device="cuda", dtype=torch.float64) / 16.0).to(dtype)
            fm = lambda: rc.lowrank_recompress_tall_batched(left, thin, k, 0.0, s=s)  # noqa: E731
            fnn = lambda: rc.lowrank_recompress_tall_batched(right_t, thin, k, 0.0, s=s)  # noqa: E731
            fm(), fnn()
            torch.cuda.synchronize()
            t_m, t_n = timed(fm, args.repeats), timed(fnn, args.repeats)
            row.update(**spread("tall_m_x_256", t_m), **spread("tall_n_x_256", t_n), time_vs_sum_of_tall_calls=t_large[0] / (t_m[0] + t_n[0]))
            del thin, eye
        else:
            pfn = lambda: rc.lowrank_recompress_tall_batched(left, right, k, 0.0, s=s)  # noqa: E731
            (pu, ps, pvt, pr), plabel = batched_launch(pfn)
            torch.cuda.synchronize()
            t_tall = timed(pfn, args.repeats)
            t_again = timed(fn, args.repeats)  # the large call again, after the tall one: the same cache state on both sides
            same = all(torch.equal(a, b) for a, b in zip((u, sv, vt, ranks), (pu, ps, pvt, pr)))
            row.update(tall_call_plan=plabel["plan"], **spread("tall_call", t_tall), **spread("recompress_large_again", t_again),
                       rate_vs_tall_call=t_tall[0] / t_again[0], same_bits_as_tall_call=bool(same))
            if not same:
                raise SystemExit("the bits differ from rc_lowrank_recompress_tall_batched_*'s at n <= 512")
            del pu, ps, pvt, pr
        results.append(row)
        print(json.dumps(row), flush=True)
        del left, right, s, u, sv, vt, ranks
        torch.cuda.empty_cache()
    out = dict(tool="tools/batched_recompress_large_bench.py", device=torch.cuda.get_device_name(0), repeats=args.repeats, results=results)
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", out_path)


if __name__ == "__main__":
    main()
