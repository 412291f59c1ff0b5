#!/usr/bin/env python3
"""Throughput of the batched sketched column ID (rc_sketch_column_id_rank_batched_*) on tall blocks with one shared Gaussian omega,
beside the three routes a caller had without it:

  (a) rc_column_id_rank_batched_* on the blocks themselves, where it accepts them (m <= 512);
  (b) the composition a torch caller has: torch.matmul(omega, a), rc_column_id_rank_batched_* on the sketches, an index gather of C;
  (c) a loop of lone rc_column_id_rank_* calls on 64 of the blocks.

Blocks have a decaying spectrum (tools/batched_id_bench.decaying_batch).  Every route is timed with device events after a warm-up,
median of --repeats with the spread.  Reported per shape: blocks/s, the bytes of A per second as a share of the 6.29 TB/s copy
bandwidth, the sketch's 2 l m n flop per block per second as a share of the MFMA peak (78.6 TFLOP/s f64, 157.3 TFLOP/s f32), and
the plan label of the launch.  On the first shape the error ||A - C Z||_F / ||A||_F of the new call is checked against route (b)'s on
the first blocks (err <= 1.5 err_b + 100 eps).  Writes profiles/batched_sketch_id_bench.json unless --out names another file.  Not used
by the tests or by bench.py.

--complex runs the same shapes with complex scalars (c64 / c64 / c32 / c64 in place of f64 / f64 / f32 / f64) through
rc_sketch_column_id_rank_complex_batched_*: complex blocks of the same decaying spectrum, a complex Gaussian omega, routes (a) to (c) with
the complex calls, and (d) the real sketched call on the real parts at the same shape, timed in the same run (complex_over_real_time;
twice the bytes and four times the MFMAs, 8 l m n real flop per block).  Writes profiles/batched_sketch_id_complex_bench.json and
leaves the real output file alone.

    python tools/batched_sketch_id_bench.py [--complex] [--repeats 5] [--shapes 0,1,2,3] [--out path.json]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import rusty_compression_amd as rc  # noqa: E402
from rusty_compression_amd.batch import column_id_rank  # noqa: E402
from rusty_compression_amd.random_matrix import Rng  # noqa: E402
from tests.helpers import batched_launch  # noqa: E402
from tools.batched_id_bench import decaying_batch, timed  # noqa: E402

SHAPES = [  # (count, m, n, l, k, dtype)
    (2048, 2048, 256, 40, 32, torch.float64),
    (8192, 512, 256, 40, 32, torch.float64),
    (2048, 1024, 512, 72, 64, torch.float32),
    (512, 8192, 128, 24, 16, torch.float64),
]
COPY_BW = 6.29e12
MFMA_PEAK = {torch.float64: 78.6e12, torch.float32: 157.3e12, torch.complex128: 78.6e12, torch.complex64: 157.3e12}
COMPLEX_OF = {torch.float64: torch.complex128, torch.float32: torch.complex64}
LOOP_BLOCKS = 64


def rel_err(a, c, z):
    wide = torch.complex128 if a.dtype.is_complex else torch.float64
    a64 = a.to(wide)
    return [float(torch.linalg.norm(a64[i] - c[i].to(wide) @ z[i].to(wide)) / torch.linalg.norm(a64[i])) for i in range(a.shape[0])]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--shapes", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--complex", action="store_true", help="time rc_sketch_column_id_rank_complex_batched_c64 / _c32 on complex blocks of the same shapes")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs an MI355X")
    out_path = args.out or os.path.join(ROOT, "profiles", "batched_sketch_id_complex_bench.json" if args.complex else "batched_sketch_id_bench.json")
    sketch_call = rc.sketch_column_id_rank_batched_complex if args.complex else rc.sketch_column_id_rank_batched
    results = []
    for si in [int(x) for x in (args.shapes or ",".join(str(i) for i in range(len(SHAPES)))).split(",")]:
        count, m, n, l, k, dtype = SHAPES[si]
        real_dtype = dtype
        if args.complex:
            dtype = COMPLEX_OF[dtype]
        a = decaying_batch(count, m, n, dtype, 2468 + si)
        omega = rc.random_gaussian((l, m), Rng(si), dtype)
        elem = a.element_size()

        def new():
            return sketch_call(a, k, 0.0, omega=omega)

        def composed():
            y = torch.matmul(omega, a)
            _, z, ind, ranks = rc.column_id_rank_batched(y, k, 0.0)
            c = torch.gather(a, 2, ind[:, None, :k].expand(count, m, k))
            return c, z, ind, ranks

        def loop():
            return [column_id_rank(a[i], k) for i in range(LOOP_BLOCKS)]

        (c, z, ind, ranks), label = batched_launch(new)  # warm-up (code objects, workspace) and the plan
        torch.cuda.synchronize()
        t_med, t_min, t_max = timed(new, args.repeats)
        row = dict(count=count, m=m, n=n, l=l, k=k, dtype=str(dtype).replace("torch.", ""), plan=label["plan"], grid=label["grid"], slots=label["slots"],
                   sketch_id_s=t_med, sketch_id_s_min=t_min, sketch_id_s_max=t_max, blocks_per_s=count / t_med,
                   a_bytes_per_s_share_of_copy_bw=count * m * n * elem / t_med / COPY_BW,
                   sketch_flops_share_of_mfma_peak=(8.0 if args.complex else 2.0) * l * m * n * count / t_med / MFMA_PEAK[dtype])
        cb, zb, indb, _ = composed()
        torch.cuda.synchronize()
        b_med, b_min, b_max = timed(composed, args.repeats)
        row.update(composed_s=b_med, composed_s_min=b_min, composed_s_max=b_max, composed_blocks_per_s=count / b_med, speedup_vs_composed=b_med / t_med)
        if si == 0:
            e_new, e_b = rel_err(a[:4], c[:4], z[:4]), rel_err(a[:4], cb[:4], zb[:4])
            eps = torch.finfo(real_dtype).eps
            row.update(err_new=e_new, err_composed=e_b, err_rule_holds=all(x <= 1.5 * y + 100 * eps for x, y in zip(e_new, e_b)),
                       same_pivots_as_composed=bool((ind[:, :k] == indb[:, :k]).all()))
        del cb, zb, indb
        if m <= 512:
            def direct():
                return rc.column_id_rank_batched(a, k, 0.0)

            direct()
            torch.cuda.synchronize()
            d_med, d_min, d_max = timed(direct, args.repeats)
            row.update(direct_batched_s=d_med, direct_batched_s_min=d_min, direct_batched_s_max=d_max, direct_batched_blocks_per_s=count / d_med,
                       speedup_vs_direct_batched=d_med / t_med)
        else:
            row.update(direct_batched="impossible: rc_column_id_rank_batched_* rejects m > 512")
        loop()
        torch.cuda.synchronize()
        l_med, l_min, l_max = timed(loop, args.repeats)
        row.update(lone_loop_blocks=LOOP_BLOCKS, lone_loop_s=l_med, lone_loop_s_min=l_min, lone_loop_s_max=l_max, lone_loop_blocks_per_s=LOOP_BLOCKS / l_med)
        if args.complex:  # (d) the real sketched call on the real parts, same shape, same run
            ar, omr = a.real.contiguous(), omega.real.contiguous()

            def real_call():
                return rc.sketch_column_id_rank_batched(ar, k, 0.0, omega=omr)

            _, rlabel = batched_launch(real_call)
            torch.cuda.synchronize()
            r_med, r_min, r_max = timed(real_call, args.repeats)
            row.update(real_sketch_id_s=r_med, real_sketch_id_s_min=r_min, real_sketch_id_s_max=r_max, real_blocks_per_s=count / r_med, real_plan=rlabel["plan"],
                       complex_over_real_time=t_med / r_med)
            del ar, omr
        results.append(row)
        print(json.dumps(row), flush=True)
        del a, omega, c, z, ind, ranks
        torch.cuda.empty_cache()
    out = dict(tool="tools/batched_sketch_id_bench.py" + (" --complex" if args.complex else ""), device=torch.cuda.get_device_name(0), results=results)
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", out_path)


if __name__ == "__main__":
    main()
