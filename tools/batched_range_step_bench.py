#!/usr/bin/env python3
"""Throughput of the batched range step (rc_sketch_range_step_batched_*) and of the power-iterated sketched column ID built on it
(batch.sketch_column_id_rank_power_batched at one iteration: range step, tall recompression with right = I, sketched ID), on the four
shapes of tools/batched_sketch_id_bench.py with one shared Gaussian omega, beside

  (0) the one-pass call rc_sketch_column_id_rank_batched_* in the same process (time ratios step / one-pass and power / one-pass);
  (t) the composition a torch caller has for one round: torch.matmul(omega, a), torch.linalg.qr of Y^T, torch.bmm(a, Q), torch.linalg.qr
      of P, timed on the first --torch-blocks blocks (torch's batched QR of tall matrices is slow) and reported per block, beside our
      own full round (round_*: the step and the tall recompression with right = I, batch.sketch_power_omega_batched).

Blocks have a decaying spectrum (tools/batched_id_bench.decaying_batch).  Every route is timed with device events after a warm-up, median
of --repeats with the spread.  The relative errors ||A - C Z||_F / ||A||_F at zero and at one iteration are recorded on the first four
blocks of every shape.  Writes profiles/batched_range_step_bench.json unless --out names another file.  Not used by the tests or by
bench.py.

--complex runs the same shapes with complex scalars (c64 / c64 / c32 / c64 in place of f64 / f64 / f32 / f64) through
rc_sketch_range_step_complex_batched_* and the _complex compositions: complex blocks of the same decaying spectrum, a complex Gaussian
omega, (t) with complex matmul / linalg.qr / bmm (Q conjugated for the projection), and beside them (r) the real step, round and
power ID on the real parts at the same shape, timed in the same run (step / round / power complex_over_real_time).  Writes
profiles/batched_range_step_complex_bench.json and leaves the real output file alone.

    python tools/batched_range_step_bench.py [--complex] [--repeats 5] [--shapes 0,1,2,3] [--torch-blocks 128] [--out path.json]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import rusty_compression_amd as rc  # noqa: E402
from rusty_compression_amd import _lib  # noqa: E402
from rusty_compression_amd.random_matrix import Rng  # noqa: E402
from tools.batched_id_bench import decaying_batch, timed  # noqa: E402
from tools.batched_sketch_id_bench import COMPLEX_OF, COPY_BW, SHAPES, rel_err  # noqa: E402


def profiled(fn):
    """fn() under the default context's event profile: (fn's result, the op:batched_* labels it recorded, in order)."""
    import ctypes

    ctx = _lib.default_context()
    lib = _lib.lib()
    labels = []
    ctx.check(lib.rc_profile_enable(ctx._h, 1))
    try:
        ctx.check(lib.rc_profile_reset(ctx._h))
        out = fn()
        cnt = ctypes.c_int32(0)
        ctx.check(lib.rc_profile_count(ctx._h, ctypes.byref(cnt)))
        for i in range(cnt.value):
            name = ctypes.create_string_buffer(192)
            ms, calls = ctypes.c_double(0), ctypes.c_int64(0)
            ctx.check(lib.rc_profile_get(ctx._h, i, name, 192, ctypes.byref(ms), ctypes.byref(calls)))
            if name.value.decode().startswith("op:batched_"):
                labels.append(name.value.decode())
    finally:
        lib.rc_profile_enable(ctx._h, 0)
        lib.rc_profile_reset(ctx._h)
    return out, labels


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--shapes", default=None)
    ap.add_argument("--torch-blocks", type=int, default=128)
    ap.add_argument("--out", default=None)
    ap.add_argument("--complex", action="store_true", help="time rc_sketch_range_step_complex_batched_c64 / _c32 on complex blocks of the same shapes")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs an MI355X")
    out_path = args.out or os.path.join(ROOT, "profiles", "batched_range_step_complex_bench.json" if args.complex else "batched_range_step_bench.json")
    cx = "_complex" if args.complex else ""
    one_pass_call, step_call = getattr(rc, "sketch_column_id_rank_batched" + cx), getattr(rc, "sketch_range_step_batched" + cx)
    power_call, omega_call = getattr(rc, "sketch_column_id_rank_power_batched" + cx), getattr(rc, "sketch_power_omega_batched" + cx)
    results = []
    for si in [int(x) for x in (args.shapes or ",".join(str(i) for i in range(len(SHAPES)))).split(",")]:
        count, m, n, l, k, dtype = SHAPES[si]
        if args.complex:
            dtype = COMPLEX_OF[dtype]
        a = decaying_batch(count, m, n, dtype, 2468 + si)
        omega = rc.random_gaussian((l, m), Rng(si), dtype)
        elem = a.element_size()

        def one_pass():
            return one_pass_call(a, k, 0.0, omega=omega)

        def step():
            return step_call(a, omega)

        def power():
            return power_call(a, k, 0.0, power_iterations=1, omega=omega)

        def full_round():  # the step and the orthonormalisation of P: what (t) computes
            return omega_call(a, k, 1, omega=omega)

        tb = min(args.torch_blocks, count)
        at = a[:tb]

        def torch_round():
            y = torch.matmul(omega, at)
            q = torch.linalg.qr(y.mT).Q
            p = torch.bmm(at, q.conj() if args.complex else q)  # a Q^H with Q = q^T: a conj(q)
            return torch.linalg.qr(p).Q

        (c0, z0, _, _), _ = profiled(one_pass)
        (c1, z1, _, _), power_labels = profiled(power)
        _, step_labels = profiled(step)
        torch.cuda.synchronize()
        o_med, o_min, o_max = timed(one_pass, args.repeats)
        s_med, s_min, s_max = timed(step, args.repeats)
        p_med, p_min, p_max = timed(power, args.repeats)
        r_med, r_min, r_max = timed(full_round, args.repeats)
        torch_round()
        torch.cuda.synchronize()
        t_med, t_min, t_max = timed(torch_round, max(2, args.repeats // 2))
        row = dict(count=count, m=m, n=n, l=l, k=k, dtype=str(dtype).replace("torch.", ""), step_label=step_labels[0], power_labels=power_labels,
                   one_pass_s=o_med, one_pass_s_min=o_min, one_pass_s_max=o_max, one_pass_blocks_per_s=count / o_med,
                   step_s=s_med, step_s_min=s_min, step_s_max=s_max, step_blocks_per_s=count / s_med, step_over_one_pass_time=s_med / o_med,
                   step_a_bytes_per_s_share_of_copy_bw=2 * count * m * n * elem / s_med / COPY_BW,
                   power_q1_s=p_med, power_q1_s_min=p_min, power_q1_s_max=p_max, power_q1_blocks_per_s=count / p_med,
                   power_q1_over_one_pass_time=p_med / o_med,
                   torch_round_blocks=tb, torch_round_s=t_med, torch_round_s_min=t_min, torch_round_s_max=t_max, torch_round_blocks_per_s=tb / t_med,
                   round_s=r_med, round_s_min=r_min, round_s_max=r_max, round_blocks_per_s=count / r_med,
                   round_speedup_vs_torch_round=(t_med / tb) / (r_med / count),
                   err_q0=rel_err(a[:4], c0[:4], z0[:4]), err_q1=rel_err(a[:4], c1[:4], z1[:4]))
        if args.complex:  # (r) the real calls on the real parts, same shape, same run
            ar, omr = a.real.contiguous(), omega.real.contiguous()
            rs_med, _, _ = timed(lambda: rc.sketch_range_step_batched(ar, omr), args.repeats)
            rr_med, _, _ = timed(lambda: rc.sketch_power_omega_batched(ar, k, 1, omega=omr), args.repeats)
            rp_med, _, _ = timed(lambda: rc.sketch_column_id_rank_power_batched(ar, k, 0.0, power_iterations=1, omega=omr), args.repeats)
            row.update(real_step_s=rs_med, real_step_blocks_per_s=count / rs_med, step_complex_over_real_time=s_med / rs_med,
                       real_round_s=rr_med, real_round_blocks_per_s=count / rr_med, round_complex_over_real_time=r_med / rr_med,
                       real_power_q1_s=rp_med, real_power_q1_blocks_per_s=count / rp_med, power_q1_complex_over_real_time=p_med / rp_med)
            del ar, omr
        results.append(row)
        print(json.dumps(row), flush=True)
        del a, omega, at, c0, z0, c1, z1
        torch.cuda.empty_cache()
    out = dict(tool="tools/batched_range_step_bench.py" + (" --complex" if args.complex else ""), device=torch.cuda.get_device_name(0), results=results)
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", out_path)


if __name__ == "__main__":
    main()
