#!/usr/bin/env python3
"""Throughput of the block-sparse operator (rc_block_operator_apply_*) against the compositions it replaces.

Each case is a block low-rank matrix of G block rows with E entries each, every entry its own block (Gaussian factors at full rank k, so
every byte of the factors is read): entry j of block row g sits at block column (g + j * 7) mod G.  Timed with device events after
warm-up, median of --repeats:

  operator    one rc_block_operator_apply_* call;
  composed    what a caller of the parent commit writes: gather the segments of x (index_select), rc.lowrank_apply_batched,
              index_add_ into y -- three launches, two extra buffers, atomics on y;
  bmm         the same gather and scatter around a torch.bmm chain (right @ b, then left @ .);
  apply       rc.lowrank_apply_batched alone on the pre-gathered segments: the rate the operator is expected to reach when
              groups x tiles fills the grid (its traffic differs by the y it does not write per entry, about 1 / k).

The mixed case replaces 10 % of the entries by dense blocks (one torch.bmm more in the compositions).  Bytes are algorithmic: every
factor and dense block once, the x segment of every entry, y once; the fraction is of the 6.29 TB/s a float4 copy reaches on the
MI355X.  The plan label of the launch (tile width, grid, slots) is read from the event profile.  Writes profiles/batched_operator_apply_bench.json unless --out names another file.  Not used by the tests or by bench.py.

--mixed measures the mixed-storage operator instead (rc_block_operator_apply_mixed_f64 / _c64: low-rank factors kept in f32 / c32,
dense blocks, x and y in full precision) on cases 0, 1, 3 and 4: the factors are demoted and promoted back, and the full-precision call
on the promoted factors (the yardstick: this library's unchanged kernel) and the mixed call on the stored ones are timed in the same
process by the same method and checked to give the same bits.  Bytes as above with the factor elements at their stored size.  Writes
profiles/batched_operator_apply_mixed_bench.json.

    python tools/batched_operator_apply_bench.py [--repeats 5] [--cases 0,1,2,3,4] [--out path.json] [--mixed]
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
from tests.helpers import batched_launch  # noqa: E402
from tools.batched_id_bench import timed  # noqa: E402

CASES = [  # (groups, entries per group, m = n, k, nrhs, dtype, dense share)
    (4096, 16, 256, 32, 1, torch.float64, 0.0),
    (4096, 16, 256, 32, 16, torch.float64, 0.0),
    (128, 128, 128, 64, 1, torch.float64, 0.0),   # the few-groups limit: 128 units for a grid of several hundred workgroups
    (4096, 16, 128, 32, 1, torch.complex128, 0.0),
    (4096, 16, 256, 32, 1, torch.float64, 0.1),
]
COPY_BW = 6.29e12  # bytes/s, measured float4 copy


def scatter_add(y, index, src):
    """y[index[i]] += src[i] (index_add_, atomics); complex data as (re, im) pairs."""
    if y.dtype.is_complex:
        torch.view_as_real(y).index_add_(0, index, torch.view_as_real(src.contiguous()))
    else:
        y.index_add_(0, index, src)


def randn(shape, dtype, gen):
    return torch.randn(shape, generator=gen, device="cuda", dtype=dtype)


def main_mixed(args):
    out_path = args.out or os.path.join(ROOT, "profiles", "batched_operator_apply_mixed_bench.json")
    results = []
    for ci in [int(v) for v in (args.cases or "0,1,3,4").split(",")]:
        groups, per, mn, k, nrhs, dtype, share = CASES[ci]
        m = n = mn
        gen = torch.Generator(device="cuda").manual_seed(100 + ci)
        total = groups * per
        g_of, j_of = np.repeat(np.arange(groups), per), np.tile(np.arange(per), groups)
        rows, cols = g_of * m, ((g_of + j_of * 7) % groups) * n
        is_dense = np.zeros(total, dtype=bool)
        if share > 0:
            is_dense[np.random.default_rng(ci).choice(total, int(total * share), replace=False)] = True
        count, dcount = int((~is_dense).sum()), int(is_dense.sum())
        ids = np.empty(total, dtype=np.int64)
        ids[~is_dense], ids[is_dense] = np.arange(count), count + np.arange(dcount)
        low = [rc.demote_batched(randn((count, m, k), dtype, gen) / k ** 0.5), rc.demote_batched(randn((count, k, n), dtype, gen) / n ** 0.5)]
        up = [rc.promote_batched(v) for v in low]
        dense = randn((dcount, m, n), dtype, gen) / n ** 0.5 if dcount else None
        x = randn((groups * n, nrhs), dtype, gen)
        y_full, y_mixed = (torch.zeros((groups * m, nrhs), dtype=dtype, device="cuda") for _ in range(2))
        pattern, _ = rc.block_csr(rows, cols, ids)
        dev_pattern = tuple(torch.from_numpy(v).cuda() for v in pattern)

        def full():
            rc.block_operator_apply(x, *dev_pattern, left=up[0], right=up[1], dense=dense, y=y_full)

        def mixed():
            rc.block_operator_apply_mixed(x, *dev_pattern, left=low[0], right=low[1], dense=dense, y=y_mixed)

        full()
        _, label = batched_launch(mixed)  # warm-up, and the plan, grid and slots of the launch from the event profile
        torch.cuda.synchronize()
        same = bool(torch.equal(y_full, y_mixed))
        es, ss = up[0].element_size(), low[0].element_size()
        other = es * (dcount * m * n + total * n * nrhs + groups * m * nrhs)
        bytes_full, bytes_mixed = es * count * (m * k + k * n) + other, ss * count * (m * k + k * n) + other
        # full, mixed, full again: the second full run shows how far the yardstick itself moves between two measurements
        t_full, t_mixed, t_again = timed(full, args.repeats), timed(mixed, args.repeats), timed(full, args.repeats)
        row = dict(case=ci, groups=groups, entries_per_group=per, m=m, n=n, k=k, nrhs=nrhs, dtype=str(dtype).replace("torch.", ""),
                   storage=str(low[0].dtype).replace("torch.", ""), dense_entries=dcount, op=label["op"], plan=label["plan"], grid=label["grid"],
                   slots=label["slots"], bit_equal=same,
                   full=dict(seconds=t_full[0], min=t_full[1], max=t_full[2], again=t_again[0], bytes=bytes_full, blocks_per_s=total / t_full[0],
                             share_of_copy_bandwidth=bytes_full / t_full[0] / COPY_BW),
                   mixed=dict(seconds=t_mixed[0], min=t_mixed[1], max=t_mixed[2], bytes=bytes_mixed, blocks_per_s=total / t_mixed[0],
                              share_of_copy_bandwidth=bytes_mixed / t_mixed[0] / COPY_BW),
                   bytes_ratio=bytes_full / bytes_mixed, speedup=t_full[0] / t_mixed[0])
        print(json.dumps(row), flush=True)
        results.append(row)
        del low, up, dense, x, y_full, y_mixed
        torch.cuda.empty_cache()
    with open(out_path, "w") as f:
        json.dump(dict(tool="tools/batched_operator_apply_bench.py --mixed", device=torch.cuda.get_device_name(0), repeats=args.repeats,
                       copy_bandwidth=COPY_BW, cases=results), f, indent=1)
        f.write("\n")
    print("wrote", out_path)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--cases", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--mixed", action="store_true", help="time the mixed-storage operator against the full-precision call on promoted factors")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs an MI355X")
    if args.mixed:
        return main_mixed(args)
    out_path = args.out or os.path.join(ROOT, "profiles", "batched_operator_apply_bench.json")
    results = []
    for ci in [int(v) for v in (args.cases or ",".join(str(i) for i in range(len(CASES)))).split(",")]:
        groups, per, mn, k, nrhs, dtype, share = CASES[ci]
        m = n = mn
        gen = torch.Generator(device="cuda").manual_seed(100 + ci)
        total = groups * per
        g_of, j_of = np.repeat(np.arange(groups), per), np.tile(np.arange(per), groups)
        rows, cols = g_of * m, ((g_of + j_of * 7) % groups) * n
        is_dense = np.zeros(total, dtype=bool)
        if share > 0:
            is_dense[np.random.default_rng(ci).choice(total, int(total * share), replace=False)] = True
        count, dcount = int((~is_dense).sum()), int(is_dense.sum())
        ids = np.empty(total, dtype=np.int64)
        ids[~is_dense], ids[is_dense] = np.arange(count), count + np.arange(dcount)
        left, right = randn((count, m, k), dtype, gen) / k ** 0.5, randn((count, k, n), dtype, gen) / n ** 0.5
        dense = randn((dcount, m, n), dtype, gen) / n ** 0.5 if dcount else None
        x = randn((groups * n, nrhs), dtype, gen)
        y = torch.zeros((groups * m, nrhs), dtype=dtype, device="cuda")
        pattern, _ = rc.block_csr(rows, cols, ids)
        dev_pattern = tuple(torch.from_numpy(v).cuda() for v in pattern)

        def operator():
            rc.block_operator_apply(x, *dev_pattern, left=left, right=right, dense=dense, y=y)

        # the compositions: entries in the pattern's order, low-rank ones first in the gathered buffers
        e_block, e_col = pattern[2], pattern[3]
        e_row = np.repeat(pattern[1], np.diff(pattern[0]))
        lr = e_block < count
        span_n, span_m = torch.arange(n, device="cuda"), torch.arange(m, device="cuda")
        to_dev = lambda v: torch.from_numpy(np.ascontiguousarray(v)).cuda()  # noqa: E731
        gather_lr = (to_dev(e_col[lr])[:, None] + span_n).reshape(-1)
        scatter_lr = (to_dev(e_row[lr])[:, None] + span_m).reshape(-1)
        gather_d = (to_dev(e_col[~lr])[:, None] + span_n).reshape(-1) if dcount else None
        scatter_d = (to_dev(e_row[~lr])[:, None] + span_m).reshape(-1) if dcount else None
        # the entries name the blocks of either kind in storage order, so the compositions use the batches where they lie
        assert np.array_equal(e_block[lr], np.arange(count)) and np.array_equal(e_block[~lr] - count, np.arange(dcount))

        def dense_part(yy):
            if dcount:
                scatter_add(yy, scatter_d, torch.bmm(dense, x.index_select(0, gather_d).view(dcount, n, nrhs)).view(-1, nrhs))

        def composed():
            yy = torch.zeros_like(y)
            b = x.index_select(0, gather_lr).view(count, n, nrhs)
            scatter_add(yy, scatter_lr, rc.lowrank_apply_batched(left, right, b=b).view(-1, nrhs))
            dense_part(yy)
            return yy

        def bmm():
            yy = torch.zeros_like(y)
            b = x.index_select(0, gather_lr).view(count, n, nrhs)
            scatter_add(yy, scatter_lr, torch.bmm(left, torch.bmm(right, b)).view(-1, nrhs))
            dense_part(yy)
            return yy

        b_fixed = x.index_select(0, gather_lr).view(count, n, nrhs).contiguous()

        def apply():
            rc.lowrank_apply_batched(left, right, b=b_fixed)

        _, label = batched_launch(operator)  # warm-up, and the plan, grid and slots of the launch from the event profile
        ref = composed()
        torch.cuda.synchronize()
        err = float((y - ref).abs().max() / ref.abs().max())  # the compositions add in another order: rounding level, not bits
        assert err < (1e-4 if dtype in (torch.float32, torch.complex64) else 1e-11), err
        del ref
        es = torch.empty(0, dtype=dtype).element_size()
        nbytes = es * (count * (m * k + k * n) + dcount * m * n + total * n * nrhs + groups * m * nrhs)
        row = dict(case=ci, groups=groups, entries_per_group=per, m=m, n=n, k=k, nrhs=nrhs, dtype=str(dtype).replace("torch.", ""),
                   dense_entries=dcount, plan=label["plan"], grid=label["grid"], slots=label["slots"], algorithmic_bytes=nbytes,
                   max_rel_diff_vs_composed=err)
        for name, fn in (("operator", operator), ("composed", composed), ("bmm", bmm), ("apply", apply)):
            fn()
            torch.cuda.synchronize()
            med, lo, hi = timed(fn, args.repeats)
            row[name] = dict(seconds=med, min=lo, max=hi, blocks_per_s=(count if name == "apply" else total) / med)
        row["operator"]["share_of_copy_bandwidth"] = nbytes / row["operator"]["seconds"] / COPY_BW
        for name in ("composed", "bmm"):
            row[f"speedup_vs_{name}"] = row[name]["seconds"] / row["operator"]["seconds"]
        row["operator_rate_over_apply_rate"] = row["operator"]["blocks_per_s"] / row["apply"]["blocks_per_s"]
        print(json.dumps(row))
        results.append(row)
        del left, right, dense, x, y, b_fixed
        torch.cuda.empty_cache()
    with open(out_path, "w") as f:
        json.dump(dict(tool="tools/batched_operator_apply_bench.py", repeats=args.repeats, copy_bandwidth=COPY_BW, cases=results), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
