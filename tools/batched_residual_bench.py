#!/usr/bin/env python3
"""Throughput of the batched residual norms (rc_lowrank_residual_batched_*) on the factors of the library's own batched compressors,
beside the two routes a caller had without it:

  (a) the torch composition: a - torch.bmm(c, z), then torch.linalg.matrix_norm of the difference and of a (the zero tails of c and z
      make it rank-correct);
  (b) where m <= 512: rc_lowrank_apply_batched_* rebuilding every block (to_mat), then the same subtraction and norms.

Shapes: the four of tools/batched_sketch_id_bench.py with the factors of the sketched column ID, and 16384 blocks of 128 x 128 with the
factors of rc_column_id_rank_batched_* at tol = 1e-8, so that the ranks vary.  Every route is timed with device events after a warm-up,
median of --repeats with the spread.  Reported per shape: blocks/s, the bytes of a, left and right per second as a share of the
6.29 TB/s copy bandwidth, and the plan label of the launch.  On the first 8 blocks of every shape err of the new call is held to the
bound of tests/residual_ref.py against the host, and err of routes (a) and (b) to the same bound against the new call.
Writes profiles/batched_residual_bench.json unless --out names another file.  Not used by the tests or by bench.py.

--complex times rc_lowrank_residual_batched_c64 / _c32 on the same shapes: complex blocks of the same decaying spectrum and the factors of
rc_column_id_rank_batched_c* (for m > 512, beyond that call's domain, of the sketch omega a with c gathered from a, which is what the
sketched column ID does for real data), beside (a) and (b) on the same data and the real call on a real batch of the same shape in the
same run (complex_over_real_time; two to four is expected: twice the bytes, four times the MFMAs).  The checks use the bound of
tests/residual_ref_complex.py.  Writes profiles/batched_residual_complex_bench.json.

    python tools/batched_residual_bench.py [--complex] [--repeats 5] [--shapes 0,1,2,3,4] [--out path.json]
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
from rusty_compression_amd.random_matrix import Rng  # noqa: E402
from tests import residual_ref as rr  # noqa: E402
from tests import residual_ref_complex as rrc  # noqa: E402
from tests.helpers import batched_launch  # noqa: E402
from tools.batched_id_bench import decaying_batch, timed  # noqa: E402

SHAPES = [  # (count, m, n, l, k, tol, dtype); l = 0: rc_column_id_rank_batched_* instead of the sketched ID
    (2048, 2048, 256, 40, 32, 0.0, torch.float64),
    (8192, 512, 256, 40, 32, 0.0, torch.float64),
    (2048, 1024, 512, 72, 64, 0.0, torch.float32),
    (512, 8192, 128, 24, 16, 0.0, torch.float64),
    (16384, 128, 128, 0, 64, 1e-8, torch.float64),
]
COPY_BW = 6.29e12
CHECKED_BLOCKS = 8
COMPLEX_OF = {torch.float64: torch.complex128, torch.float32: torch.complex64}


def real_factors(si):
    """The real run's input of SHAPES[si]: (a, c, z, ranks)."""
    count, m, n, l, k, tol, dtype = SHAPES[si]
    a = decaying_batch(count, m, n, dtype, 1357 + si)
    if l:
        c, z, _, ranks = rc.sketch_column_id_rank_batched(a, k, tol, omega=rc.random_gaussian((l, m), Rng(si), dtype))
    else:
        c, z, _, ranks = rc.column_id_rank_batched(a, k, tol)
    return a, c, z, ranks


def complex_factors(si):
    """Complex blocks of SHAPES[si] and column-ID factors from rc_column_id_rank_batched_c*: of the blocks themselves when m <= 512, else of
    their sketches omega a (omega complex Gaussian, l x m) with c gathered from a and zeroed past the rank."""
    count, m, n, l, k, tol, dtype = SHAPES[si]
    cdt = COMPLEX_OF[dtype]
    a = decaying_batch(count, m, n, cdt, 1357 + si)
    if not l:
        c, z, _, ranks = rc.column_id_rank_batched(a, k, tol)
        return a, c, z, ranks
    g = torch.Generator(device="cuda").manual_seed(si)
    omega = torch.randn(l, m, generator=g, device="cuda", dtype=cdt)
    _, z, ind, ranks = rc.column_id_rank_batched(torch.matmul(omega, a), k, tol)
    kk = z.shape[1]
    c = torch.gather(a, 2, ind[:, None, :kk].expand(count, m, kk))
    c = c * (torch.arange(kk, device="cuda")[None, :] < ranks[:, None])[:, None, :].to(cdt)
    return a, c.contiguous(), z, ranks


def main_complex(args):
    out_path = args.out or os.path.join(ROOT, "profiles", "batched_residual_complex_bench.json")
    results = []
    for si in [int(x) for x in (args.shapes or ",".join(str(i) for i in range(len(SHAPES)))).split(",")]:
        count, m, n, l, k, tol, dtype = SHAPES[si]
        # the real call on the real run's input, for the ratio
        ar, cr, zr, rr_ = real_factors(si)
        real_fn = lambda: rc.column_id_residual_batched(ar, cr, zr, rr_)  # noqa: E731
        real_fn()
        torch.cuda.synchronize()
        r_med, r_min, r_max = timed(real_fn, args.repeats)
        del ar, cr, zr, rr_
        torch.cuda.empty_cache()
        a, c, z, ranks = complex_factors(si)
        elem = a.element_size()

        def new():
            return rc.column_id_residual_batched_complex(a, c, z, ranks)

        def composed():
            return torch.linalg.matrix_norm(a - torch.bmm(c, z)), torch.linalg.matrix_norm(a)

        def applied():
            return torch.linalg.matrix_norm(a - rc.column_id_apply_batched(c, z, ranks)), torch.linalg.matrix_norm(a)

        (err, nrm), label = batched_launch(new)  # warm-up (code objects, workspace) and the plan
        torch.cuda.synchronize()
        t_med, t_min, t_max = timed(new, args.repeats)
        rk = ranks.cpu().numpy()
        row = dict(count=count, m=m, n=n, k=k, tol=tol, dtype=str(a.dtype).replace("torch.", ""),
                   compressor="column_id of the sketch, c gathered" if l else "column_id", rank_min=int(rk.min()), rank_max=int(rk.max()),
                   plan=label["plan"], grid=label["grid"], slots=label["slots"], residual_s=t_med, residual_s_min=t_min, residual_s_max=t_max,
                   blocks_per_s=count / t_med, bytes_per_s_share_of_copy_bw=count * (m * n + m * k + k * n) * elem / t_med / COPY_BW,
                   real_residual_s=r_med, real_residual_s_min=r_min, real_residual_s_max=r_max, real_blocks_per_s=count / r_med,
                   complex_over_real_time=t_med / r_med)
        err_b, nrm_b = composed()
        torch.cuda.synchronize()
        b_med, b_min, b_max = timed(composed, args.repeats)
        row.update(composed_s=b_med, composed_s_min=b_min, composed_s_max=b_max, composed_blocks_per_s=count / b_med, speedup_vs_composed=b_med / t_med)
        npdt = np.complex128 if a.dtype == torch.complex128 else np.complex64
        ratios, agree, bounds = [], [], []
        for i in range(CHECKED_BLOCKS):
            ai, ci, zi, r = a[i].cpu().numpy(), c[i].cpu().numpy(), z[i].cpu().numpy(), int(rk[i])
            _, e_ref = rrc.reference(ai, ci, zi, None, None, r)
            _, err_bound, _ = rrc.bound(ai, ci, zi, None, None, r, npdt, rrc.chain_length(m, n))
            ratios.append(abs(float(err[i]) - float(np.linalg.norm(e_ref))) / err_bound)
            agree.append(abs(float(err[i]) - float(err_b[i])) / err_bound)
            bounds.append(err_bound)
        row.update(err_first=[float(x) for x in err[:CHECKED_BLOCKS]], err_composed_first=[float(x) for x in err_b[:CHECKED_BLOCKS]],
                   err_vs_host_over_bound=ratios, err_vs_composed_over_bound=agree)
        assert max(ratios) <= 1.0 and max(agree) <= 1.0, row
        del err_b, nrm_b
        if m <= 512:
            err_p, _ = applied()
            torch.cuda.synchronize()
            agree_p = [abs(float(err[i]) - float(err_p[i])) / bounds[i] for i in range(CHECKED_BLOCKS)]
            row.update(err_vs_apply_route_over_bound=agree_p)
            assert max(agree_p) <= 1.0, row
            del err_p
            p_med, p_min, p_max = timed(applied, args.repeats)
            row.update(apply_route_s=p_med, apply_route_s_min=p_min, apply_route_s_max=p_max, apply_route_blocks_per_s=count / p_med,
                       speedup_vs_apply_route=p_med / t_med)
        else:
            row.update(apply_route="impossible: rc_lowrank_apply_batched_* rejects m > 512")
        results.append(row)
        print(json.dumps(row), flush=True)
        del a, c, z, ranks, err, nrm
        torch.cuda.empty_cache()
    out = dict(tool="tools/batched_residual_bench.py --complex", device=torch.cuda.get_device_name(0), results=results)
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", out_path)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--shapes", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--complex", action="store_true", help="time rc_lowrank_residual_batched_c64 / _c32 on complex blocks of the same shapes")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs an MI355X")
    if args.complex:
        return main_complex(args)
    out_path = args.out or os.path.join(ROOT, "profiles", "batched_residual_bench.json")
    results = []
    for si in [int(x) for x in (args.shapes or ",".join(str(i) for i in range(len(SHAPES)))).split(",")]:
        count, m, n, l, k, tol, dtype = SHAPES[si]
        a = decaying_batch(count, m, n, dtype, 1357 + si)
        if l:
            c, z, _, ranks = rc.sketch_column_id_rank_batched(a, k, tol, omega=rc.random_gaussian((l, m), Rng(si), dtype))
        else:
            c, z, _, ranks = rc.column_id_rank_batched(a, k, tol)
        elem = a.element_size()

        def new():
            return rc.column_id_residual_batched(a, c, z, ranks)

        def composed():
            return torch.linalg.matrix_norm(a - torch.bmm(c, z)), torch.linalg.matrix_norm(a)

        def applied():
            return torch.linalg.matrix_norm(a - rc.column_id_apply_batched(c, z, ranks)), torch.linalg.matrix_norm(a)

        (err, nrm), label = batched_launch(new)  # warm-up (code objects, workspace) and the plan
        torch.cuda.synchronize()
        t_med, t_min, t_max = timed(new, args.repeats)
        rk = ranks.cpu().numpy()
        row = dict(count=count, m=m, n=n, k=k, tol=tol, dtype=str(dtype).replace("torch.", ""), compressor="sketch_column_id" if l else "column_id",
                   rank_min=int(rk.min()), rank_max=int(rk.max()), plan=label["plan"], grid=label["grid"], slots=label["slots"],
                   residual_s=t_med, residual_s_min=t_min, residual_s_max=t_max, blocks_per_s=count / t_med,
                   bytes_per_s_share_of_copy_bw=count * (m * n + m * k + k * n) * elem / t_med / COPY_BW)
        err_b, nrm_b = composed()
        torch.cuda.synchronize()
        b_med, b_min, b_max = timed(composed, args.repeats)
        row.update(composed_s=b_med, composed_s_min=b_min, composed_s_max=b_max, composed_blocks_per_s=count / b_med, speedup_vs_composed=b_med / t_med)
        # the first blocks against the host and the two routes against each other
        npdt = np.float64 if dtype == torch.float64 else np.float32
        ratios, agree, bounds = [], [], []
        for i in range(CHECKED_BLOCKS):
            ai, ci, zi, r = a[i].cpu().numpy(), c[i].cpu().numpy(), z[i].cpu().numpy(), int(rk[i])
            _, e_ref = rr.reference(ai, ci, zi, None, None, r)
            _, err_bound, _ = rr.bound(ai, ci, zi, None, None, r, npdt, rr.chain_length(m, n))
            ratios.append(abs(float(err[i]) - float(np.linalg.norm(e_ref))) / err_bound)
            agree.append(abs(float(err[i]) - float(err_b[i])) / err_bound)
            bounds.append(err_bound)
        row.update(err_first=[float(x) for x in err[:CHECKED_BLOCKS]], err_composed_first=[float(x) for x in err_b[:CHECKED_BLOCKS]],
                   err_vs_host_over_bound=ratios, err_vs_composed_over_bound=agree)
        assert max(ratios) <= 1.0 and max(agree) <= 1.0, row
        del err_b, nrm_b
        if m <= 512:
            err_p, _ = applied()
            torch.cuda.synchronize()
            agree_p = [abs(float(err[i]) - float(err_p[i])) / bounds[i] for i in range(CHECKED_BLOCKS)]
            row.update(err_vs_apply_route_over_bound=agree_p)
            assert max(agree_p) <= 1.0, row
            del err_p
            p_med, p_min, p_max = timed(applied, args.repeats)
            row.update(apply_route_s=p_med, apply_route_s_min=p_min, apply_route_s_max=p_max, apply_route_blocks_per_s=count / p_med,
                       speedup_vs_apply_route=p_med / t_med)
        else:
            row.update(apply_route="impossible: rc_lowrank_apply_batched_* rejects m > 512")
        results.append(row)
        print(json.dumps(row), flush=True)
        del a, c, z, ranks, err, nrm
        torch.cuda.empty_cache()
    out = dict(tool="tools/batched_residual_bench.py", device=torch.cuda.get_device_name(0), results=results)
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", out_path)


if __name__ == "__main__":
    main()
