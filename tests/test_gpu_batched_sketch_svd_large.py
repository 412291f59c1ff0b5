"""The randomized SVD of wide blocks built on the batched sketch product (batch.sketch_range_step_large_batched,
batch.sketch_svd_rank_large_batched): for n > 512 the range step is three launches (Y = omega a by rc_sketch_product_batched_*, the row
basis by rc_lowrank_recompress_tall_batched_* on Y^T with right = I, P = a Q^T by the product on transposed views) and the chain ends with
rc_lowrank_recompress_large_batched_*; for n <= 512 both delegate to the one-launch range step's compositions.

Checked: the wiring (the outputs are those of the public pieces called by hand in the documented order, bit for bit) and the delegation;
the step's contract (zero rows of Q and columns of P from the rank on, orthonormality of Q and the span of Y within 100 l eps, P inside the
dot-product bound |p - a Q^T| <= c (n + 4) u (|a| |Q^T|), c = 1 (f32) or 2 (f64), with the device's own Q); the accuracy of the chain at
one and two steps against the host model of tests/range_step_ref.py under the power-SVD test's rules (err <= 1.5 host err + 100 eps,
orthonormality of U and Vt <= 4 TOL[dtype]["orth"], S descending and positive); the tolerance case's rank; a zero block; and the C++
mirror's compositions (tests/cpp/batched_sketch_product_example.cpp, whose range step writes u through the transposed view of q).

The host model runs once per case and step count on the f64 values; the f32 blocks are those values rounded, a relative change of 6e-8
in a block against errors of 0.06 to 0.43 under a factor of 1.5."""
import os
import subprocess

import numpy as np
import pytest
import torch

import rusty_compression_amd as rc
from tests import range_step_ref as ref
from tests import sketch_large_cases as cases
from tests.helpers import TOL, npy
from tests.test_abi_cpu import build_cpp_mirror_examples

pytestmark = pytest.mark.gpu

DTYPES = [np.float64, np.float32]
TDTYPES = [torch.float64, torch.float32]


def tt(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def same_bits(x, y):
    x, y = np.asarray(x), np.asarray(y)
    return x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes()


def host(ts):
    torch.cuda.synchronize()
    return tuple(npy(t.contiguous()) for t in ts)


def eye(l, cnt, dtype):
    return torch.eye(l, dtype=dtype, device="cuda").expand(cnt, l, l)


def step_by_hand(a, om):
    """The documented three launches of one range step for n > 512."""
    cnt, m, n = a.shape
    l = om.shape[-2]
    y = rc.sketch_product_batched(a, om)
    u, _, _, ranks = rc.lowrank_recompress_tall_batched(y.mT, eye(l, cnt, a.dtype), l, 0.0)
    q = u.mT
    p = torch.empty((cnt, m, l), dtype=a.dtype, device="cuda")
    rc.sketch_product_batched(a.mT, q, out=p.mT)
    return q, p, ranks


# ---------------------------------------------------------------- 1. wiring
@pytest.mark.parametrize("dtype", TDTYPES)
def test_the_chain_is_the_public_pieces_called_by_hand(dtype):
    rng = np.random.default_rng(21)
    cnt, m, n, l, k = 2, 600, 700, 40, 32
    a = tt(rng.standard_normal((cnt, m, n))).to(dtype)
    om = tt(rng.standard_normal((l, m))).to(dtype)
    q, p, ranks = step_by_hand(a, om)
    for w, g in zip(host((q, p, ranks)), host(rc.sketch_range_step_large_batched(a, om))):
        assert same_bits(w, g)
    # one step: the large recompression of (p, q) at the step's ranks
    for w, g in zip(host(rc.lowrank_recompress_large_batched(p, q, k, 1e-6, ranks=ranks)), host(rc.sketch_svd_rank_large_batched(a, k, 1e-6, 1, omega=om))):
        assert same_bits(w, g)
    # two steps: p orthonormalised by the tall recompression with right = I at the step's ranks, u^T the next omega
    om2 = rc.lowrank_recompress_tall_batched(p, eye(l, cnt, dtype), l, 0.0, ranks=ranks)[0].mT
    q2, p2, ranks2 = step_by_hand(a, om2)
    for w, g in zip(host(rc.lowrank_recompress_large_batched(p2, q2, k, 1e-6, ranks=ranks2)), host(rc.sketch_svd_rank_large_batched(a, k, 1e-6, 2, omega=om))):
        assert same_bits(w, g)
    # the default omega is the sketched ID's
    drawn = rc.random_gaussian((k + 4, m), rc.Rng(5), dtype)
    for w, g in zip(host(rc.sketch_range_step_large_batched(a, drawn)), host(rc.sketch_range_step_large_batched(a, k=k, oversampling=4, seed=5))):
        assert same_bits(w, g)
    for w, g in zip(host(rc.sketch_svd_rank_large_batched(a, k, omega=drawn)), host(rc.sketch_svd_rank_large_batched(a, k, oversampling=4, seed=5))):
        assert same_bits(w, g)


# ---------------------------------------------------------------- 2. delegation
@pytest.mark.parametrize("dtype", TDTYPES)
def test_narrow_blocks_delegate_to_the_one_launch_step(dtype):
    rng = np.random.default_rng(22)
    cnt, m, n, l, k = 2, 1030, 300, 40, 32
    a = tt(rng.standard_normal((cnt, m, n))).to(dtype)
    om = tt(rng.standard_normal((l, m))).to(dtype)
    for w, g in zip(host(rc.sketch_range_step_batched(a, om)), host(rc.sketch_range_step_large_batched(a, om))):
        assert same_bits(w, g)
    for its in (1, 2):
        for w, g in zip(host(rc.sketch_svd_rank_power_batched(a, k, 1e-6, its, omega=om)), host(rc.sketch_svd_rank_large_batched(a, k, 1e-6, its, omega=om))):
            assert same_bits(w, g)


# ---------------------------------------------------------------- 3. the step's contract
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m,n,l", [(130, 513, 24), (600, 700, 40), (70, 1100, 64)])
def test_step_of_a_wide_block(m, n, l, dtype):
    """Three blocks: Gaussian under a full omega (r = l); Gaussian under an omega whose last three rows are zero, so Y^T has three exactly
    zero columns, the recompression three exactly zero singular values and r = l - 3; and a zero block (r = 0)."""
    rng = np.random.default_rng(100 * m + n)
    a = rng.standard_normal((3, m, n)).astype(dtype)
    a[2] = 0
    om = rng.standard_normal((3, l, m)).astype(dtype)
    om[1, l - 3:] = 0
    ad = tt(a)
    q, p, ranks = host(rc.sketch_range_step_large_batched(ad, tt(om)))
    y = host((rc.sketch_product_batched(ad, tt(om)),))[0]
    assert q.shape == (3, l, n) and p.shape == (3, m, l) and q.dtype == p.dtype == np.dtype(dtype)
    assert list(ranks) == [l, l - 3, 0]
    u = np.finfo(dtype).eps / 2
    cst = 1.0 if dtype == np.float32 else 2.0
    for i in range(3):
        r = int(ranks[i])
        assert not np.any(q[i][r:]) and not np.any(p[i][:, r:])
        assert np.all(np.isfinite(q[i])) and np.all(np.isfinite(p[i]))
        a64, q64, y64 = a[i].astype(np.float64), q[i].astype(np.float64), y[i].astype(np.float64)
        if r:
            orth = np.linalg.norm(q64[:r] @ q64[:r].T - np.eye(r))
            span = np.linalg.norm(y64 - (y64 @ q64[:r].T) @ q64[:r]) / np.linalg.norm(y64)
            print(f"large step {m}x{n} l={l} {np.dtype(dtype).name} block {i}: r {r} orth {orth:.3e} span {span:.3e} (bound {100 * l * np.finfo(dtype).eps:.1e})")
            assert orth <= 100 * l * np.finfo(dtype).eps and span <= 100 * l * np.finfo(dtype).eps
        bound = cst * (n + 4) * u * (np.abs(a64) @ np.abs(q64.T))
        err = np.abs(p[i].astype(np.float64) - a64 @ q64.T)
        print(f"    projection: max |p - a q^T| / bound = {float(np.max(err / np.maximum(bound, np.finfo(np.float64).tiny))):.3e}")
        assert np.all(err <= bound)


# ---------------------------------------------------------------- 4. accuracy against the host model
_HOST = {}


def host_model(case, steps):
    """(relative error, rank) of the host model on the f64 values of a case (run once per case and step count)."""
    if (case, steps) not in _HOST:
        a, om = cases.block_and_omega(case)
        _HOST[(case, steps)] = ref.svd_power(a, om, case[3], 0.0, steps)
    return _HOST[(case, steps)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("steps", [1, 2])
@pytest.mark.parametrize("case", cases.CASES)
def test_large_svd_against_the_host_model(case, steps, dtype):
    m, n, l, k = case
    a64, om64 = cases.block_and_omega(case)
    a, om = a64.astype(dtype), om64.astype(dtype)
    u, s, vt, ranks = host(rc.sketch_svd_rank_large_batched(tt(a[None]), k, 0.0, steps, omega=tt(om)))
    assert u.shape == (1, m, k) and vt.shape == (1, k, n) and ranks[0] == k
    u0, s0, vt0 = u[0].astype(np.float64), s[0][:k].astype(np.float64), vt[0].astype(np.float64)
    orth = max(np.abs(u0.T @ u0 - np.eye(k)).max(), np.abs(vt0 @ vt0.T - np.eye(k)).max())
    err = np.linalg.norm(a.astype(np.float64) - (u0 * s0) @ vt0) / np.linalg.norm(a.astype(np.float64))
    oerr, orank = host_model(case, steps)
    print(f"large SVD {m}x{n} l={l} k={k} steps={steps} {np.dtype(dtype).name}: err {err:.4e} host {oerr:.4e}; orth {orth:.3e} "
          f"bound {4 * TOL[np.dtype(dtype)]['orth']:.3e}")
    assert orank == k
    assert orth <= 4 * TOL[np.dtype(dtype)]["orth"]
    assert np.all(np.diff(s0) <= 0) and s0[-1] > 0
    assert err <= 1.5 * oerr + 100 * np.finfo(dtype).eps


# ---------------------------------------------------------------- 5. the tolerance case
@pytest.mark.parametrize("dtype", DTYPES)
def test_tolerance_case_reaches_rank_22(dtype):
    m, n, l, k = cases.TOL_CASE
    a64, om64 = cases.block_and_omega(cases.TOL_CASE, cases.TOL_SIGMA_MIN)
    ranks = host(rc.sketch_svd_rank_large_batched(tt(a64.astype(dtype)[None]), k, cases.TOL, 1, omega=tt(om64.astype(dtype))))[3]
    print(f"tolerance case {np.dtype(dtype).name}: rank {int(ranks[0])}")
    assert ranks[0] == cases.TOL_RANK == 22


# ---------------------------------------------------------------- 6. a zero block, and the refused step count
@pytest.mark.parametrize("dtype", TDTYPES)
def test_zero_block_beside_a_gaussian_one(dtype):
    rng = np.random.default_rng(26)
    m, n, l, k = 200, 600, 20, 12
    g = tt(rng.standard_normal((1, m, n))).to(dtype)
    om = tt(rng.standard_normal((l, m))).to(dtype)
    pair = torch.cat([torch.zeros_like(g), g])
    for its in (1, 2):
        alone = host(rc.sketch_svd_rank_large_batched(g, k, 0.0, its, omega=om))
        u, s, vt, ranks = host(rc.sketch_svd_rank_large_batched(pair, k, 0.0, its, omega=om))
        assert ranks[0] == 0 and ranks[1] == k
        for x in (u[0], s[0], vt[0]):
            assert np.all(np.isfinite(x)) and not np.any(x)
        for w, got in zip(alone, (u, s, vt, ranks)):
            assert same_bits(w[0], got[1])
    with pytest.raises(AssertionError, match="512"):
        rc.sketch_svd_rank_large_batched(pair, k, 0.0, 0, omega=om)
    with pytest.raises(AssertionError, match="min"):  # l = 20 > m = 10
        rc.sketch_range_step_large_batched(torch.zeros((1, 10, 600), dtype=dtype, device="cuda"), torch.zeros((20, 10), dtype=dtype, device="cuda"))
    with pytest.raises(TypeError):
        rc.sketch_svd_rank_large_batched(torch.zeros((1, 30, 600), dtype=torch.complex128, device="cuda"), 4)


# ---------------------------------------------------------------- 7. the C++ mirror
def test_cpp_example_runs(tmp_path):
    """tests/cpp/batched_sketch_product_example.cpp through include/rusty_compression.hpp: every check of the example passes."""
    exe = build_cpp_mirror_examples(tmp_path, "batched_sketch_product_example.cpp")
    res = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=dict(os.environ))
    print(res.stdout)
    assert res.returncode == 0 and "ALL OK" in res.stdout, res.stdout + res.stderr
