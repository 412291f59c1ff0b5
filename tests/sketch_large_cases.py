"""The accuracy cases of the batched randomized SVD of wide blocks (batch.sketch_svd_rank_large_batched), shared by
test_abi_batched_sketch_product_cpu.py (the conditions on the host model) and test_gpu_batched_sketch_svd_large.py (the device against
it).  The host model is tests/range_step_ref.py as it is: the large chain computes what sketch_svd_rank_power_batched computes, with the
row basis from an SVD-based orthonormalisation instead of a pivoted QR, which spans the same rows."""
import numpy as np

from tests import range_step_ref as ref

# (m, n, l, k): wide, very wide with a short left side, and tall with n just above the one-launch step's 512 columns
CASES = [(600, 700, 40, 32), (130, 1100, 24, 16), (700, 600, 40, 32)]
# the tolerance example: spectrum 1 .. 1e-12 over 130 values, l = k = 40, tol = 1e-2
TOL_CASE = (130, 1100, 40, 40)
TOL_SIGMA_MIN = 1e-12
TOL = 1e-2
TOL_RANK = 22

_MADE = {}


def block_and_omega(case, sigma_min=1e-10):
    """The f64 block and test matrix of a case (made once): ref.decaying(m + n, m, n) and ref.gaussian(7 m + n, l, m)."""
    key = (case, sigma_min)
    if key not in _MADE:
        m, n, l, _ = case
        _MADE[key] = (ref.decaying(m + n, m, n, sigma_min), ref.gaussian(7 * m + n, l, m))
    return _MADE[key]


def model_singular_ratios(a, om, steps):
    """s_j / s_0 of the model's P Q after `steps` range steps (what the chain's last call truncates by)."""
    q, p = ref.range_step(a, ref.power_omega(a, om, steps - 1))
    s = np.linalg.svd(p @ q, compute_uv=False)
    return s / s[0]
