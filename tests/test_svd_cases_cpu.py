"""tests/svd_cases.py on the host: LAPACK, standing in for the GPU call, meets every bound of check_svd on every input that
tests/test_gpu_svd_routes.py sends to the GPU (so a failure there is the kernel's, not the reference's or the bound's), the route
table restated from the sources gives the edges the GPU file is written around, and check_svd rejects planted faults."""
import numpy as np
import pytest

from tests import svd_cases as sc

DTYPES = [np.float64, np.float32]


def lapack(a):
    """numpy.linalg.svd of the f32 / f64 array itself (?gesdd in the array's own precision)."""
    u, s, vt = np.linalg.svd(a, full_matrices=False)
    assert u.dtype == a.dtype
    return u, s, vt


def test_bounds_are_the_ones_of_the_existing_route_tests():
    assert sc.BOUNDS == {np.dtype(np.float64): dict(sval=1e-12, orth=1e-12, recon=1e-12),
                         np.dtype(np.float32): dict(sval=2e-5, orth=1e-4, recon=5e-5)}
    assert sc.SCALES == (1.0, 2.0 ** -10, 2.0 ** -16)


def test_route_table_edges():
    """The edges of the core-size table, derived from the restated formulas of jacobi_lds.hpp."""
    assert sc.last_lds_core(np.float64) == 141 and sc.jacobi_pitch(141, np.float64) == 141  # (pitch n | 1: the padded one is too large)
    assert sc.jacobi_pitch(128, np.float64) == 144 and sc.jacobi_pitch(129, np.float64) == 144 and sc.jacobi_pitch(139, np.float64) == 139
    assert sc.last_lds_core(np.float32) == 192 and sc.jacobi_pitch(192, np.float32) == 208
    assert sc.core_is_fused(128) and not sc.core_is_fused(129)
    for dt in DTYPES:
        sizes = sc.CORE_SIZES[np.dtype(dt)]
        last = sc.last_lds_core(dt)
        assert {128, 129, last, last + 1, last + 2} <= set(sizes)
    # the CholeskyQR2 reduction needs the r x r QRCP image in LDS: in f64 the first global core (142) is beyond it
    assert sc.tsqr_supported(1024, 129, np.float64) and not sc.tsqr_supported(1024, 142, np.float64)
    assert sc.tsqr_supported(1024, 193, np.float32) and not sc.tsqr_supported(1023, 64, np.float32)


@pytest.mark.parametrize("dtype", DTYPES)
def test_lapack_meets_every_bound_on_the_route_cases(dtype):
    cases = sc.route_cases(dtype)
    assert len({sc.case_id(c) for c in cases}) == len(cases)
    for case in cases:
        shape, gen, scale = case
        a = sc.make_case(shape, gen, scale, dtype)
        assert a.dtype == dtype and a.shape == shape
        sc.check_svd(a, *lapack(a), dtype)
        if gen == "exact_zeros":
            s = np.linalg.svd(a.astype(np.float64), compute_uv=False)
            rank = sc.exact_zeros_rank(*shape)
            assert np.all(s[:rank] > 1e-3) and np.all(s[rank:] <= 1e-13 * s[0])
        if gen == "low_rank":
            s = np.linalg.svd(a.astype(np.float64), compute_uv=False)
            rho = sc.low_rank_rho(*shape)
            assert s[rho] <= 1e-5 * s[0] and s[rho - 1] > 1e-2 * s[0], "numerically rank deficient after the cast"
            if dtype == np.float32:
                assert s[0] * s[0] * np.finfo(np.float32).eps ** 2 > 2.0 ** -105  # (squared noise norms stay normal f32 numbers)


@pytest.mark.parametrize("dtype", DTYPES)
def test_lapack_meets_every_bound_on_clustered_and_graded_spectra(dtype):
    for r in sc.reduction_sizes(dtype):
        fam = sc.clustered(r, r, dtype)
        assert len(fam) == 3
        for name, a in fam.items():
            assert a.dtype == dtype
            sc.check_svd(a, *lapack(a), dtype)
            s = np.linalg.svd(a.astype(np.float64), compute_uv=False)
            if name != "all equal":  # the perturbation survived the cast
                assert s[0] - s[-1] > 10 * np.finfo(dtype).eps
    for n in sc.GRADED_SIZES[np.dtype(dtype)]:
        a = sc.graded(n, dtype)
        sc.check_svd(a, *lapack(a), dtype)


@pytest.mark.parametrize("dtype", [np.float64, np.float32, np.complex128, np.complex64])
def test_batched_cases_are_what_they_say(dtype):
    for m, n in sc.BATCHED_SHAPES:
        a = sc.batched_case(m, n, dtype)
        assert a.shape == (5, m, n) and a.dtype == dtype
        rho = sc.low_rank_rho(m, n)
        for i in range(5):
            s = np.linalg.svd(a[i].astype(np.complex128 if a.dtype.kind == "c" else np.float64), compute_uv=False)
            if i in (1, 3):
                assert s[rho] <= 1e-5 * s[0] and s[0] < 1.0  # (scaled down: a Gaussian's sigma_0 here is above 10)
            else:
                assert s[-1] > 1e-4 * s[0]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("fault", ["cosine", "swapped", "zero column", "scaled row"])
def test_check_svd_rejects_planted_faults(dtype, fault):
    a = sc.gaussian(40, 24, dtype)
    u, s, vt = (x.astype(np.float64) for x in np.linalg.svd(a.astype(np.float64), full_matrices=False))
    sc.check_svd(a, u, s, vt, dtype)
    if fault == "cosine":  # the last two columns of U get the cosine 1e-2
        u[:, -1] += 1e-2 * u[:, -2]
        u[:, -1] /= np.linalg.norm(u[:, -1])
        what = "orth U"
    elif fault == "swapped":
        s[[3, 4]] = s[[4, 3]]
        what = "not descending"
    elif fault == "zero column":
        u[:, 5] = 0
        what = "orth U"
    else:
        vt[7] *= 1 + 1e-3
        what = "orth V"
    got = {}
    with pytest.raises(AssertionError, match=what):
        sc.check_svd(a, u, s, vt, dtype, measured=got)
    if what.startswith("orth"):
        assert max(got["orth_u"], got["orth_v"]) > 1e-3  # (the figures reach the caller although the check failed)
