"""CPU tests of tests/permutation_ref.py, the host model the GPU index-contract tests are judged by.

For valid permutations the model is the oracle (oracle/ref_lapack.py, the reference's src/permutation.rs) and reproduces the reference's
known answers; for the two inputs that are no permutations it gives answers written out by hand here.  The last test shows that the
backward-error bound the GPU test applies to the Z solve is one a plain working-precision back substitution meets at every shape."""
import numpy as np
import pytest
import scipy.linalg

from oracle import ref_lapack as o
from tests import permutation_ref as pr
from tests.helpers import golden

ID_K = (1, 15, 16, 17, 33, 128)
ID_SHAPES = sorted({(k, n) for k in ID_K for n in (k + 1, 255, 256, 257, 513) if k < n}) + [(12, 12)]
ID_SHAPES_COMPLEX = [(1, 2), (16, 257), (33, 513)]


@pytest.mark.parametrize("dtype", [np.float64, np.float32, np.complex128, np.complex64])
@pytest.mark.parametrize("shape", [(37, 53), (1, 1), (5, 2)])
def test_model_equals_the_oracle_for_valid_permutations(shape, dtype):
    rng = np.random.default_rng(11)
    mat = (rng.standard_normal(shape) + (1j * rng.standard_normal(shape) if np.dtype(dtype).kind == "c" else 0)).astype(dtype)
    for mode in pr.MODES:
        perm = rng.permutation(shape[1] if mode.startswith("COL") else shape[0])
        out, rejected = pr.apply_matrix_unique(mat, perm, mode)
        assert not rejected and out.dtype == mat.dtype
        assert np.array_equal(out, o.apply_permutation_matrix(mat, perm, mode)), mode
    vec = mat[:, 0].copy()
    perm = rng.permutation(shape[0])
    for mode in pr.VMODES:
        choices, rejected = pr.apply_vector(vec, perm, mode)
        assert not rejected
        assert np.array_equal(np.array([c[0][0] for c in choices]), o.apply_permutation_vector(vec, perm, mode)), mode
    adm = pr.checked_invert(perm, shape[0])
    assert np.array_equal(pr.any_inverse(adm), o.invert_permutation_vector(perm))


def test_model_reproduces_the_known_answers_of_the_reference():
    g = golden("perm_known.npz")
    for mode in pr.MODES:
        out, rejected = pr.apply_matrix_unique(g["mat"], g["perm"], mode)
        assert not rejected and np.array_equal(out, g[mode]), mode
    for mode in pr.VMODES:
        choices, rejected = pr.apply_vector(g["vec"], g["perm"], mode)
        assert not rejected and np.array_equal(np.array([c[0][0] for c in choices]), g[mode]), mode
    assert np.array_equal(pr.any_inverse(pr.checked_invert(g["perm"], 3)), np.array([1, 2, 0]))


def test_a_duplicated_entry_by_hand():
    src = np.array([[1.0, 2.0, 3.0], [4.0, 5.0, 6.0]])
    perm = [2, 2, 0]
    # a gather repeats the column and rejects nothing
    out, rejected = pr.checked_gather(src, perm)
    assert not rejected and np.array_equal(out, np.array([[3.0, 3.0, 1.0], [6.0, 6.0, 4.0]]))
    # the inverse: 0 is named by position 2, 1 by nobody, 2 by positions 0 and 1 (either may win on the device)
    adm = pr.checked_invert(perm, 3)
    assert adm == [(2,), (), (0, 1)]
    assert np.array_equal(pr.any_inverse(adm), np.array([2, -1, 0]))
    assert pr.inverse_admissible(np.array([2, -1, 0]), adm).all() and pr.inverse_admissible(np.array([2, -1, 1]), adm).all()
    assert not pr.inverse_admissible(np.array([2, 0, 1]), adm)[1] and not pr.inverse_admissible(np.array([2, -1, 2]), adm)[2]
    # COLINV: out[:, 0] = src[:, 2], out[:, 1] = 0 (bit 32), out[:, 2] = src[:, 0] or src[:, 1]
    choices, rejected = pr.apply_matrix(src, perm, "COLINV")
    assert rejected
    assert pr.admissible(np.array([[3.0, 0.0, 1.0], [6.0, 0.0, 4.0]]), choices).all()
    assert pr.admissible(np.array([[3.0, 0.0, 2.0], [6.0, 0.0, 5.0]]), choices).all()
    assert pr.admissible(np.array([[3.0, 2.0, 3.0], [6.0, 5.0, 6.0]]), choices).tolist() == [True, False, False]
    # ROWINV of the transpose is the same statement about rows
    choices_r, rejected_r = pr.apply_matrix(src.T, perm, "ROWINV")
    assert rejected_r and all(np.array_equal(a, b) for ca, cb in zip(choices, choices_r) for a, b in zip(ca, cb))


def test_out_of_range_entries_by_hand():
    src = np.array([[1.0, 2.0, 3.0], [4.0, 5.0, 6.0]])
    perm = [0, 5, -1]
    out, rejected = pr.checked_gather(src, perm)
    assert rejected and np.array_equal(out, np.array([[1.0, 0.0, 0.0], [4.0, 0.0, 0.0]]))
    adm = pr.checked_invert(perm, 3)
    assert adm == [(0,), (), ()]
    assert np.array_equal(pr.any_inverse(adm), np.array([0, -1, -1]))
    out, rejected = pr.apply_matrix_unique(src, perm, "COLINV")
    assert rejected and np.array_equal(out, np.array([[1.0, 0.0, 0.0], [4.0, 0.0, 0.0]]))
    out, rejected = pr.apply_matrix_unique(src.T, perm, "ROW")
    assert rejected and np.array_equal(out, np.array([[1.0, 4.0], [0.0, 0.0], [0.0, 0.0]]))
    # indices far outside int32 are entries like any other
    out, rejected = pr.checked_gather(src, np.array([-2 ** 63, 2 ** 40, 2 ** 62], dtype=np.int64))
    assert rejected and not out.any()
    assert pr.checked_invert(np.array([-2 ** 63, 2 ** 40, 2 ** 62], dtype=np.int64), 3) == [(), (), ()]


def test_vectorised_inverse_equals_the_model():
    rng = np.random.default_rng(3)
    for n in (1, 2, 7, 300):
        perm = rng.permutation(n).astype(np.int64)
        for bad in (None, -1, n, n + 1, 2 ** 62):
            p = perm.copy()
            if bad is not None:
                p[n // 2] = bad
            assert np.array_equal(pr.checked_invert_unique(p, n), pr.any_inverse(pr.checked_invert(p, n)))
    with pytest.raises(AssertionError):
        pr.checked_invert_unique([2, 2, 0], 3)


@pytest.mark.parametrize("dtype", [np.float64, np.float32, np.complex128, np.complex64])
def test_id_factors_are_diagonally_dominant_and_the_reference_solve_meets_the_bound(dtype):
    """The factors the GPU test feeds k_id_z, and the bound it asserts: a back substitution in the working precision (LAPACK ?trtrs
    through SciPy) must itself stay below rho_factor() * gamma_k at every shape before the kernel is held to it."""
    shapes = ID_SHAPES_COMPLEX if np.dtype(dtype).kind == "c" else ID_SHAPES
    worst = 0.0
    for k, n in shapes:
        rng = np.random.default_rng(1000 * k + n)
        q, r = pr.id_factors(rng, 24, k, n, dtype)
        assert q.shape == (24, k) and r.shape == (k, n) and r.dtype == np.dtype(dtype)
        r11 = r[:, :k]
        assert not np.tril(r11, -1).any()
        d = np.abs(np.diag(r11)).astype(np.float64)
        assert (d >= 1 - 1e-6).all() and (d <= 2 + 1e-6).all()
        assert ((np.abs(r11).astype(np.float64).sum(axis=1) - d) < 0.5).all()  # strictly dominant by rows, with room
        assert np.linalg.cond(r11.astype(np.complex128)) < 8
        if k == n:
            continue
        z12 = scipy.linalg.solve_triangular(r11, r[:, k:], lower=False, check_finite=False)
        assert z12.dtype == np.dtype(dtype)
        rho = pr.backward_error(r11, z12, r[:, k:], pr.wide_type(dtype))
        ratio = rho / pr.gamma(k, dtype)
        worst = max(worst, ratio)
        assert ratio <= pr.rho_factor(), (k, n, rho, pr.gamma(k, dtype))
    print(f"{np.dtype(dtype).name}: largest rho / gamma_k of the LAPACK solve {worst:.3f}")


def test_backward_error_sees_a_wrong_solve():
    rng = np.random.default_rng(5)
    _, r = pr.id_factors(rng, 24, 17, 40, np.float64)
    z = scipy.linalg.solve_triangular(r[:, :17], r[:, 17:], lower=False)
    assert pr.backward_error(r[:, :17], z, r[:, 17:], np.longdouble) <= 2 * pr.gamma(17, np.float64)
    z[16, 3] *= 1 + 1e-12  # a handful of ulps in one entry
    assert pr.backward_error(r[:, :17], z, r[:, 17:], np.longdouble) > 2 * pr.gamma(17, np.float64)
