"""tests/dense_scale_cases.py on the host, with the oracle (SciPy LAPACK) in place of the device: the inputs carry the properties that
tests/test_gpu_dense_scales.py relies on, so a failure there is the library's and not the reference's, the bound's or the data's.

(a) LAPACK passes every tolerance checker at every exponent, kind, shape and dtype of the tables.
(b) For the two kinds compared bit for bit, every input and every oracle output that carries the scale (R, L, s), descaled and scaled,
    is finite and zero or normal at every exponent: no cell of these kinds may be excused from the comparison on the device.
(c) ?geqp3 is scale-equivariant bit for bit: pivots, Q and descaled R equal the unit cell's.  ?gesdd is not (it rescales by a factor
    that is no power of two), so here the SVD is held to the bounds only; the device normalises by a power of two and is held to bits.
(d) A pivoted QR whose norms are plain sums of squares in the working type fails the pivot or R check at the four outer and edge
    exponents of each type."""
import numpy as np
import pytest

from oracle import ref_lapack as o
from tests import dense_scale_cases as dc
from tests import scale_cases as sc

ALL = dc.REAL + dc.COMPLEX
QR_SHAPES = {np.dtype(dt): sorted({(v[0], v[1]) for v in dc.QR_ROUTES.values()}) for dt in dc.REAL}
QR_SHAPES.update({np.dtype(dt): [(s, min(s)) for s in dc.COMPLEX_QR_SHAPES] for dt in dc.COMPLEX})
LQ_SHAPES = {np.dtype(dt): sorted({v[0] for v in dc.LQ_ROUTES.values()}) for dt in dc.REAL}
LQ_SHAPES.update({np.dtype(dt): dc.COMPLEX_QR_SHAPES for dt in dc.COMPLEX})


def every_cell(shape, dtype, check):
    """check(a, kind index, e) on the 21 cells of a shape; the failing (kind, e) cells in one message."""
    units, cells = dc.cases(shape, dtype)
    failed = []
    for i, e in cells:
        try:
            check(units[i], i, e)
        except AssertionError as err:
            failed.append((dc.KINDS[i], e, dc.where(err)))
    assert not failed, f"{shape}: {len(failed)} of {len(cells)} cells failed: {failed}"


def bitwise(i):
    return dc.KINDS[i] in dc.BITWISE_KINDS


@pytest.mark.parametrize("dtype", ALL)
def test_the_oracle_passes_the_qr_checkers_and_is_equivariant_bit_for_bit(dtype):
    for shape, k in QR_SHAPES[np.dtype(dtype)]:
        unit = {}

        def check(a, i, e):
            x = sc.scale(a, e)
            q, r, ind = o.pivoted_qr(x)
            dc.check_qr(a, e, q[:, :k], r[:k], ind, k)
            if bitwise(i):
                assert sc.in_normal_range(x, dtype) and sc.in_normal_range(r, dtype) and sc.in_normal_range(sc.descale(r, e), dtype)
                u = unit.setdefault(i, (q, r, ind))  # (the unit cell of a kind comes first)
                dc.assert_same_as_unit(("ind", "q", "r"), (u[2], u[0], u[1]), (ind, q, sc.descale(r, e)))

        every_cell(shape, dtype, check)


@pytest.mark.parametrize("dtype", ALL)
def test_the_oracle_passes_the_lq_checker_and_is_equivariant_bit_for_bit(dtype):
    for shape in LQ_SHAPES[np.dtype(dtype)]:
        unit = {}

        def check(a, i, e):
            x = sc.scale(a, e)
            l, q, ind = o.pivoted_lq(x)
            dc.check_lq(a, e, l, q, ind)
            if bitwise(i):
                assert sc.in_normal_range(l, dtype) and sc.in_normal_range(sc.descale(l, e), dtype)
                u = unit.setdefault(i, (l, q, ind))
                dc.assert_same_as_unit(("ind", "q", "l"), (u[2], u[1], u[0]), (ind, q, sc.descale(l, e)))

        every_cell(shape, dtype, check)


@pytest.mark.parametrize("dtype", ALL)
def test_the_oracle_passes_the_geqp3_checker_and_is_equivariant_bit_for_bit(dtype):
    shapes = sorted({v[0] for v in dc.GEQP3_ROUTES.values()}) if not sc.is_complex(dtype) else dc.COMPLEX_QR_SHAPES
    for shape in shapes:
        unit = {}
        k = min(shape)

        def check(a, i, e):
            f, jp, tau = o.geqp3_raw(sc.scale(a, e))
            q = o.orgqr_raw(f, tau)
            dc.check_geqp3_at(a, e, f, jp, tau, q)
            if bitwise(i):
                f1 = dc.descale_geqp3(f, e, k)
                assert sc.in_normal_range(np.triu(f[:k]), dtype) and sc.in_normal_range(np.triu(f1[:k]), dtype)
                u = unit.setdefault(i, (f, jp, tau, q))
                dc.assert_same_as_unit(("jpvt", "f", "tau", "q"), (u[1], u[0], u[2], u[3]), (jp, f1, tau, q))

        every_cell(shape, dtype, check)


@pytest.mark.parametrize("dtype", ALL)
def test_the_oracle_passes_the_svd_checker_at_every_scale(dtype):
    for shape, _ in dc.svd_routes(dtype).values():
        def check(a, i, e):
            u, s, vt = o.compute_svd(sc.scale(a, e))
            dc.check_svd(a, e, u, s, vt)
            if bitwise(i):
                assert sc.in_normal_range(s, dtype) and sc.in_normal_range(sc.descale(s, e), dtype)

        every_cell(shape, dtype, check)


@pytest.mark.parametrize("dtype", ALL)
def test_the_norms_of_every_cell_are_in_the_normal_range(dtype):
    """rc_max_col_norm_* of 2^e a is ldexp(unit, e) and stays normal; rel_diff_fro's operands are a and a perturbed copy of it."""
    rd = sc.real_of(dtype)
    for shape in [(60, 40), (1024, 33)]:
        def check(a, i, e):
            nrm = rd.type(o.max_col_norm(a))
            assert sc.in_normal_range(np.ldexp(nrm, e), rd) and sc.in_normal_range(sc.scale(dc.perturbed(a), e), dtype)

        every_cell(shape, dtype, check)


@pytest.mark.parametrize("dtype", dc.REAL)
def test_a_qr_with_unscaled_norms_is_rejected_at_the_outer_and_edge_exponents(dtype):
    """The model of the kernels before the normalisation on the per-step shape: accepted at 0, rejected at the two outer exponents
    (every norm 0 or inf) and at the two edge ones (squares that go subnormal or overflow), by the pivot or the R check."""
    shape, k = dc.QR_ROUTES["per-step"][:2]
    units, cells = dc.cases(shape, dtype)
    es = sc.exponents(dtype)
    for i, kind in enumerate(dc.KINDS):
        if kind not in dc.BITWISE_KINDS:
            continue
        a = units[i]
        ind0 = o.pivoted_qr(a)[2]
        r0 = dc.unscaled_norm_qr(a)[0]

        def verdict(e):
            """The pivots are ?geqp3's and the descaled R is the model's own unit-scale R, bit for bit."""
            r, ind = dc.unscaled_norm_qr(sc.scale(a, e))
            return np.array_equal(ind, ind0) and sc.same_bits(sc.descale(r, e), r0)

        assert verdict(0) and dc.rel(np.abs(r0), np.abs(o.pivoted_qr(a)[1])) <= dc.TOL[np.dtype(dtype)]["factor"], kind
        # (the squared column norms of the decay kind are at most sigma_max^2 = 1: times 4^62 or 4^510 they stay inside the range, so its
        # upper edge is no edge for plain sums; the Gaussian kind's are about m)
        for e in (es[0], es[1], es[-2], es[-1]) if kind == "gaussian" else (es[0], es[1], es[-1]):
            assert not verdict(e), (kind, e)
