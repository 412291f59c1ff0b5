"""tests/scale_cases.py on the host: (a) LAPACK, standing in for the device, passes every family checker at every exponent and its
descaled results are the unit-scale ones bit for bit (so a failure of tests/test_gpu_batched_scales.py is the kernel's, not the
reference's or the bound's); (b) a model of the kernels before the normalisation, a pivoted Householder QR whose norms are plain sums
of squares in the working type, is rejected at the outer and at the edge exponents and accepted at 0 and at +-40 / +-300; (c) every
scaled input, every descaled expectation and ||A||_F 2^e are finite and normal in the working type, so the domain the header promises
is not vacuous.

The same three parts for the calls that consume those outputs (the last section): (a) the host recompression and a host residual with
?lassq's accumulation pass check_recompress / check_residual at every exponent and carrier; (b) a recompression whose singular values are
plain sums of squares in the working type is rejected at the outer exponents and at +62 / +510, a residual with plain f64 sums of squares
at -900, +510 and +900; (c) every operand, expectation and norm of those cases is finite and normal."""
import numpy as np
import pytest
import scipy.linalg

from oracle import ref_lapack as o
from tests import range_step_ref
from tests import scale_cases as sc

REAL = [np.float64, np.float32]
ALL = [np.float64, np.float32, np.complex128, np.complex64]
SHAPE, K = (96, 80), 40  # the matrix of the issue's own check: pivots of ?geqp3 identical at 2^+-90 (f32) and 2^+-900 (f64)
L = 24


def tol_of(dtype):
    return sc.TOLS[sc.real_of(dtype)]


# ------------------------------------------------------------------------------------------------ the oracle as the call under test
def oracle_column_id(x, k, tol):
    """The reference sequence QR::compute_from -> compress -> column_id in x's own precision, with the batched rank rule (k steps at most,
    the tolerance on |R_jj / R_00|): (c, z, ind, r) padded to k like the batched call's outputs."""
    full = o.QR.compute_from(x)
    d = np.abs(np.diag(full.r))
    kk = min(k, *x.shape)
    r = next((j for j in range(kk) if d[j] == 0 or d[j] / d[0] < tol), kk)
    cid = full.compress_qr_rank(r).column_id()
    c = np.zeros((x.shape[0], kk), dtype=x.dtype)
    z = np.zeros((kk, x.shape[1]), dtype=x.dtype)
    c[:, :r], z[:r] = x[:, full.ind[:r]], cid.z
    return c, z, full.ind, r


def oracle_two_sided(x, k, tol):
    full = o.QR.compute_from(x)
    d = np.abs(np.diag(full.r))
    kk = min(k, *x.shape)
    r = next((j for j in range(kk) if d[j] == 0 or d[j] / d[0] < tol), kk)
    ts = full.compress_qr_rank(r).column_id().two_sided_id()
    c = np.zeros((x.shape[0], kk), dtype=x.dtype)
    xx = np.zeros((kk, kk), dtype=x.dtype)
    rr = np.zeros((kk, x.shape[1]), dtype=x.dtype)
    c[:, :r], xx[:r, :r], rr[:r] = ts.c, x[ts.row_ind[:r]][:, ts.col_ind[:r]], ts.r
    return c, xx, rr, ts.row_ind, ts.col_ind, r


def oracle_svd(x, k, tol, dtype):
    """numpy.linalg.svd in x's own precision with the batched sign / phase rule and rank rule."""
    u, s, vh = np.linalg.svd(x, full_matrices=False)
    kk = min(k, len(s))
    r = next((j for j in range(kk) if s[j] == 0 or s[j] / s[0] < tol), kk)
    uo = np.zeros((x.shape[0], kk), dtype=x.dtype)
    vo = np.zeros((kk, x.shape[1]), dtype=x.dtype)
    for j in range(r):
        i = int(np.argmax(np.abs(u[:, j])))
        ph = np.conj(u[i, j]) / np.abs(u[i, j])
        col = u[:, j] * ph
        if sc.is_complex(dtype):
            col[i] = np.abs(u[i, j])  # the rule's entry is real and positive, imaginary part exactly 0
        uo[:, j], vo[j] = col, vh[j] * np.conj(ph)
    return uo, s, vo, r


@pytest.mark.parametrize("dtype", ALL)
def test_the_oracle_passes_the_column_id_checker_at_every_scale(dtype):
    units, cells, stacked = sc.batch(SHAPE, dtype)
    outs = [oracle_column_id(x, K, tol_of(dtype)) for x in stacked]
    for (i, e), (c, z, ind, r) in zip(cells, outs):
        assert r == (sc.exact_rank(SHAPE) if sc.KINDS[i] == "exact" else K)
        sc.check_column_id(units[i], e, c, z, ind, r, K, dtype, tol_of(dtype))
        u = outs[sc.unit_cell(cells, i)]
        sc.assert_same_as_unit(("c", "z", "ind", "ranks"), u, (sc.descale(c, e), z, ind, r), sc.id_stable_prefix(units[i], u[2], u[3], dtype))


@pytest.mark.parametrize("dtype", REAL)
def test_geqp3_is_equivariant_bit_for_bit(dtype):
    """The pivots and, after descaling, R of ?geqp3 on the 1e-3 matrix are the unit-scale ones at every exponent."""
    units, cells, stacked = sc.batch(SHAPE, dtype)
    q0, r0, ind0 = o.pivoted_qr(units[1])
    for (i, e), x in zip(cells, stacked):
        if i != 1:
            continue
        _, r, ind = o.pivoted_qr(x)
        assert np.array_equal(ind, ind0) and sc.same_bits(sc.descale(r, e), r0), e


@pytest.mark.parametrize("dtype", ALL)
def test_the_oracle_passes_the_two_sided_checker_at_every_scale(dtype):
    units, cells, stacked = sc.batch(SHAPE, dtype)
    for (i, e), x in zip(cells, stacked):
        c, xx, rr, row_ind, col_ind, r = oracle_two_sided(x, K, tol_of(dtype))
        sc.check_two_sided_id(units[i], e, c, xx, rr, row_ind, col_ind, r, K, dtype)


@pytest.mark.parametrize("dtype", ALL)
def test_the_oracle_passes_the_svd_checker_at_every_scale(dtype):
    shape = (60, 30)
    units, cells, stacked = sc.batch(shape, dtype)
    s_unit = {}
    for (i, e), x in zip(cells, stacked):
        u, s, vt, r = oracle_svd(x, 30, tol_of(dtype), dtype)
        assert r == (sc.exact_rank(shape) if sc.KINDS[i] == "exact" else 30)
        sc.check_svd(units[i], e, u, s, vt, r, 30, dtype)
        s_unit.setdefault(i, np.linalg.svd(units[i], compute_uv=False))
        # ?gesdd scales its input by a factor that is not a power of two: not bit for bit, but to a few ulps of s_0 (measured 1.2e-15 in f64)
        assert np.abs(sc.descale(s, e) - s_unit[i]).max() <= 8 * np.finfo(sc.real_of(dtype)).eps * s_unit[i][0]


@pytest.mark.parametrize("dtype", ALL)
def test_the_host_route_passes_the_sketched_id_checker_at_every_scale(dtype):
    m, n = SHAPE
    units, cells, stacked = sc.batch(SHAPE, dtype)
    om = sc.omega(SHAPE, L, dtype)
    for (i, e), x in zip(cells, stacked):
        y = om @ x  # the working type's own product: only x carries the scale
        c, z, ind, r = oracle_column_id(y, L, tol_of(dtype))
        cc = np.zeros((m, L), dtype=dtype)
        cc[:, :r] = x[:, ind[:r]]
        sc.check_sketch_id(units[i], om, e, cc, z, ind, r, y, L, dtype)


@pytest.mark.parametrize("dtype", REAL)
def test_the_host_model_passes_the_range_step_checker_at_every_scale(dtype):
    units, cells, stacked = sc.batch(SHAPE, dtype)
    om = sc.omega(SHAPE, L, dtype)
    for (i, e), x in zip(cells, stacked):
        y = om @ x
        q = scipy.linalg.qr(y.T, mode="economic", pivoting=True)[0].T
        assert q.dtype == np.dtype(dtype)
        sc.check_range_step(units[i], om, e, q, x @ q.T, L, y, dtype)
    q64, p64 = range_step_ref.range_step(units[1], om)  # the f64 model of the compositions spans the same rows
    assert np.linalg.norm(q64 @ q64.T - np.eye(L)) <= 1e-12 and p64.shape == (SHAPE[0], L)


# ------------------------------------------------------------------------------------------------ (b) the planted model
def unscaled_norm_column_id(x, k, tol):
    """The batched column ID as the kernels ran it before the normalisation, in x's own precision: a pivoted Householder QR whose column
    norms (the pivot search's and ?larfg's) are np.sum(v * v, dtype=dtype) without scaling, the rank rule on R_jj, Z by back
    substitution.  Returns (c, z, ind, r) padded to k."""
    dt = x.dtype
    w = np.array(x, copy=True)
    m, n = w.shape
    kk = min(k, m, n)
    ind = np.arange(n)
    taus = np.zeros(kk, dtype=dt)
    r = kk
    with np.errstate(all="ignore"):
        for j in range(kk):
            vn = np.sqrt(np.sum(w[j:, j:] * w[j:, j:], axis=0, dtype=dt))
            cand = np.where(np.isnan(vn), dt.type(-1), vn)
            p = j + int(np.argmax(cand))
            if p != j:
                w[:, [j, p]] = w[:, [p, j]]
                ind[[j, p]] = ind[[p, j]]
            alpha = w[j, j]
            xnorm = np.sqrt(np.sum(w[j + 1:, j] * w[j + 1:, j], dtype=dt))
            beta, tau = alpha, dt.type(0)
            if xnorm != 0:
                beta = -np.copysign(np.hypot(alpha, xnorm), alpha)
                w[j + 1:, j] *= dt.type(1) / (alpha - beta)
                tau = (beta - alpha) / beta
                w[j, j] = beta
            if beta == 0 or abs(beta / w[0, 0]) < tol:
                r = j
                break
            taus[j] = tau
            if tau != 0 and j + 1 < n:
                v = np.concatenate([[dt.type(1)], w[j + 1:, j]]).astype(dt)
                w[j:, j + 1:] -= np.outer(v, tau * (v @ w[j:, j + 1:]))
        z = np.zeros((kk, n), dtype=dt)
        if r > 0:
            z12 = np.array(w[:r, r:], copy=True)
            for i in range(r - 1, -1, -1):
                z12[i] = (z12[i] - w[i, i + 1:r] @ z12[i + 1:]) / w[i, i]
            z[:r, ind[:r]] = np.eye(r, dtype=dt)
            z[:r, ind[r:]] = z12
    c = np.zeros((m, kk), dtype=dt)
    c[:, :r] = x[:, ind[:r]]
    return c, z, ind, r


def verdict(a, e, out, unit_out, dtype):
    """The two assertions tests/test_gpu_batched_scales.py makes per matrix: None when both pass, else the AssertionError."""
    c, z, ind, r = out
    try:
        sc.check_column_id(a, e, c, z, ind, r, K, dtype, tol_of(dtype))
        sc.assert_same_as_unit(("c", "z", "ind", "ranks"), unit_out, (sc.descale(c, e), z, ind, r), sc.id_stable_prefix(a, unit_out[2], unit_out[3], dtype))
    except AssertionError as err:
        return err
    return None


@pytest.mark.parametrize("dtype", REAL)
def test_a_model_with_unscaled_norms_is_rejected_outside_the_central_exponents(dtype):
    units, cells, stacked = sc.batch(SHAPE, dtype)
    exps = sc.exponents(dtype)
    accepted = {exps[2], 0, exps[4]}  # 0 and +-40 / +-300
    outer = {exps[0], exps[-1]}
    outs = [unscaled_norm_column_id(x, K, tol_of(dtype)) for x in stacked]
    for (i, e), out in zip(cells, outs):
        err = verdict(units[i], e, out, outs[sc.unit_cell(cells, i)], dtype)
        if e in accepted:
            assert err is None, (sc.KINDS[i], e, err)
        elif e in outer or sc.KINDS[i] == "gaussian":
            # the edge exponents are placed by entries of order one, the Gaussian kind's: the squares of the 1e-3 kind's entries (about
            # 2^-5 at this shape) stay ten binades further inside and need not fail there
            assert err is not None, f"the model passed at {sc.KINDS[i]}, e = {e}: the checks would not have caught the unscaled norms"


# ------------------------------------------------------------------------------------------------ (c) the domain is not vacuous
@pytest.mark.parametrize("dtype", ALL)
@pytest.mark.parametrize("family", ["id", "svd", "sketch", "step"])
def test_inputs_expectations_and_norms_stay_in_the_normal_range(family, dtype):
    rd = sc.real_of(dtype)
    shapes = {"id": [s[:2] for s in sc.ID_SHAPES], "svd": sc.SVD_SHAPES, "sketch": [s[:2] for s in sc.SKETCH_SHAPES], "step": [s[:2] for s in sc.STEP_SHAPES]}[family]
    with np.errstate(over="raise"):
        for shape in shapes:
            units, cells, stacked = sc.batch(shape, dtype)
            assert stacked.dtype == np.dtype(dtype) and sc.in_normal_range(stacked, dtype)  # every scaled input
            for (i, e), x in zip(cells, stacked):
                assert sc.same_bits(sc.descale(x, e), units[i])  # the scaling lost nothing: 2^e a is exact
            for i, a in enumerate(units):
                s = np.linalg.svd(a.astype(np.complex128 if sc.is_complex(dtype) else np.float64), compute_uv=False)
                kept = s[s > 1e-6 * s[0]]  # the singular values a call keeps (the exact kind's tail is rounding noise that the tolerance cuts)
                fro = float(np.linalg.norm(a.astype(np.complex128)))
                for e in (min(sc.exponents(dtype)), max(sc.exponents(dtype))):
                    for v in (fro, float(kept[0]), float(kept[-1])):  # ||A||_F 2^e and the extreme expected singular values
                        w = np.ldexp(rd.type(v), e)
                        assert np.isfinite(w) and abs(w) >= np.finfo(rd).tiny, (shape, sc.KINDS[i], e, v)


# ------------------------------------------------------------------------------------------------ recompression and residual norms
RC_SHAPE = (96, 80, 24)


def recompress_verdicts(dtype, carrier, plain_norms):
    """{(kind, e): None or the AssertionError} of the host route (or the planted model) on every cell of the carrier's batch."""
    m, n, K = RC_SHAPE
    units, cells, (left, right, mid, s), refs = sc.recompress_batch(RC_SHAPE, dtype, carrier)
    pick = lambda x, idx: None if x is None else x[idx]  # noqa: E731
    outs = [sc.host_recompress(left[idx], right[idx], pick(mid, idx), pick(s, idx), dtype, plain_norms) for idx in range(len(cells))]
    verdicts = {}
    for idx, (i, e) in enumerate(cells):
        u, s_out, vt, r = outs[idx]
        u0, s0, vt0, r0 = outs[sc.unit_cell(cells, i)]
        try:
            sc.check_recompress(refs[i], carrier, e, u, s_out, vt, r, K, dtype, (u0, s0, vt0, r0))
            verdicts[(sc.recompress_kinds(carrier, dtype)[i], e)] = None
        except AssertionError as err:
            verdicts[(sc.recompress_kinds(carrier, dtype)[i], e)] = err
    return verdicts


@pytest.mark.parametrize("dtype", ALL)
@pytest.mark.parametrize("carrier", list(sc.CARRIERS))
def test_the_host_route_passes_the_recompression_checker_at_every_scale(carrier, dtype):
    failed = {k: str(v)[:120] for k, v in recompress_verdicts(dtype, carrier, False).items() if v is not None}
    assert not failed, failed


@pytest.mark.parametrize("dtype", ALL)
@pytest.mark.parametrize("carrier", list(sc.CARRIERS))
def test_a_recompression_with_plain_sums_of_squares_is_rejected_outside_the_central_exponents(carrier, dtype):
    """The planted model is accepted at 0 and +-40 / +-300 and, for the carriers whose product carries 2^e, rejected at the outer
    exponents and at +62 / +510 (the split carrier's product is at unit scale: it passes this model by construction, its job is a kernel
    that normalises some operands only)."""
    exps = sc.exponents(dtype)
    accepted, outer, edge = {exps[2], 0, exps[4]}, {exps[0], exps[6]}, exps[5]
    for (kind, e), err in recompress_verdicts(dtype, carrier, True).items():
        if e in accepted or carrier == "split":
            assert err is None, (kind, e, err)
        elif e in outer or (e == edge and kind == "gauss"):
            # the edge exponent is placed by a core of norm well above one, the Gaussian kind's: the spectrum kind's largest singular value
            # is 1, its squares reach 2^1020 (2^124) at most and need not fail there
            assert err is not None, f"the model passed at {kind}, e = {e}: the checks would not have caught the plain sums of squares"


def host_residual(x, K, dtype, plain_sums):
    """(err, nrm, e) of one entry x = dict(a, left, right, mid, s) as given (scaled): the rebuild in the wide type, e rounded to the working
    type, and the two norms by ?lassq's accumulation (sc.lassq_norm) or, plain_sums, by np.sum(v * v) in f64: the kernels' former sums."""
    wide = np.complex128 if sc.is_complex(dtype) else np.float64
    rd = sc.real_of(dtype)
    w = x["right"].astype(wide)[:K]
    if x["s"] is not None:
        w = x["s"].astype(np.float64)[:K, None] * w
    if x["mid"] is not None:
        w = x["mid"].astype(wide)[:K, :K] @ w
    e = (x["a"].astype(wide) - x["left"].astype(wide)[:, :K] @ w).astype(dtype)
    if plain_sums:
        with np.errstate(all="ignore"):
            norm = lambda v: np.sqrt(np.sum((v.astype(wide) * v.astype(wide).conj()).real))  # noqa: E731
            return rd.type(norm(e)), rd.type(norm(x["a"])), e
    return rd.type(sc.lassq_norm(e)), rd.type(sc.lassq_norm(x["a"])), e


def residual_verdicts(dtype, mode, plain_sums):
    m, n, K = sc.RESIDUAL_SHAPES[0]
    units, cells, stacked = sc.residual_batch(sc.RESIDUAL_SHAPES[0], dtype, mode)
    outs = [host_residual({k: None if v is None else v[idx] for k, v in stacked.items()}, K, dtype, plain_sums) for idx in range(len(cells))]
    verdicts = {}
    for idx, (i, e) in enumerate(cells):
        err, nrm, eo = outs[idx]
        try:
            sc.check_residual(units[i], e, err, nrm, eo, outs[sc.unit_cell(cells, i)][2], dtype)
            verdicts[(sc.RESIDUAL_KINDS[i], e)] = None
        except AssertionError as exc:
            verdicts[(sc.RESIDUAL_KINDS[i], e)] = exc
    return verdicts


@pytest.mark.parametrize("dtype", ALL)
@pytest.mark.parametrize("mode", list(sc.RESIDUAL_CARRIER))
def test_the_host_residual_passes_the_residual_checker_at_every_scale(mode, dtype):
    failed = {k: str(v)[:120] for k, v in residual_verdicts(dtype, mode, False).items() if v is not None}
    assert not failed, failed


@pytest.mark.parametrize("dtype", ALL)
@pytest.mark.parametrize("mode", list(sc.RESIDUAL_CARRIER))
def test_a_residual_with_plain_sums_of_squares_is_rejected_where_f64_squares_leave_the_range(mode, dtype):
    """f64 / c64: rejected at -900, +510 and +900 (the plain sums give 0, inf and inf), accepted at 0 and +-300.  f32 / c32: the squares
    are taken in f64 and stay in range, so the plain sums pass everywhere; the GPU test pins that the kernels' single accumulator does."""
    wide = sc.real_of(dtype) == np.dtype(np.float64)
    for (kind, e), err in residual_verdicts(dtype, mode, True).items():
        if wide and e in (-900, 510, 900):
            assert err is not None, f"the model passed at {kind}, e = {e}"
        elif not wide or e in (-300, 0, 300):
            assert err is None, (kind, e, err)


@pytest.mark.parametrize("dtype", ALL)
def test_recompression_and_residual_cases_stay_in_the_normal_range(dtype):
    rd = sc.real_of(dtype)
    lo, hi = min(sc.exponents(dtype)), max(sc.exponents(dtype))
    with np.errstate(over="raise"):
        for shape in [RC_SHAPE] + [sh for fam in sc.RECOMPRESS_SHAPES.values() for sh in fam]:
            for carrier in sc.CARRIERS:
                units, cells, operands, refs = sc.recompress_batch(shape, dtype, carrier)
                for x in operands:
                    assert x is None or sc.in_normal_range(x, dtype), (shape, carrier)
                for idx, (i, e) in enumerate(cells):
                    for x, x0 in zip(sc.carry(tuple(None if y is None else y[idx] for y in operands), carrier, -e), units[i]):
                        assert x0 is None or sc.same_bits(x, x0)  # the scaling lost nothing
                for i, (a, sigma, ref) in enumerate(refs):
                    kept = ref.s[:shape[2]]
                    for e in (lo, hi):
                        for v in (float(np.linalg.norm(a)), float(kept[0]), float(kept[-1])):
                            w = np.ldexp(rd.type(v), sc.net_exponent(carrier, e))
                            assert np.isfinite(w) and abs(w) >= np.finfo(rd).tiny, (shape, carrier, i, e, v)
        for shape in sc.RESIDUAL_SHAPES:
            for mode in sc.RESIDUAL_CARRIER:
                units, cells, stacked = sc.residual_batch(shape, dtype, mode)
                for x in stacked.values():
                    assert x is None or sc.in_normal_range(x, dtype), (shape, mode)
                ref = sc.rrc if sc.is_complex(dtype) else sc.rr
                for i, f in enumerate(units):
                    _, e_ref = ref.reference(f["a"], f["left"], f["right"], f["mid"], f["s"], shape[2])
                    for e in (lo, hi):
                        for v in (float(np.linalg.norm(f["a"].astype(np.complex128))), float(np.linalg.norm(e_ref))):
                            w = np.ldexp(rd.type(v), e)
                            assert np.isfinite(w) and abs(w) >= np.finfo(rd).tiny, (shape, mode, i, e, v)
