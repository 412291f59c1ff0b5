// The host code the dense real API (rc_api.hip: f64 / f32) and the dense complex API (rc_complex.hip: c64 / c32) have in common, written once
// over the element type E (double, float, cplx<double>, cplx<float>); real_t<E> (rc_batched.hpp) is the type of norms and tolerances.  Host templates only:
// no kernel stands here, and nothing here is exported.  Each of the two files includes this header AFTER its own primitives, inside its
// `using namespace rc`, and expands RC_DEFINE_DENSE_SHARED for its two suffixes.
//
// What stands here once: the operator the range finders sample (OpView), the three range finders with orth_full, compute_from_range_estimate
// of the pivoted QR, rank_by_tolerance, apply_perm_matrix, and the C entry points whose bodies read the same for all four types.
//
// The primitives it is written in, one spelling per family (overloads on the element type, found in the including file):
//   tmp_colmajor<E>, tmp_omega<E>   temporaries in the family's layouts.  Real: column-major with an even leading dimension; Omega and the
//                                   accumulated projection row-major (that selects the GEMM arm).  Complex: everything column-major with
//                                   ld = max(rows, 1) (k_c_split reads coalesced only that way).  Callbacks see these views.
//   product(c, alpha, adj_a, a, b, beta, cm)   cm = alpha op(a) b + beta cm, op = adjoint when adj_a
//   qrcp(c, w, k, q, r, ind)        k steps of the pivoted QR of w, which it may destroy; q and r may be empty
//   fill_gaussian, copy_mat (complex: with a conjugate flag), gather_cols, max_col_norm_dev, invert_perm, read_back (rc_common.hpp)
#pragma once
#include <algorithm>
#include <cmath>
#include <string>
#include <type_traits>
#include <vector>

#include "rc_common.hpp"
#include "rc_cplx.hpp"

namespace {

// The operator the range finders sample: the reference implements them for ANY `Op: MatMat` / `Op: ConjMatMat`
// (/root/reference/src/random_sampling.rs:102, :130, :222; trait contract src/types.rs:40-51, :77-81, products :58-71, :88-101; all four
// scalar types: src/random_sampling.rs:123-126, :165-168, :277-280).  Either a dense device matrix (one product of the family per call) or
// the host's callback table (rc_operator, the rc_*_op_* entry points; complex views are interleaved rc_matrix descriptors with strides in
// complex elements): the compositions below are written once against these three products.
template <typename E>
struct OpView {
    int64_t rows = 0, cols = 0;
    Mat<E> dense;
    const rc_operator *cb = nullptr;
    static OpView of(Mat<E> a) { OpView o; o.rows = a.rows; o.cols = a.cols; o.dense = a; return o; }
    static OpView of(const rc_operator *op) {
        RC_REQUIRE(op != nullptr && op->matmat != nullptr && op->rows >= 0 && op->cols >= 0, RC_INVALID_ARGUMENT, "rc_operator: null table / matmat or negative extent");
        OpView o; o.rows = op->rows; o.cols = op->cols; o.cb = op; return o;
    }
    static rc_matrix to_c(Mat<E> m) { rc_matrix r; r.data = m.p; r.rows = m.rows; r.cols = m.cols; r.row_stride = m.rs; r.col_stride = m.cs; return r; }
    void call(rc_context *c, rc_operator_product_fn fn, const char *what, Mat<E> x, Mat<E> y) const {
        RC_REQUIRE(fn != nullptr, RC_INVALID_ARGUMENT, "rc_operator: this call needs the operator's %s", what);
        RC_REQUIRE(!c->capturing, RC_INVALID_ARGUMENT, "rc_operator: callbacks cannot be recorded into a hipGraph");
        const std::string before = c->last_error;
        const rc_status st = fn(cb->user, c, to_c(x), to_c(y));
        if (st != RC_OK) {
            const std::string inner = c->last_error != before ? c->last_error : std::string();
            fail(st, "operator callback %s (%lld x %lld -> %lld x %lld) returned status %d%s%s", what, (long long)x.rows, (long long)x.cols,
                 (long long)y.rows, (long long)y.cols, (int)st, inner.empty() ? "" : ": ", inner.c_str());
        }
    }
    // y (rows x s) = A x
    void matmat(rc_context *c, Mat<E> x, Mat<E> y) const {
        RC_REQUIRE(x.rows == cols && y.rows == rows && x.cols == y.cols, RC_INVALID_ARGUMENT, "matmat: shape mismatch");
        if (cb) call(c, cb->matmat, "matmat", x, y);
        else product(c, 1, false, dense, x, 0, y);
    }
    // y (cols x s) = A^H x  (conj_matmat: src/types.rs:128-132)
    void conj_matmat(rc_context *c, Mat<E> x, Mat<E> y) const {
        RC_REQUIRE(x.rows == rows && y.rows == cols && x.cols == y.cols, RC_INVALID_ARGUMENT, "conj_matmat: shape mismatch");
        if (cb) call(c, cb->conj_matmat, "conj_matmat", x, y);
        else product(c, 1, true, dense, x, 0, y);
    }
    // b (k x n) = range^H A = (A^H range)^H (the reference: conj_matmat, then .t(), conjugated for complex: src/qr.rs:316-317,
    // src/svd.rs:175-176).  Real: the callback is handed the n x k view of b's transpose.  Complex: a temporary and one conjugating copy.
    void project(rc_context *c, Mat<E> range, Mat<E> b) const {
        if (!cb) { product(c, 1, true, range, dense, 0, b); return; }
        if constexpr (std::is_same<E, real_t<E>>::value) {
            conj_matmat(c, range, b.t());
        } else {
            ArenaMark mark(c);
            Mat<E> t = tmp_colmajor<E>(c, cols, range.cols);
            conj_matmat(c, range, t);
            copy_mat(c, t.t(), b, true);
        }
    }
};

// QRTraits::compute_from_range_estimate (/root/reference/src/qr.rs:311-323)
template <typename E>
void qr_from_range(rc_context *c, Mat<E> range, const OpView<E> &a, Mat<E> q, Mat<E> r, int64_t *ind) {
    const int64_t m = a.rows, n = a.cols, rr = range.cols, k = std::min(rr, n);
    RC_REQUIRE(range.rows == m && q.rows == m && q.cols == k && r.rows == k && r.cols == n, RC_INVALID_ARGUMENT,
               "qr_from_range_estimate: shape mismatch");
    ArenaMark mark(c);
    Mat<E> w = tmp_colmajor<E>(c, rr, n);
    a.project(c, range, w);
    Mat<E> qb = tmp_colmajor<E>(c, rr, k);
    qrcp(c, w, k, qb, r, ind);
    product(c, 1, false, range, qb, 0, q);
}

// SampleRange::sample_range_by_rank (/root/reference/src/random_sampling.rs:103-118).
// Only the first k Householder steps influence Q[:, :k], so the factorization stops there.
template <typename E>
void sample_range_by_rank(rc_context *c, const OpView<E> &a, int64_t k, int64_t p, Mat<E> omega, uint64_t seed, Mat<E> q) {
    const int64_t m = a.rows, n = a.cols, l = k + p;
    RC_REQUIRE(k >= 0 && p >= 0, RC_INVALID_ARGUMENT, "sample_range_by_rank: negative k or p");
    const int64_t kk = std::min(k, std::min(m, l));
    RC_REQUIRE(q.rows == m && q.cols == kk, RC_INVALID_ARGUMENT, "sample_range_by_rank: q must be %lld x %lld", (long long)m, (long long)kk);
    if (kk == 0) return;
    ArenaMark mark(c);
    if (omega.p == nullptr) {
        omega = tmp_omega<E>(c, n, l);
        fill_gaussian(c, omega, seed, 0);
    } else {
        RC_REQUIRE(omega.rows == n && omega.cols == l, RC_INVALID_ARGUMENT, "sample_range_by_rank: omega must be %lld x %lld", (long long)n, (long long)l);
    }
    Mat<E> w = tmp_colmajor<E>(c, m, l);
    a.matmat(c, omega, w);
    int64_t *ind = c->alloc<int64_t>((size_t)l);
    qrcp(c, w, kk, q, Mat<E>(), ind);
}

// full pivoted QR, Q only (helper of the power iteration)
template <typename E>
Mat<E> orth_full(rc_context *c, Mat<E> w) {
    const int64_t k = std::min(w.rows, w.cols);
    Mat<E> q = tmp_colmajor<E>(c, w.rows, k);
    int64_t *ind = c->alloc<int64_t>((size_t)std::max<int64_t>(w.cols, 1));
    qrcp(c, w, k, q, Mat<E>(), ind);
    return q;
}

// SampleRangePowerIteration (/root/reference/src/random_sampling.rs:131-160).
// The inner `let op_omega = ...` (:150) shadows the outer binding, so every
// iteration restarts from A Omega and only the last one is kept: for any
// it_count >= 1 the result is QRCP(A orth(A^H orth(A Omega)))[:, :k].
template <typename E>
void sample_range_power(rc_context *c, const OpView<E> &a, int64_t k, int64_t p, int64_t it_count, Mat<E> omega, uint64_t seed, Mat<E> q) {
    if (it_count <= 0) { sample_range_by_rank(c, a, k, p, omega, seed, q); return; }
    const int64_t m = a.rows, n = a.cols, l = k + p;
    ArenaMark mark(c);
    if (omega.p == nullptr) {
        omega = tmp_omega<E>(c, n, l);
        fill_gaussian(c, omega, seed, 0);
    } else {
        RC_REQUIRE(omega.rows == n && omega.cols == l, RC_INVALID_ARGUMENT, "sample_range_power_iteration: omega must be %lld x %lld", (long long)n, (long long)l);
    }
    Mat<E> y1 = tmp_colmajor<E>(c, m, l);
    a.matmat(c, omega, y1);
    // The reference's loop restarts every iteration from the first product (a shadowed variable), so exactly one
    // power step survives; RC_OPT_POWER_ITERATION_FIXED = 1 runs the it_count steps the documentation describes.
    const int64_t steps = c->opt_power_fixed ? it_count : 1;
    for (int64_t it = 0; it < steps; ++it) {
        Mat<E> q0 = orth_full(c, y1);                    // m x min(m, l)
        Mat<E> z = tmp_colmajor<E>(c, n, q0.cols);
        a.conj_matmat(c, q0, z);
        Mat<E> wq = orth_full(c, z);                     // n x min(n, q0.cols)
        y1 = tmp_colmajor<E>(c, m, wq.cols);
        a.matmat(c, wq, y1);
    }
    const int64_t kk = std::min(k, std::min(m, y1.cols));
    RC_REQUIRE(q.rows == m && q.cols == kk, RC_INVALID_ARGUMENT, "sample_range_power_iteration: q must be %lld x %lld", (long long)m, (long long)kk);
    int64_t *ind = c->alloc<int64_t>((size_t)std::max<int64_t>(y1.cols, 1));
    qrcp(c, y1, kk, q, Mat<E>(), ind);
}

// AdaptiveSampling::sample_range_adaptive (/root/reference/src/random_sampling.rs:223-274)
template <typename E>
void sample_range_adaptive(rc_context *c, const OpView<E> &a, double rel_tol_d, int64_t s, Mat<E> omegas, uint64_t seed, Mat<E> qcap,
                           int64_t *rank_out, int64_t *hist_rank, double *hist_res, int64_t hist_cap, int64_t *hist_len) {
    using R = real_t<E>;
    const int64_t m = a.rows, n = a.cols, cap = qcap.cols;
    RC_REQUIRE(s >= 1 && qcap.rows == m, RC_INVALID_ARGUMENT, "sample_range_adaptive: bad sample_size or q buffer");
    const bool explicit_omega = omegas.p != nullptr;
    if (explicit_omega) RC_REQUIRE(omegas.rows == n, RC_INVALID_ARGUMENT, "sample_range_adaptive: omegas must have %lld rows", (long long)n);
    const R tol_factor = (R)(10.0 * std::sqrt(2.0 / 3.14159265358979323846));  // random_sampling.rs:231-234
    const R rel_tol = (R)rel_tol_d;
    const int64_t sq = std::min(m, s);  // columns a pivoted QR of an m x s block yields

    int64_t blocks_used = 0;
    auto next_omega = [&](Mat<E> dst) {
        if (explicit_omega) {
            RC_REQUIRE((blocks_used + 1) * s <= omegas.cols, RC_COMPRESSION_ERROR,
                       "sample_range_adaptive: explicit Omega blocks exhausted after %lld blocks", (long long)blocks_used);
            copy_mat(c, omegas.sub(0, n, blocks_used * s, s), dst);
        } else {
            fill_gaussian(c, dst, seed, (uint64_t)blocks_used * (uint64_t)(n * s));
        }
        ++blocks_used;
    };

    Mat<E> omega = tmp_omega<E>(c, n, s);
    Mat<E> y = tmp_colmajor<E>(c, m, s);
    Mat<E> qacc = tmp_colmajor<E>(c, m, cap);
    Mat<E> bacc = tmp_omega<E>(c, cap, n);
    Mat<E> t1 = tmp_colmajor<E>(c, cap, s);
    int64_t *ind = c->alloc<int64_t>((size_t)s);
    R *scal = c->alloc<R>(1);

    next_omega(omega);
    a.matmat(c, omega, y);
    R mc;
    max_col_norm_dev(c, y, scal);
    read_back(c, scal, &mc, 1);
    const R operator_norm = mc * tol_factor;
    R max_norm = operator_norm;
    int64_t r = 0, nh = 0;
    while (max_norm / operator_norm >= rel_tol) {
        RC_REQUIRE(r + sq <= cap, RC_COMPRESSION_ERROR, "sample_range_adaptive: basis capacity %lld exhausted at rank %lld", (long long)cap, (long long)r);
        if (r > 0) {  // y -= q (q^H y)
            Mat<E> qr_ = qacc.sub(0, m, 0, r), tt = t1.sub(0, r, 0, s);
            product(c, 1, true, qr_, y, 0, tt);
            product(c, -1, false, qr_, tt, 1, y);
        }
        Mat<E> qnew = qacc.sub(0, m, r, sq);
        qrcp(c, y, sq, qnew, Mat<E>(), ind);                   // pivoted QR of the block (:254)
        a.project(c, qnew, bacc.sub(r, sq, 0, n));             // b = [b ; (A^H Q_new)^H] (:256-260)
        r += sq;
        next_omega(omega);
        {   // y = A Omega - q (b Omega)  (:265-266)
            Mat<E> qr_ = qacc.sub(0, m, 0, r), tt = t1.sub(0, r, 0, s);
            product(c, 1, false, bacc.sub(0, r, 0, n), omega, 0, tt);
            a.matmat(c, omega, y);
            product(c, -1, false, qr_, tt, 1, y);
        }
        max_col_norm_dev(c, y, scal);
        read_back(c, scal, &mc, 1);
        max_norm = mc * tol_factor;
        if (nh < hist_cap) {
            if (hist_rank) hist_rank[nh] = r;
            if (hist_res) hist_res[nh] = (double)(max_norm / operator_norm);
        }
        ++nh;
    }
    copy_mat(c, qacc.sub(0, m, 0, r), qcap.sub(0, m, 0, r));
    if (rank_out) *rank_out = r;
    if (hist_len) *hist_len = std::min(nh, hist_cap);
    RC_HIP(hipStreamSynchronize(c->stream));
}

// |x| / |x0| as rank_by_tolerance compares it: in the scalar type for real, a hypot ratio in double for complex
template <typename T> double magnitude_ratio(T x, T x0) { return (double)std::fabs(x / x0); }
template <typename R> double magnitude_ratio(cplx<R> x, cplx<R> x0) { return std::hypot((double)x.re, (double)x.im) / std::hypot((double)x0.re, (double)x0.im); }

template <typename E>
void rank_by_tolerance(rc_context *c, Mat<E> tri, double tol, int64_t *rank) {
    RC_REQUIRE(tol < 1.0 && 0.0 <= tol, RC_INVALID_ARGUMENT, "Require 0 <= tol < 1.0");
    const int64_t len = std::min(tri.rows, tri.cols);
    RC_REQUIRE(len >= 1, RC_COMPRESSION_ERROR, "rank_by_tolerance: empty factor");
    ArenaMark mark(c);
    E *d = c->alloc<E>((size_t)len);
    copy_mat(c, Mat<E>(tri.p, len, 1, tri.rs + tri.cs, 1), Mat<E>(d, len, 1, 1, 1));
    std::vector<E> h((size_t)len);
    read_back(c, d, h.data(), (size_t)len);
    for (int64_t i = 0; i < len; ++i) {
        if (magnitude_ratio(h[i], h[0]) < tol) { *rank = i; return; }  // qr.rs:194
    }
    fail(RC_COMPRESSION_ERROR, "Could not compress to desired tolerance");
}

template <typename E>
void apply_perm_matrix(rc_context *c, int mode, Mat<E> in, const int64_t *perm, int64_t plen, Mat<E> out) {
    RC_REQUIRE(in.rows == out.rows && in.cols == out.cols, RC_INVALID_ARGUMENT, "apply_permutation: shape mismatch");
    ArenaMark mark(c);
    const bool cols = (mode == RC_PERM_COL || mode == RC_PERM_COLINV);
    const bool inv = (mode == RC_PERM_COLINV || mode == RC_PERM_ROWINV);
    RC_REQUIRE(mode >= 0 && mode <= 3, RC_INVALID_ARGUMENT, "apply_permutation: unknown mode %d", mode);
    if (cols) RC_REQUIRE(plen == in.cols, RC_INVALID_ARGUMENT, "Length of index array and number of columns differ.");
    else RC_REQUIRE(plen == in.rows, RC_INVALID_ARGUMENT, "Length of index array and number of rows differ.");
    const int64_t *idx = perm;
    if (inv) {
        int64_t *iv = c->alloc<int64_t>((size_t)std::max<int64_t>(plen, 1));
        invert_perm(c, perm, plen, iv);
        idx = iv;
    }
    if (cols) gather_cols(c, in, idx, out);
    else gather_cols(c, in.t(), idx, out.t());
}

}  // namespace

// The entry points whose bodies are the same for all four types: E the element, R = real_t<E>.  svd_from_range is each family's own.
#define RC_DEFINE_DENSE_SHARED(SUF, E, R)                                                                                                \
    rc_status rc_apply_permutation_matrix_##SUF(rc_context *ctx, int32_t mode, rc_matrix in, const int64_t *perm, int64_t plen,          \
                                                rc_matrix out) {                                                                         \
        return guarded(ctx, [&] { apply_perm_matrix<E>(ctx, mode, from_c<E>(in), perm, plen, from_c<E>(out)); });                        \
    }                                                                                                                                    \
    rc_status rc_apply_permutation_vector_##SUF(rc_context *ctx, int32_t mode, rc_matrix in, const int64_t *perm, int64_t plen,          \
                                                rc_matrix out) {                                                                         \
        return guarded(ctx, [&] {                                                                                                        \
            RC_REQUIRE(mode == RC_VPERM_INV || mode == RC_VPERM_NOINV, RC_INVALID_ARGUMENT, "unknown vector permutation mode");          \
            RC_REQUIRE(in.cols == 1 && out.cols == 1 && plen == in.rows, RC_INVALID_ARGUMENT,                                           \
                       "The input vector and the index array must have the same length");                                               \
            apply_perm_matrix<E>(ctx, mode == RC_VPERM_INV ? RC_PERM_ROWINV : RC_PERM_ROW, from_c<E>(in), perm, plen, from_c<E>(out));   \
        });                                                                                                                              \
    }                                                                                                                                    \
    rc_status rc_rank_by_tolerance_##SUF(rc_context *ctx, rc_matrix tri, double tol, int64_t *rank) {                                    \
        return guarded(ctx, [&] { rank_by_tolerance<E>(ctx, from_c<E>(tri), tol, rank); });                                              \
    }                                                                                                                                    \
    rc_status rc_max_col_norm_##SUF(rc_context *ctx, rc_matrix y, R *out) {                                                              \
        return guarded(ctx, [&] {                                                                                                        \
            /* input scale: the norms of 2^-e y, which no square leaves the range of, times 2^e */              \
            Mat<E> Y = from_c<E>(y), w = tmp_colmajor<E>(ctx, Y.rows, Y.cols);                                                           \
            R *d = ctx->alloc<R>(1);                                                                                                     \
            const int *e = input_exponent(ctx, Y);                                                                                       \
            copy_mat_scaled(ctx, Y, w, e);                                                                                               \
            max_col_norm_dev(ctx, w, d);                                                                                                 \
            rescale(ctx, Mat<R>(d, 1, 1, 1, 1), e, 1);                                                                                   \
            read_back(ctx, d, out, 1);                                                                                                   \
        });                                                                                                                              \
    }                                                                                                                                    \
    rc_status rc_qr_from_range_estimate_##SUF(rc_context *ctx, rc_matrix range, rc_matrix a, rc_matrix q, rc_matrix r, int64_t *ind) {   \
        return guarded(ctx, [&] { qr_from_range<E>(ctx, from_c<E>(range), OpView<E>::of(from_c<E>(a)), from_c<E>(q), from_c<E>(r), ind); }); \
    }                                                                                                                                    \
    rc_status rc_svd_from_range_estimate_##SUF(rc_context *ctx, rc_matrix range, rc_matrix a, rc_matrix u, R *s, rc_matrix vt) {         \
        return guarded(ctx, [&] { svd_from_range(ctx, from_c<E>(range), OpView<E>::of(from_c<E>(a)), from_c<E>(u), s, from_c<E>(vt)); }); \
    }                                                                                                                                    \
    rc_status rc_sample_range_by_rank_##SUF(rc_context *ctx, rc_matrix a, int64_t k, int64_t p, rc_matrix omega, uint64_t seed,          \
                                            rc_matrix q) {                                                                               \
        return guarded(ctx, [&] { sample_range_by_rank<E>(ctx, OpView<E>::of(from_c<E>(a)), k, p, from_c<E>(omega), seed, from_c<E>(q)); }); \
    }                                                                                                                                    \
    rc_status rc_sample_range_power_iteration_##SUF(rc_context *ctx, rc_matrix a, int64_t k, int64_t p, int64_t it, rc_matrix omega,     \
                                                    uint64_t seed, rc_matrix q) {                                                        \
        return guarded(ctx, [&] { sample_range_power<E>(ctx, OpView<E>::of(from_c<E>(a)), k, p, it, from_c<E>(omega), seed, from_c<E>(q)); }); \
    }                                                                                                                                    \
    rc_status rc_sample_range_adaptive_##SUF(rc_context *ctx, rc_matrix a, double rel_tol, int64_t s, rc_matrix omegas, uint64_t seed,   \
                                             rc_matrix q_cap, int64_t *rank, int64_t *hist_rank, double *hist_res, int64_t hist_cap,     \
                                             int64_t *hist_len) {                                                                        \
        return guarded(ctx, [&] {                                                                                                        \
            sample_range_adaptive<E>(ctx, OpView<E>::of(from_c<E>(a)), rel_tol, s, from_c<E>(omegas), seed, from_c<E>(q_cap), rank, hist_rank, \
                                     hist_res, hist_cap, hist_len);                                                                      \
        });                                                                                                                              \
    }                                                                                                                                    \
    /* the same compositions over the host's operator callbacks (rc_operator) */                                                         \
    rc_status rc_sample_range_by_rank_op_##SUF(rc_context *ctx, const rc_operator *op, int64_t k, int64_t p, rc_matrix omega,            \
                                               uint64_t seed, rc_matrix q) {                                                             \
        return guarded(ctx, [&] { sample_range_by_rank<E>(ctx, OpView<E>::of(op), k, p, from_c<E>(omega), seed, from_c<E>(q)); });       \
    }                                                                                                                                    \
    rc_status rc_sample_range_power_iteration_op_##SUF(rc_context *ctx, const rc_operator *op, int64_t k, int64_t p, int64_t it,         \
                                                       rc_matrix omega, uint64_t seed, rc_matrix q) {                                    \
        return guarded(ctx, [&] { sample_range_power<E>(ctx, OpView<E>::of(op), k, p, it, from_c<E>(omega), seed, from_c<E>(q)); });     \
    }                                                                                                                                    \
    rc_status rc_sample_range_adaptive_op_##SUF(rc_context *ctx, const rc_operator *op, double rel_tol, int64_t s, rc_matrix omegas,     \
                                                uint64_t seed, rc_matrix q_cap, int64_t *rank, int64_t *hist_rank, double *hist_res,     \
                                                int64_t hist_cap, int64_t *hist_len) {                                                   \
        return guarded(ctx, [&] {                                                                                                        \
            sample_range_adaptive<E>(ctx, OpView<E>::of(op), rel_tol, s, from_c<E>(omegas), seed, from_c<E>(q_cap), rank, hist_rank,     \
                                     hist_res, hist_cap, hist_len);                                                                      \
        });                                                                                                                              \
    }                                                                                                                                    \
    rc_status rc_qr_from_range_estimate_op_##SUF(rc_context *ctx, rc_matrix range, const rc_operator *op, rc_matrix q, rc_matrix r,      \
                                                 int64_t *ind) {                                                                         \
        return guarded(ctx, [&] { qr_from_range<E>(ctx, from_c<E>(range), OpView<E>::of(op), from_c<E>(q), from_c<E>(r), ind); });       \
    }                                                                                                                                    \
    rc_status rc_svd_from_range_estimate_op_##SUF(rc_context *ctx, rc_matrix range, const rc_operator *op, rc_matrix u, R *s,            \
                                                  rc_matrix vt) {                                                                        \
        return guarded(ctx, [&] { svd_from_range(ctx, from_c<E>(range), OpView<E>::of(op), from_c<E>(u), s, from_c<E>(vt)); });          \
    }
