// rusty_compression.hpp -- header-only C++ mirror of the reference crate's operator / trait
// surface (rusty-compression v0.1.1, /root/reference/src/lib.rs:90-102) over the C ABI of
// librusty_compression_amd.so (rusty_compression_amd.h).  The reference is compiled (Rust) code
// and no Rust toolchain exists in the build image, so this is the compiled-language host side:
// same names, same argument meaning, same error behaviour -- and no arithmetic: every method is
// one call into the C ABI.  The Rust rendition of the same surface is in bindings/rust/.
//
//   using namespace rusty_compression;
//   Context ctx(0);
//   auto a   = DeviceMatrix<double>::from_host(ctx, host_ptr, m, n);        // C-order host data
//   auto qr  = QR<double>::compute_from(a).compress(CompressionType::RANK(20));
//   auto tid = qr.column_id().two_sided_id();                               // examples/interpolative_decomposition.rs
//   double err = rel_diff_fro(tid.to_mat(), a);
#pragma once

#include <algorithm>
#include <cmath>
#include <complex>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <utility>
#include <type_traits>
#include <vector>

#include "rusty_compression_amd.h"

namespace rusty_compression {

// ---- errors: RustyCompressionError (reference src/types.rs:11-21) ------------------------------
struct RustyCompressionError : std::runtime_error { using std::runtime_error::runtime_error; };
struct LinalgError : RustyCompressionError { using RustyCompressionError::RustyCompressionError; };
struct CompressionError : RustyCompressionError { using RustyCompressionError::RustyCompressionError; };
struct LayoutError : RustyCompressionError { using RustyCompressionError::RustyCompressionError; };
struct PivotedQRError : RustyCompressionError { using RustyCompressionError::RustyCompressionError; };
struct AssertionFailed : std::logic_error { using std::logic_error::logic_error; };  // the reference panics
struct HipRuntimeError : RustyCompressionError { using RustyCompressionError::RustyCompressionError; };

// ---- CompressionType (reference src/lib.rs:82-87) ----------------------------------------------
struct CompressionType {
    enum Kind { ADAPTIVE_, RANK_ } kind;
    double value;
    static CompressionType ADAPTIVE(double tol) { return {ADAPTIVE_, tol}; }
    static CompressionType RANK(std::size_t rank) { return {RANK_, (double)rank}; }
};
enum class MatrixPermutationMode { COL = RC_PERM_COL, ROW = RC_PERM_ROW, COLINV = RC_PERM_COLINV, ROWINV = RC_PERM_ROWINV };

class Context {
  public:
    explicit Context(int device = 0, void *hip_stream = nullptr) {
        if (rc_create(&raw_, device, hip_stream) != RC_OK) throw HipRuntimeError("rc_create failed (no MI355X visible?)");
    }
    ~Context() { rc_destroy(raw_); }
    Context(const Context &) = delete;
    Context &operator=(const Context &) = delete;
    rc_context *raw() const { return raw_; }
    void synchronize() const { check(rc_synchronize(raw_)); }
    void set_option(int32_t option, int64_t value) const { check(rc_set_option(raw_, option, value)); }
    void check(rc_status st) const {
        if (st == RC_OK) return;
        const std::string msg = rc_last_error_message(raw_);
        switch (st) {
            case RC_LINALG_ERROR: throw LinalgError(msg);
            case RC_COMPRESSION_ERROR: throw CompressionError(msg.empty() ? "Could not compress to desired tolerance" : msg);
            case RC_LAYOUT_ERROR: throw LayoutError(msg);
            case RC_PIVOTED_QR_ERROR: throw PivotedQRError(msg);
            case RC_INVALID_ARGUMENT: throw AssertionFailed(msg);
            default: throw HipRuntimeError(msg);
        }
    }

  private:
    rc_context *raw_ = nullptr;
};

// ---- scalar dispatch --------------------------------------------------------------------------
// the reference's `Scalar` (f32, f64, c32, c64; src/lib.rs): Real = the type of norms, tolerances and singular values, wire = how
// a scalar crosses the C ABI (complex numbers as the (re, im) pairs rc_complex32 / rc_complex64)
template <typename T> struct Scalar {
    using real = T;
    static constexpr bool is_complex = false;
    static T wire(T v) { return v; }
};
template <> struct Scalar<std::complex<float>> {
    using real = float;
    static constexpr bool is_complex = true;
    static rc_complex32 wire(std::complex<float> v) { return rc_complex32{v.real(), v.imag()}; }
};
template <> struct Scalar<std::complex<double>> {
    using real = double;
    static constexpr bool is_complex = true;
    static rc_complex64 wire(std::complex<double> v) { return rc_complex64{v.real(), v.imag()}; }
};
using c32 = std::complex<float>;
using c64 = std::complex<double>;

template <typename T> struct Api;
#define RC_API(T, SUF, RSUF)                                                                                      \
    template <> struct Api<T> {                                                                                     \
        static constexpr auto random_gaussian = rc_random_gaussian_##SUF;                                           \
        static constexpr auto matmat = rc_matmat_##SUF;                                                             \
        static constexpr auto conj_matmat = rc_conj_matmat_##SUF;                                                   \
        static constexpr auto gemm = rc_gemm_##SUF;                                                                 \
        static constexpr auto rel_diff_fro = rc_rel_diff_fro_##SUF;                                                 \
        static constexpr auto apply_permutation_matrix = rc_apply_permutation_matrix_##SUF;                         \
        static constexpr auto pivoted_qr = rc_pivoted_qr_##SUF;                                                     \
        static constexpr auto pivoted_lq = rc_pivoted_lq_##SUF;                                                     \
        static constexpr auto geqp3 = rc_geqp3_##SUF;                                                               \
        static constexpr auto orgqr = rc_orgqr_##SUF;                                                               \
        static constexpr auto trsm_upper = rc_trsm_upper_##SUF;                                                     \
        static constexpr auto compute_svd = rc_compute_svd_##SUF;                                                   \
        static constexpr auto rank_by_tolerance = rc_rank_by_tolerance_##SUF;                                       \
        static constexpr auto qr_to_mat = rc_qr_to_mat_##SUF;                                                       \
        static constexpr auto lq_to_mat = rc_lq_to_mat_##SUF;                                                       \
        static constexpr auto qr_column_id = rc_qr_column_id_##SUF;                                                 \
        static constexpr auto lq_row_id = rc_lq_row_id_##SUF;                                                       \
        static constexpr auto qr_from_range_estimate = rc_qr_from_range_estimate_##SUF;                             \
        static constexpr auto svd_rank_by_tolerance = rc_svd_rank_by_tolerance_##RSUF; /* singular values are real */                           \
        static constexpr auto svd_to_mat = rc_svd_to_mat_##SUF;                                                     \
        static constexpr auto svd_to_qr = rc_svd_to_qr_##SUF;                                                       \
        static constexpr auto svd_from_range_estimate = rc_svd_from_range_estimate_##SUF;                           \
        static constexpr auto column_id_two_sided = rc_column_id_two_sided_##SUF;                                   \
        static constexpr auto row_id_two_sided = rc_row_id_two_sided_##SUF;                                         \
        static constexpr auto max_col_norm = rc_max_col_norm_##SUF;                                                 \
        static constexpr auto sample_range_by_rank = rc_sample_range_by_rank_##SUF;                                 \
        static constexpr auto sample_range_power_iteration = rc_sample_range_power_iteration_##SUF;                 \
        static constexpr auto sample_range_adaptive = rc_sample_range_adaptive_##SUF;                               \
        static constexpr auto column_id_rank = rc_column_id_rank_##SUF;                                             \
        static constexpr auto column_id_rank_batched = rc_column_id_rank_batched_##SUF;                             \
        static constexpr auto two_sided_id_rank_batched = rc_two_sided_id_rank_batched_##SUF;                       \
        static constexpr auto svd_rank_batched = rc_svd_rank_batched_##SUF;                                         \
        static constexpr auto lowrank_apply_batched = rc_lowrank_apply_batched_##SUF;                               \
    };
RC_API(double, f64, f64)
RC_API(float, f32, f32)
RC_API(c64, c64, f64)
RC_API(c32, c32, f32)
#undef RC_API

// ---- device-resident C-order arrays (the reference's Array2 / Array1<usize>) ----------------------
template <typename T>
class DeviceBuffer {
  public:
    DeviceBuffer() = default;
    DeviceBuffer(const Context &ctx, std::size_t count) : ctx_(&ctx), count_(count) {
        ctx.check(rc_device_malloc(ctx.raw(), count * sizeof(T), &ptr_));
    }
    DeviceBuffer(DeviceBuffer &&o) noexcept { *this = std::move(o); }
    DeviceBuffer &operator=(DeviceBuffer &&o) noexcept {
        release();
        ctx_ = o.ctx_; ptr_ = o.ptr_; count_ = o.count_;
        o.ptr_ = nullptr; o.count_ = 0;
        return *this;
    }
    DeviceBuffer(const DeviceBuffer &) = delete;
    DeviceBuffer &operator=(const DeviceBuffer &) = delete;
    ~DeviceBuffer() { release(); }
    T *data() const { return static_cast<T *>(ptr_); }
    std::size_t size() const { return count_; }
    const Context &ctx() const { return *ctx_; }
    std::vector<T> to_host() const {
        std::vector<T> h(count_);
        if (count_) ctx_->check(rc_memcpy_d2h(ctx_->raw(), h.data(), ptr_, count_ * sizeof(T)));
        return h;
    }
    void from_host(const T *src) { if (count_) ctx_->check(rc_memcpy_h2d(ctx_->raw(), ptr_, src, count_ * sizeof(T))); }

  private:
    void release() { if (ptr_ && ctx_) rc_device_free(ctx_->raw(), ptr_); ptr_ = nullptr; }
    const Context *ctx_ = nullptr;
    void *ptr_ = nullptr;
    std::size_t count_ = 0;
};

template <typename T>
class DeviceMatrix {
  public:
    DeviceMatrix() = default;
    DeviceMatrix(const Context &ctx, int64_t rows, int64_t cols) : buf_(ctx, (std::size_t)(rows * cols)), rows_(rows), cols_(cols) {}
    static DeviceMatrix from_host(const Context &ctx, const T *c_order, int64_t rows, int64_t cols) {
        DeviceMatrix m(ctx, rows, cols);
        m.buf_.from_host(c_order);
        return m;
    }
    std::vector<T> to_host() const { return buf_.to_host(); }
    int64_t nrows() const { return rows_; }
    int64_t ncols() const { return cols_; }
    const Context &ctx() const { return buf_.ctx(); }
    rc_matrix view() const { return rc_matrix{buf_.data(), rows_, cols_, cols_, 1}; }
    // owned copy of the leading rows x cols block (the reference's slice(..).to_owned()):
    // one strided gather through the permutation entry point with the identity index
    DeviceMatrix leading(int64_t rows, int64_t cols) const {
        DeviceMatrix out(ctx(), rows, cols);
        if (rows == 0 || cols == 0) return out;
        std::vector<int64_t> h((std::size_t)cols);
        for (int64_t i = 0; i < cols; ++i) h[(std::size_t)i] = i;
        DeviceBuffer<int64_t> idx(ctx(), (std::size_t)cols);
        idx.from_host(h.data());
        rc_matrix src{buf_.data(), rows, cols, cols_, 1};
        ctx().check(Api<T>::apply_permutation_matrix(ctx().raw(), RC_PERM_COL, src, idx.data(), cols, out.view()));
        ctx().synchronize();  // idx is freed on return
        return out;
    }

  private:
    DeviceBuffer<T> buf_;
    int64_t rows_ = 0, cols_ = 0;
};

using DeviceIndex = DeviceBuffer<int64_t>;

inline DeviceIndex clone_index(const DeviceIndex &src) {
    DeviceIndex out(src.ctx(), src.size());
    auto h = src.to_host();
    out.from_host(h.data());
    return out;
}
template <typename T>
inline DeviceMatrix<T> clone_matrix(const DeviceMatrix<T> &src) { return src.leading(src.nrows(), src.ncols()); }

// ---- types.rs ----------------------------------------------------------------------------------
template <typename T>
DeviceMatrix<T> dot(const DeviceMatrix<T> &a, const DeviceMatrix<T> &b) {  // ndarray .dot
    DeviceMatrix<T> c(a.ctx(), a.nrows(), b.ncols());
    a.ctx().check(Api<T>::gemm(a.ctx().raw(), 0, 0, Scalar<T>::wire((T)1), a.view(), b.view(), Scalar<T>::wire((T)0), c.view()));
    return c;
}
// op(a) op(b) with op = 0: as is, 1: transpose, 2: conjugate transpose (the reference writes `.t().map(|x| x.conj())`)
template <typename T>
DeviceMatrix<T> dot_op(int op_a, const DeviceMatrix<T> &a, int op_b, const DeviceMatrix<T> &b) {
    DeviceMatrix<T> c(a.ctx(), op_a ? a.ncols() : a.nrows(), op_b ? b.nrows() : b.ncols());
    a.ctx().check(Api<T>::gemm(a.ctx().raw(), op_a, op_b, Scalar<T>::wire((T)1), a.view(), b.view(), Scalar<T>::wire((T)0), c.view()));
    return c;
}
template <typename T>
DeviceMatrix<T> matmat(const DeviceMatrix<T> &op, const DeviceMatrix<T> &x) {  // MatMat::matmat, src/types.rs:58-71
    DeviceMatrix<T> y(op.ctx(), op.nrows(), x.ncols());
    op.ctx().check(Api<T>::matmat(op.ctx().raw(), op.view(), x.view(), y.view()));
    return y;
}
template <typename T>
DeviceMatrix<T> conj_matmat(const DeviceMatrix<T> &op, const DeviceMatrix<T> &x) {  // ConjMatMat, src/types.rs:88-101
    DeviceMatrix<T> y(op.ctx(), op.ncols(), x.ncols());
    op.ctx().check(Api<T>::conj_matmat(op.ctx().raw(), op.view(), x.view(), y.view()));
    return y;
}
template <typename T>
typename Scalar<T>::real rel_diff_fro(const DeviceMatrix<T> &first, const DeviceMatrix<T> &second) {  // RelDiff, src/types.rs:182-188
    typename Scalar<T>::real out = 0;
    first.ctx().check(Api<T>::rel_diff_fro(first.ctx().raw(), first.view(), second.view(), &out));
    return out;
}
template <typename T>
DeviceMatrix<T> random_gaussian(const Context &ctx, int64_t rows, int64_t cols, uint64_t seed, uint64_t offset = 0) {
    DeviceMatrix<T> out(ctx, rows, cols);  // RandomMatrix::random_gaussian, src/random_matrix.rs:21
    ctx.check(Api<T>::random_gaussian(ctx.raw(), out.view(), seed, offset));
    return out;
}

template <typename T> struct ColumnID;
template <typename T> struct RowID;
template <typename T> struct TwoSidedID;

// ---- the LAPACK seam: what the reference calls per factorization ($qrf = ?geqp3 at src/pivoted_qr.rs:139-172, lax::Lapack::q =
// ?orgqr / ?ungqr at :104-108, solve_triangular = ?trtrs at src/qr.rs:298, :392), in LAPACK's own formats ----------------------
template <typename T>
struct Geqp3 {
    DeviceMatrix<T> a;        // the factored A P: R on / above the diagonal, Householder vectors below it (columns in pivoted order)
    DeviceIndex jpvt;         // 0-based
    DeviceBuffer<T> tau;
};
template <typename T>
Geqp3<T> geqp3(const DeviceMatrix<T> &mat, int64_t kmax = -1) {
    const int64_t m = mat.nrows(), n = mat.ncols();
    if (kmax < 0) kmax = m < n ? m : n;
    Geqp3<T> out{clone_matrix(mat), DeviceIndex(mat.ctx(), (std::size_t)n), DeviceBuffer<T>(mat.ctx(), (std::size_t)(kmax > 0 ? kmax : 1))};
    using wire_t = decltype(Scalar<T>::wire(T()));
    mat.ctx().check(Api<T>::geqp3(mat.ctx().raw(), out.a.view(), kmax, out.jpvt.data(), reinterpret_cast<wire_t *>(out.tau.data())));
    return out;
}
template <typename T>
DeviceMatrix<T> orgqr(const Geqp3<T> &f, int64_t k) {
    using wire_t = decltype(Scalar<T>::wire(T()));
    DeviceMatrix<T> q(f.a.ctx(), f.a.nrows(), k);
    f.a.ctx().check(Api<T>::orgqr(f.a.ctx().raw(), f.a.view(), reinterpret_cast<const wire_t *>(f.tau.data()), k, q.view()));
    return q;
}
template <typename T>
DeviceMatrix<T> trsm_upper(const DeviceMatrix<T> &t, const DeviceMatrix<T> &b) {  // returns X with T X = B
    DeviceMatrix<T> x = clone_matrix(b);
    t.ctx().check(Api<T>::trsm_upper(t.ctx().raw(), t.view(), x.view()));
    return x;
}

// ---- qr.rs ---------------------------------------------------------------------------------------
template <typename T>
struct QR {  // src/qr.rs:31-40
    DeviceMatrix<T> q, r;
    DeviceIndex ind;
    int64_t nrows() const { return q.nrows(); }
    int64_t ncols() const { return r.ncols(); }
    int64_t rank() const { return q.ncols(); }

    // src/qr.rs:251-253.  Input scale: the paragraph at rc_pivoted_qr_* (rusty_compression_amd.h) holds for compute_from here, in LQ and
    // in SVD; compute_from_range_estimate promises no input-scale domain yet.
    static QR compute_from(const DeviceMatrix<T> &a) {
        const int64_t m = a.nrows(), n = a.ncols(), k = m < n ? m : n;
        QR out{DeviceMatrix<T>(a.ctx(), m, k), DeviceMatrix<T>(a.ctx(), k, n), DeviceIndex(a.ctx(), (std::size_t)n)};
        a.ctx().check(Api<T>::pivoted_qr(a.ctx().raw(), a.view(), out.q.view(), out.r.view(), out.ind.data()));
        return out;
    }
    static QR compute_from_range_estimate(const DeviceMatrix<T> &range, const DeviceMatrix<T> &op) {  // src/qr.rs:311-323
        const int64_t m = op.nrows(), n = op.ncols(), k = range.ncols() < n ? range.ncols() : n;
        QR out{DeviceMatrix<T>(op.ctx(), m, k), DeviceMatrix<T>(op.ctx(), k, n), DeviceIndex(op.ctx(), (std::size_t)n)};
        op.ctx().check(Api<T>::qr_from_range_estimate(op.ctx().raw(), range.view(), op.view(), out.q.view(), out.r.view(), out.ind.data()));
        return out;
    }
    DeviceMatrix<T> to_mat() const {  // src/qr.rs:160-166
        DeviceMatrix<T> out(q.ctx(), nrows(), ncols());
        q.ctx().check(Api<T>::qr_to_mat(q.ctx().raw(), q.view(), r.view(), ind.data(), out.view()));
        return out;
    }
    QR compress_qr_rank(int64_t max_rank) const {  // src/qr.rs:169-184
        if (max_rank > q.ncols()) max_rank = q.ncols();
        return QR{q.leading(q.nrows(), max_rank), r.leading(max_rank, r.ncols()), clone_index(ind)};
    }
    QR compress_qr_tolerance(double tol) const {  // src/qr.rs:187-200
        int64_t rank = -1;
        q.ctx().check(Api<T>::rank_by_tolerance(q.ctx().raw(), r.view(), tol, &rank));
        return compress_qr_rank(rank);
    }
    QR compress(CompressionType ct) const {  // src/qr.rs:203-208
        return ct.kind == CompressionType::ADAPTIVE_ ? compress_qr_tolerance(ct.value) : compress_qr_rank((int64_t)ct.value);
    }
    ColumnID<T> column_id() const;  // src/qr.rs:270-309
};

template <typename T>
struct LQ {  // src/qr.rs:42-51
    DeviceMatrix<T> l, q;
    DeviceIndex ind;
    int64_t nrows() const { return l.nrows(); }
    int64_t ncols() const { return q.ncols(); }
    int64_t rank() const { return q.nrows(); }
    static LQ compute_from(const DeviceMatrix<T> &a) {  // src/qr.rs:354-362
        const int64_t m = a.nrows(), n = a.ncols(), k = m < n ? m : n;
        LQ out{DeviceMatrix<T>(a.ctx(), m, k), DeviceMatrix<T>(a.ctx(), k, n), DeviceIndex(a.ctx(), (std::size_t)m)};
        a.ctx().check(Api<T>::pivoted_lq(a.ctx().raw(), a.view(), out.l.view(), out.q.view(), out.ind.data()));
        return out;
    }
    DeviceMatrix<T> to_mat() const {  // src/qr.rs:73-77
        DeviceMatrix<T> out(q.ctx(), nrows(), ncols());
        q.ctx().check(Api<T>::lq_to_mat(q.ctx().raw(), l.view(), q.view(), ind.data(), out.view()));
        return out;
    }
    LQ compress_lq_rank(int64_t max_rank) const {  // src/qr.rs:80-96
        if (max_rank > q.nrows()) max_rank = q.nrows();
        return LQ{l.leading(l.nrows(), max_rank), q.leading(max_rank, q.ncols()), clone_index(ind)};
    }
    LQ compress(CompressionType ct) const {  // src/qr.rs:99-119
        if (ct.kind == CompressionType::RANK_) return compress_lq_rank((int64_t)ct.value);
        int64_t rank = -1;
        q.ctx().check(Api<T>::rank_by_tolerance(q.ctx().raw(), l.view(), ct.value, &rank));
        return compress_lq_rank(rank);
    }
    RowID<T> row_id() const;  // src/qr.rs:363-403
};

// ---- col / row / two-sided interpolative decompositions ----------------------------------------------
template <typename T>
struct TwoSidedID {  // src/two_sided_interp_decomp.rs:19-30
    DeviceMatrix<T> c, x, r;
    DeviceIndex row_ind, col_ind;
    int64_t rank() const { return c.ncols(); }
    DeviceMatrix<T> to_mat() const { return rusty_compression::dot(c, rusty_compression::dot(x, r)); }             // :62-64
    DeviceMatrix<T> dot(const DeviceMatrix<T> &rhs) const {                                                        // Apply, :154-171
        return rusty_compression::dot(c, rusty_compression::dot(x, rusty_compression::dot(r, rhs)));
    }
};
template <typename T>
struct ColumnID {  // src/col_interp_decomp.rs:23-31
    DeviceMatrix<T> c, z;
    DeviceIndex col_ind;
    int64_t rank() const { return c.ncols(); }
    DeviceMatrix<T> to_mat() const { return rusty_compression::dot(c, z); }                                        // :63-65
    DeviceMatrix<T> dot(const DeviceMatrix<T> &rhs) const { return rusty_compression::dot(c, rusty_compression::dot(z, rhs)); }  // Apply
    TwoSidedID<T> two_sided_id() const {  // src/col_interp_decomp.rs:116-125
        const int64_t m = c.nrows(), k = c.ncols(), kk = m < k ? m : k;
        TwoSidedID<T> out{DeviceMatrix<T>(c.ctx(), m, kk), DeviceMatrix<T>(c.ctx(), kk, k), clone_matrix(z), DeviceIndex(c.ctx(), (std::size_t)m), clone_index(col_ind)};
        c.ctx().check(Api<T>::column_id_two_sided(c.ctx().raw(), c.view(), out.c.view(), out.x.view(), out.row_ind.data()));
        return out;
    }
};
template <typename T>
struct RowID {  // src/row_interp_decomp.rs:25-33
    DeviceMatrix<T> x, r;
    DeviceIndex row_ind;
    int64_t rank() const { return r.nrows(); }
    DeviceMatrix<T> to_mat() const { return rusty_compression::dot(x, r); }
    DeviceMatrix<T> dot(const DeviceMatrix<T> &rhs) const { return rusty_compression::dot(x, rusty_compression::dot(r, rhs)); }
    TwoSidedID<T> two_sided_id() const {  // src/row_interp_decomp.rs:120-130
        const int64_t k = r.nrows(), n = r.ncols(), kk = k < n ? k : n;
        TwoSidedID<T> out{clone_matrix(x), DeviceMatrix<T>(r.ctx(), k, kk), DeviceMatrix<T>(r.ctx(), kk, n), clone_index(row_ind), DeviceIndex(r.ctx(), (std::size_t)n)};
        r.ctx().check(Api<T>::row_id_two_sided(r.ctx().raw(), r.view(), out.x.view(), out.r.view(), out.col_ind.data()));
        return out;
    }
};
template <typename T>
ColumnID<T> QR<T>::column_id() const {
    ColumnID<T> out{DeviceMatrix<T>(q.ctx(), nrows(), rank()), DeviceMatrix<T>(q.ctx(), rank(), ncols()), clone_index(ind)};
    q.ctx().check(Api<T>::qr_column_id(q.ctx().raw(), q.view(), r.view(), ind.data(), out.c.view(), out.z.view()));
    return out;
}
template <typename T>
RowID<T> LQ<T>::row_id() const {
    RowID<T> out{DeviceMatrix<T>(q.ctx(), nrows(), rank()), DeviceMatrix<T>(q.ctx(), rank(), ncols()), clone_index(ind)};
    q.ctx().check(Api<T>::lq_row_id(q.ctx().raw(), l.view(), q.view(), ind.data(), out.x.view(), out.r.view()));
    return out;
}

// ---- svd.rs --------------------------------------------------------------------------------------
template <typename T>
struct SVD {  // src/svd.rs:13-20
    using Real = typename Scalar<T>::real;
    DeviceMatrix<T> u;
    DeviceBuffer<Real> s;  // singular values are real for every scalar type
    DeviceMatrix<T> vt;
    int64_t rank() const { return u.ncols(); }
    static SVD compute_from(const DeviceMatrix<T> &a) {  // src/svd.rs:165-169 -> src/compute_svd.rs:18-27
        const int64_t m = a.nrows(), n = a.ncols(), r = m < n ? m : n;
        SVD out{DeviceMatrix<T>(a.ctx(), m, r), DeviceBuffer<Real>(a.ctx(), (std::size_t)r), DeviceMatrix<T>(a.ctx(), r, n)};
        a.ctx().check(Api<T>::compute_svd(a.ctx().raw(), a.view(), out.u.view(), out.s.data(), out.vt.view()));
        return out;
    }
    static SVD compute_from_range_estimate(const DeviceMatrix<T> &range, const DeviceMatrix<T> &op) {  // src/svd.rs:171-183
        const int64_t m = op.nrows(), n = op.ncols(), r = range.ncols() < n ? range.ncols() : n;
        SVD out{DeviceMatrix<T>(op.ctx(), m, r), DeviceBuffer<Real>(op.ctx(), (std::size_t)r), DeviceMatrix<T>(op.ctx(), r, n)};
        op.ctx().check(Api<T>::svd_from_range_estimate(op.ctx().raw(), range.view(), op.view(), out.u.view(), out.s.data(), out.vt.view()));
        return out;
    }
    DeviceMatrix<T> to_mat() const {  // src/svd.rs:42-54
        DeviceMatrix<T> out(u.ctx(), u.nrows(), vt.ncols());
        u.ctx().check(Api<T>::svd_to_mat(u.ctx().raw(), u.view(), s.data(), vt.view(), out.view()));
        return out;
    }
    QR<T> to_qr() const {  // src/svd.rs:150-163
        const int64_t r = vt.nrows(), n = vt.ncols(), k = r < n ? r : n;
        QR<T> out{DeviceMatrix<T>(u.ctx(), u.nrows(), k), DeviceMatrix<T>(u.ctx(), k, n), DeviceIndex(u.ctx(), (std::size_t)n)};
        u.ctx().check(Api<T>::svd_to_qr(u.ctx().raw(), u.view(), s.data(), vt.view(), out.q.view(), out.r.view(), out.ind.data()));
        return out;
    }
    SVD compress_svd_rank(int64_t max_rank) const {  // src/svd.rs:68-84
        if (max_rank > (int64_t)s.size()) max_rank = (int64_t)s.size();
        auto hs = s.to_host();
        DeviceBuffer<Real> s2(u.ctx(), (std::size_t)max_rank);
        s2.from_host(hs.data());
        return SVD{u.leading(u.nrows(), max_rank), std::move(s2), vt.leading(max_rank, vt.ncols())};
    }
    SVD compress(CompressionType ct) const {  // src/svd.rs:60-101
        if (ct.kind == CompressionType::RANK_) return compress_svd_rank((int64_t)ct.value);
        int64_t rank = -1;
        u.ctx().check(Api<T>::svd_rank_by_tolerance(u.ctx().raw(), s.data(), (int64_t)s.size(), ct.value, &rank));
        return compress_svd_rank(rank);
    }
};

// ---- random_matrix.rs (orthogonal / approximately low-rank test matrices) ---------------------------
template <typename T>
DeviceMatrix<T> transpose(const DeviceMatrix<T> &a) {  // owned C-order copy of a^T
    DeviceMatrix<T> out(a.ctx(), a.ncols(), a.nrows());
    if (a.nrows() == 0 || a.ncols() == 0) return out;
    std::vector<int64_t> h((std::size_t)a.nrows());
    for (int64_t i = 0; i < a.nrows(); ++i) h[(std::size_t)i] = i;
    DeviceIndex idx(a.ctx(), h.size());
    idx.from_host(h.data());
    rc_matrix at{a.view().data, a.ncols(), a.nrows(), 1, a.ncols()};
    a.ctx().check(Api<T>::apply_permutation_matrix(a.ctx().raw(), RC_PERM_COL, at, idx.data(), a.nrows(), out.view()));
    a.ctx().synchronize();
    return out;
}
template <typename T>
DeviceMatrix<T> conj_transpose(const DeviceMatrix<T> &a) {  // owned C-order copy of a^H (= a^T for real scalars)
    if (!Scalar<T>::is_complex) return transpose(a);
    std::vector<T> eye((std::size_t)(a.nrows() * a.nrows()), (T)0);
    for (int64_t i = 0; i < a.nrows(); ++i) eye[(std::size_t)(i * a.nrows() + i)] = (T)1;
    return dot_op(2, a, 0, DeviceMatrix<T>::from_host(a.ctx(), eye.data(), a.nrows(), a.nrows()));
}
template <typename T>
DeviceMatrix<T> random_orthogonal_matrix(const Context &ctx, int64_t rows, int64_t cols, uint64_t seed, uint64_t offset = 0) {  // src/random_matrix.rs:35-56
    const bool swap = cols > rows;
    auto g = random_gaussian<T>(ctx, swap ? cols : rows, swap ? rows : cols, seed, offset);
    auto u = std::move(SVD<T>::compute_from(g).u);
    return swap ? conj_transpose(u) : std::move(u);  // src/random_matrix.rs:51-53
}
template <typename T>
DeviceMatrix<T> random_approximate_low_rank_matrix(const Context &ctx, int64_t rows, int64_t cols, double sigma_max, double sigma_min,
                                                   uint64_t seed) {  // src/random_matrix.rs:70-93
    if (!(sigma_min < sigma_max)) throw AssertionFailed("`sigma_min` must be smaller than `sigma_max`");
    if (!(sigma_min > 0.0)) throw AssertionFailed("`sigma_min` must be positive.");
    using Real = typename Scalar<T>::real;
    const int64_t r = rows < cols ? rows : cols;
    std::vector<Real> hs((std::size_t)r);
    const double l0 = std::log10(sigma_min), l1 = std::log10(sigma_max);
    for (int64_t i = 0; i < r; ++i) hs[(std::size_t)i] = (Real)std::pow(10.0, r > 1 ? l0 + (l1 - l0) * (double)i / (double)(r - 1) : l0);
    SVD<T> f{random_orthogonal_matrix<T>(ctx, rows, r, seed, 0), DeviceBuffer<Real>(ctx, (std::size_t)r),
             random_orthogonal_matrix<T>(ctx, r, cols, seed, (uint64_t)(rows * r))};
    f.s.from_host(hs.data());
    return f.to_mat();
}

// ---- random_sampling.rs -----------------------------------------------------------------------------
template <typename T>
DeviceMatrix<T> sample_range_by_rank(const DeviceMatrix<T> &op, int64_t k, int64_t p, uint64_t seed) {  // :103-118
    int64_t kk = k < op.nrows() ? k : op.nrows();
    if (k + p < kk) kk = k + p;
    DeviceMatrix<T> q(op.ctx(), op.nrows(), kk);
    op.ctx().check(Api<T>::sample_range_by_rank(op.ctx().raw(), op.view(), k, p, rc_matrix{nullptr, 0, 0, 0, 0}, seed, q.view()));
    return q;
}
template <typename T>
DeviceMatrix<T> sample_range_power_iteration(const DeviceMatrix<T> &op, int64_t k, int64_t p, int64_t it_count, uint64_t seed) {  // :131-160
    int64_t kk = k < op.nrows() ? k : op.nrows();
    if (k + p < kk) kk = k + p;
    if (op.ncols() < kk) kk = op.ncols();
    DeviceMatrix<T> q(op.ctx(), op.nrows(), kk);
    op.ctx().check(Api<T>::sample_range_power_iteration(op.ctx().raw(), op.view(), k, p, it_count, rc_matrix{nullptr, 0, 0, 0, 0}, seed, q.view()));
    return q;
}
// the unit of work of batches (examples/interpolative_decomposition.rs:25-32 in one call, truncated factorization)
template <typename T>
ColumnID<T> column_id_rank(const DeviceMatrix<T> &a, int64_t k) {
    const int64_t kk = k < a.nrows() ? (k < a.ncols() ? k : a.ncols()) : (a.nrows() < a.ncols() ? a.nrows() : a.ncols());
    ColumnID<T> out{DeviceMatrix<T>(a.ctx(), a.nrows(), kk), DeviceMatrix<T>(a.ctx(), kk, a.ncols()), DeviceIndex(a.ctx(), (std::size_t)a.ncols())};
    a.ctx().check(Api<T>::column_id_rank(a.ctx().raw(), a.view(), kk, out.c.view(), out.z.view(), out.col_ind.data()));
    return out;
}
// the same unit for `count` small m x n matrices stacked in `a` (count * m rows, n columns) in one stream-ordered call, the rank of
// each chosen by tol (0: fixed rank k; rc_column_id_rank_batched_*): c is count * m x k, z count * k x n, col_ind count x n
template <typename T>
struct BatchedColumnID {
    DeviceMatrix<T> c, z;
    DeviceIndex col_ind, ranks;
};
template <typename T>
BatchedColumnID<T> column_id_rank_batched(const DeviceMatrix<T> &a, int32_t count, int64_t k, double tol = 0.0) {
    const int64_t m = count > 0 ? a.nrows() / count : 0, n = a.ncols();
    const int64_t kk = k < m ? (k < n ? k : n) : (m < n ? m : n);
    BatchedColumnID<T> out{DeviceMatrix<T>(a.ctx(), (int64_t)count * m, kk), DeviceMatrix<T>(a.ctx(), (int64_t)count * kk, n),
                           DeviceIndex(a.ctx(), (std::size_t)count * (std::size_t)n), DeviceIndex(a.ctx(), (std::size_t)count)};
    a.ctx().check(Api<T>::column_id_rank_batched(a.ctx().raw(), rc_matrix{a.view().data, m, n, n, 1}, m * n, count, k, tol,
                                                 rc_matrix{out.c.view().data, m, kk, kk, 1}, m * kk, rc_matrix{out.z.view().data, kk, n, n, 1},
                                                 kk * n, out.col_ind.data(), out.ranks.data()));
    return out;
}
// the one-pass randomized column ID of `count` tall m x n blocks stacked in `a` (rc_sketch_column_id_rank_batched_*): per block the sketch
// omega a_i (l x n; omega is l x m and shared by the batch) and the column ID of the sketch, C gathered from a_i: the projection of
// sample_range_by_rank (src/random_sampling.rs) followed by QR::compute_from_range_estimate + column_id (src/qr.rs:311-323).  m <= 65536,
// n <= 512, l <= 128; k is clamped to min(k, l, n).  The result is a BatchedColumnID, so apply_batched, to_mat_batched and
// recompress_batched and residual_batched take it; `sketch`, when given, receives the count * l x n sketches.  The complex entry points carry
// another stem (rc_sketch_column_id_rank_complex_batched_c64 / _c32: omega a with nothing conjugated), so the call is reached through its
// own dispatch rather than through Api<T>.
template <typename T> struct SketchApi;
template <> struct SketchApi<double> { static constexpr auto sketch_column_id_rank_batched = rc_sketch_column_id_rank_batched_f64; };
template <> struct SketchApi<float> { static constexpr auto sketch_column_id_rank_batched = rc_sketch_column_id_rank_batched_f32; };
template <> struct SketchApi<c64> { static constexpr auto sketch_column_id_rank_batched = rc_sketch_column_id_rank_complex_batched_c64; };
template <> struct SketchApi<c32> { static constexpr auto sketch_column_id_rank_batched = rc_sketch_column_id_rank_complex_batched_c32; };
template <typename T>
BatchedColumnID<T> column_id_rank_batched(const DeviceMatrix<T> &a, const DeviceMatrix<T> &omega, int32_t count, int64_t k, double tol = 0.0,
                                          DeviceMatrix<T> *sketch = nullptr) {
    const Context &ctx = a.ctx();
    const int64_t m = count > 0 ? a.nrows() / count : 0, n = a.ncols(), l = omega.nrows();
    const int64_t ln = l < n ? l : n, kk = k < ln ? k : ln;
    BatchedColumnID<T> out{DeviceMatrix<T>(ctx, (int64_t)count * m, kk), DeviceMatrix<T>(ctx, (int64_t)count * kk, n),
                           DeviceIndex(ctx, (std::size_t)count * (std::size_t)n), DeviceIndex(ctx, (std::size_t)count)};
    if (sketch) *sketch = DeviceMatrix<T>(ctx, (int64_t)count * l, n);
    ctx.check(SketchApi<T>::sketch_column_id_rank_batched(ctx.raw(), rc_matrix{a.view().data, m, n, n, 1}, m * n, omega.view(), 0, count, k, tol,
                                                          sketch ? rc_matrix{sketch->view().data, l, n, n, 1} : rc_matrix{nullptr, 0, 0, 0, 0}, l * n,
                                                          rc_matrix{out.c.view().data, m, kk, kk, 1}, m * kk,
                                                          rc_matrix{out.z.view().data, kk, n, n, 1}, kk * n, out.col_ind.data(), out.ranks.data()));
    return out;
}
// the two-sided ID A ~ C X R of the same batch in one call (rc_two_sided_id_rank_batched_*): c is count * m x k, x count * k x k,
// r count * k x n, row_ind count x m, col_ind count x n; r and col_ind are column_id_rank_batched's z and col_ind bit for bit
template <typename T>
struct BatchedTwoSidedID {
    DeviceMatrix<T> c, x, r;
    DeviceIndex row_ind, col_ind, ranks;
};
template <typename T>
BatchedTwoSidedID<T> two_sided_id_rank_batched(const DeviceMatrix<T> &a, int32_t count, int64_t k, double tol = 0.0) {
    const int64_t m = count > 0 ? a.nrows() / count : 0, n = a.ncols();
    const int64_t kk = k < m ? (k < n ? k : n) : (m < n ? m : n);
    BatchedTwoSidedID<T> out{DeviceMatrix<T>(a.ctx(), (int64_t)count * m, kk), DeviceMatrix<T>(a.ctx(), (int64_t)count * kk, kk),
                             DeviceMatrix<T>(a.ctx(), (int64_t)count * kk, n), DeviceIndex(a.ctx(), (std::size_t)count * (std::size_t)m),
                             DeviceIndex(a.ctx(), (std::size_t)count * (std::size_t)n), DeviceIndex(a.ctx(), (std::size_t)count)};
    a.ctx().check(Api<T>::two_sided_id_rank_batched(a.ctx().raw(), rc_matrix{a.view().data, m, n, n, 1}, m * n, count, k, tol,
                                                    rc_matrix{out.c.view().data, m, kk, kk, 1}, m * kk, rc_matrix{out.x.view().data, kk, kk, kk, 1},
                                                    kk * kk, rc_matrix{out.r.view().data, kk, n, n, 1}, kk * n, out.row_ind.data(),
                                                    out.col_ind.data(), out.ranks.data()));
    return out;
}
// truncated SVDs of the same batch in one call (rc_svd_rank_batched_*, every scalar type): u is count * m x k, s count x min(m, n)
// (all singular values, descending, in the real type), vt count * k x n (V^H for complex scalars); ranks[i] = the kept rank, the
// rows / columns past it zero
template <typename T>
struct BatchedSVD {
    DeviceMatrix<T> u;
    DeviceBuffer<typename Scalar<T>::real> s;
    DeviceMatrix<T> vt;
    DeviceIndex ranks;
};
template <typename T>
BatchedSVD<T> svd_rank_batched(const DeviceMatrix<T> &a, int32_t count, int64_t k, double tol = 0.0) {
    const int64_t m = count > 0 ? a.nrows() / count : 0, n = a.ncols(), p = m < n ? m : n;
    const int64_t kk = k < p ? k : p;
    BatchedSVD<T> out{DeviceMatrix<T>(a.ctx(), (int64_t)count * m, kk), DeviceBuffer<typename Scalar<T>::real>(a.ctx(), (std::size_t)count * (std::size_t)p),
                      DeviceMatrix<T>(a.ctx(), (int64_t)count * kk, n), DeviceIndex(a.ctx(), (std::size_t)count)};
    a.ctx().check(Api<T>::svd_rank_batched(a.ctx().raw(), rc_matrix{a.view().data, m, n, n, 1}, m * n, count, k, tol,
                                           rc_matrix{out.u.view().data, m, kk, kk, 1}, m * kk, out.s.data(), rc_matrix{out.vt.view().data, kk, n, n, 1},
                                           kk * n, out.ranks.data()));
    return out;
}
// apply (b: count * n x nrhs, block i in rows i n .. (i + 1) n - 1) or rebuild (b == nullptr) every block of a batch from its stacked
// factors in one rank-aware call (rc_lowrank_apply_batched_*; Apply::dot and to_mat, src/col_interp_decomp.rs:63-65, :134-154,
// src/two_sided_interp_decomp.rs:62-65, :159-170, src/svd.rs:42-55): left is count * m x k, right count * k x n, mid count * k x k or
// nullptr, s count x s_stride reals or nullptr, ranks count values or nullptr (every rank is k); returns y, count * m x nrhs (or n)
template <typename T>
DeviceMatrix<T> lowrank_apply_batched(const DeviceMatrix<T> &left, const DeviceMatrix<T> *mid, const DeviceBuffer<typename Scalar<T>::real> *s,
                                      const DeviceMatrix<T> &right, const DeviceIndex *ranks, int32_t count, const DeviceMatrix<T> *b) {
    const int64_t m = count > 0 ? left.nrows() / count : 0, k = left.ncols(), n = right.ncols();
    const int64_t ncols = b ? b->ncols() : n, p = s && count > 0 ? (int64_t)(s->size() / (std::size_t)count) : 0;
    DeviceMatrix<T> y(left.ctx(), (int64_t)count * m, ncols);
    const rc_matrix none{nullptr, 0, 0, 0, 0};
    left.ctx().check(Api<T>::lowrank_apply_batched(left.ctx().raw(), rc_matrix{left.view().data, m, k, k, 1}, m * k,
                                                   mid ? rc_matrix{mid->view().data, k, k, k, 1} : none, k * k, s ? s->data() : nullptr, p,
                                                   rc_matrix{right.view().data, k, n, n, 1}, k * n, ranks ? ranks->data() : nullptr, count,
                                                   b ? rc_matrix{b->view().data, n, ncols, ncols, 1} : none, n * ncols,
                                                   rc_matrix{y.view().data, m, ncols, ncols, 1}, m * ncols));
    return y;
}
// Mixed-precision storage of such a batch: the factors in f32 (c32) under f64 (c64) arithmetic (rc_lowrank_apply_mixed_batched_*,
// rc_demote_batched_*, rc_promote_batched_*).  T is the compute type, double or c64; Mixed<T>::storage the type the factors are kept in.
template <typename T> struct Mixed;
template <> struct Mixed<double> {
    using storage = float;
    static constexpr auto lowrank_apply_batched = rc_lowrank_apply_mixed_batched_f64;
    static constexpr auto demote_batched = rc_demote_batched_f64;
    static constexpr auto promote_batched = rc_promote_batched_f32;
};
template <> struct Mixed<c64> {
    using storage = c32;
    static constexpr auto lowrank_apply_batched = rc_lowrank_apply_mixed_batched_c64;
    static constexpr auto demote_batched = rc_demote_batched_c64;
    static constexpr auto promote_batched = rc_promote_batched_c32;
};
// the storage copy of a stack of count blocks (x is count * rows x cols), rounded to nearest even; overflow, when given, receives per
// block the number of finite elements that became infinite (count values)
template <typename T>
DeviceMatrix<typename Mixed<T>::storage> demote_batched(const DeviceMatrix<T> &x, int32_t count, DeviceIndex *overflow = nullptr) {
    const int64_t rows = count > 0 ? x.nrows() / count : 0, cols = x.ncols();
    DeviceMatrix<typename Mixed<T>::storage> out(x.ctx(), x.nrows(), cols);
    x.ctx().check(Mixed<T>::demote_batched(x.ctx().raw(), rc_matrix{x.view().data, rows, cols, cols, 1}, rows * cols, count,
                                           rc_matrix{out.view().data, rows, cols, cols, 1}, rows * cols, overflow ? overflow->data() : nullptr));
    return out;
}
// the exact way back
template <typename T>
DeviceMatrix<T> promote_batched(const DeviceMatrix<typename Mixed<T>::storage> &x, int32_t count) {
    const int64_t rows = count > 0 ? x.nrows() / count : 0, cols = x.ncols();
    DeviceMatrix<T> out(x.ctx(), x.nrows(), cols);
    x.ctx().check(Mixed<T>::promote_batched(x.ctx().raw(), rc_matrix{x.view().data, rows, cols, cols, 1}, rows * cols, count,
                                            rc_matrix{out.view().data, rows, cols, cols, 1}, rows * cols));
    return out;
}
// lowrank_apply_batched on factors in storage precision: the bits of lowrank_apply_batched<T> on promoted copies, half the factor bytes
template <typename T>
DeviceMatrix<T> lowrank_apply_batched_mixed(const DeviceMatrix<typename Mixed<T>::storage> &left, const DeviceMatrix<typename Mixed<T>::storage> *mid,
                                            const DeviceBuffer<double> *s, const DeviceMatrix<typename Mixed<T>::storage> &right,
                                            const DeviceIndex *ranks, int32_t count, const DeviceMatrix<T> *b) {
    const int64_t m = count > 0 ? left.nrows() / count : 0, k = left.ncols(), n = right.ncols();
    const int64_t ncols = b ? b->ncols() : n, p = s && count > 0 ? (int64_t)(s->size() / (std::size_t)count) : 0;
    DeviceMatrix<T> y(left.ctx(), (int64_t)count * m, ncols);
    const rc_matrix none{nullptr, 0, 0, 0, 0};
    left.ctx().check(Mixed<T>::lowrank_apply_batched(left.ctx().raw(), rc_matrix{left.view().data, m, k, k, 1}, m * k,
                                                     mid ? rc_matrix{mid->view().data, k, k, k, 1} : none, k * k, s ? s->data() : nullptr, p,
                                                     rc_matrix{right.view().data, k, n, n, 1}, k * n, ranks ? ranks->data() : nullptr, count,
                                                     b ? rc_matrix{b->view().data, n, ncols, ncols, 1} : none, n * ncols,
                                                     rc_matrix{y.view().data, m, ncols, ncols, 1}, m * ncols));
    return y;
}
// Apply::dot and to_mat of the three batched decompositions, each block at its own rank
template <typename T>
DeviceMatrix<T> apply_batched(const BatchedColumnID<T> &id, const DeviceMatrix<T> &b) {
    return lowrank_apply_batched<T>(id.c, nullptr, nullptr, id.z, &id.ranks, (int32_t)id.ranks.size(), &b);
}
template <typename T>
DeviceMatrix<T> to_mat_batched(const BatchedColumnID<T> &id) {
    return lowrank_apply_batched<T>(id.c, nullptr, nullptr, id.z, &id.ranks, (int32_t)id.ranks.size(), nullptr);
}
template <typename T>
DeviceMatrix<T> apply_batched(const BatchedTwoSidedID<T> &id, const DeviceMatrix<T> &b) {
    return lowrank_apply_batched<T>(id.c, &id.x, nullptr, id.r, &id.ranks, (int32_t)id.ranks.size(), &b);
}
template <typename T>
DeviceMatrix<T> to_mat_batched(const BatchedTwoSidedID<T> &id) {
    return lowrank_apply_batched<T>(id.c, &id.x, nullptr, id.r, &id.ranks, (int32_t)id.ranks.size(), nullptr);
}
template <typename T>
DeviceMatrix<T> apply_batched(const BatchedSVD<T> &svd, const DeviceMatrix<T> &b) {
    return lowrank_apply_batched<T>(svd.u, nullptr, &svd.s, svd.vt, &svd.ranks, (int32_t)svd.ranks.size(), &b);
}
template <typename T>
DeviceMatrix<T> to_mat_batched(const BatchedSVD<T> &svd) {
    return lowrank_apply_batched<T>(svd.u, nullptr, &svd.s, svd.vt, &svd.ranks, (int32_t)svd.ranks.size(), nullptr);
}
// recompress every factor pair of a batch to a truncated SVD without forming the blocks (rc_lowrank_recompress_batched_* for the real
// scalars, rc_lowrank_recompress_complex_batched_* for c64 and c32; the scheme of SVD::to_qr / compute_from_range_estimate,
// src/svd.rs:150-163, :171-, with compress's rank rule, :60-101).  The entry point is reached through its own dispatch: the complex
// pair has a stem of its own (see the C header) and takes tol in the real type of the data.  left is count * m x K, right
// count * K x n, mid count * K x K or nullptr, s count x s_stride reals or nullptr, ranks count inner ranks or nullptr (every rank is
// K); K <= min(m, n).  Returns u (count * m x kk), s (count x K, the real type: the singular values of each block, then zeros), vt
// (count * kk x n; V^H for complex scalars, nothing else is conjugated) and the new ranks, kk = min(k, K).
template <typename T> struct RecompressApi;
template <> struct RecompressApi<double> { using tol_type = double; static constexpr auto lowrank_recompress_batched = rc_lowrank_recompress_batched_f64; };
template <> struct RecompressApi<float> { using tol_type = double; static constexpr auto lowrank_recompress_batched = rc_lowrank_recompress_batched_f32; };
template <> struct RecompressApi<c64> { using tol_type = double; static constexpr auto lowrank_recompress_batched = rc_lowrank_recompress_complex_batched_c64; };
template <> struct RecompressApi<c32> { using tol_type = float; static constexpr auto lowrank_recompress_batched = rc_lowrank_recompress_complex_batched_c32; };
// the calls for a tall left factor (m <= 65536): rc_lowrank_recompress_tall_batched_* and rc_lowrank_recompress_tall_complex_batched_*, the same
// signatures and contracts (tol's type is RecompressApi<T>::tol_type)
template <typename T> struct RecompressTallApi;
template <> struct RecompressTallApi<double> { static constexpr auto lowrank_recompress_batched = rc_lowrank_recompress_tall_batched_f64; };
template <> struct RecompressTallApi<float> { static constexpr auto lowrank_recompress_batched = rc_lowrank_recompress_tall_batched_f32; };
template <> struct RecompressTallApi<c64> { static constexpr auto lowrank_recompress_batched = rc_lowrank_recompress_tall_complex_batched_c64; };
template <> struct RecompressTallApi<c32> { static constexpr auto lowrank_recompress_batched = rc_lowrank_recompress_tall_complex_batched_c32; };
// the call both recompress_batched and recompress_tall_batched make, on the entry point `fn` of their dispatch
template <typename T, typename Tol, typename Fn>
BatchedSVD<T> recompress_batched_through(Fn fn, const DeviceMatrix<T> &left, const DeviceMatrix<T> *mid, const DeviceBuffer<typename Scalar<T>::real> *s,
                                         const DeviceMatrix<T> &right, const DeviceIndex *ranks, int32_t count, int64_t k, double tol) {
    const Context &ctx = left.ctx();
    const int64_t m = count > 0 ? left.nrows() / count : 0, kin = left.ncols(), n = right.ncols();
    const int64_t kk = k < kin ? k : kin, p = s && count > 0 ? (int64_t)(s->size() / (std::size_t)count) : 0;
    BatchedSVD<T> out{DeviceMatrix<T>(ctx, (int64_t)count * m, kk), DeviceBuffer<typename Scalar<T>::real>(ctx, (std::size_t)count * (std::size_t)kin),
                      DeviceMatrix<T>(ctx, (int64_t)count * kk, n), DeviceIndex(ctx, (std::size_t)count)};
    const rc_matrix none{nullptr, 0, 0, 0, 0};
    ctx.check(fn(ctx.raw(), rc_matrix{left.view().data, m, kin, kin, 1}, m * kin, mid ? rc_matrix{mid->view().data, kin, kin, kin, 1} : none, kin * kin,
                 s ? s->data() : nullptr, p, rc_matrix{right.view().data, kin, n, n, 1}, kin * n, ranks ? ranks->data() : nullptr, count, k, (Tol)tol,
                 rc_matrix{out.u.view().data, m, kk, kk, 1}, m * kk, out.s.data(), rc_matrix{out.vt.view().data, kk, n, n, 1}, kk * n, out.ranks.data()));
    return out;
}
template <typename T>
BatchedSVD<T> recompress_batched(const DeviceMatrix<T> &left, const DeviceMatrix<T> *mid, const DeviceBuffer<typename Scalar<T>::real> *s,
                                 const DeviceMatrix<T> &right, const DeviceIndex *ranks, int32_t count, int64_t k, double tol = 0.0) {
    return recompress_batched_through<T, typename RecompressApi<T>::tol_type>(RecompressApi<T>::lowrank_recompress_batched, left, mid, s, right, ranks, count, k,
                                                                              tol);
}
// the same for factor pairs whose left factor is tall (m <= 65536, n <= 512; every scalar type): the SVD end of the sketched
// column_id_rank_batched.  For m <= 512 the result is recompress_batched's bit for bit.
template <typename T>
BatchedSVD<T> recompress_tall_batched(const DeviceMatrix<T> &left, const DeviceMatrix<T> *mid, const DeviceBuffer<typename Scalar<T>::real> *s,
                                      const DeviceMatrix<T> &right, const DeviceIndex *ranks, int32_t count, int64_t k, double tol = 0.0) {
    return recompress_batched_through<T, typename RecompressApi<T>::tol_type>(RecompressTallApi<T>::lowrank_recompress_batched, left, mid, s, right, ranks, count,
                                                                              k, tol);
}
template <typename T>
BatchedSVD<T> recompress_tall_batched(const BatchedColumnID<T> &id, int64_t k, double tol = 0.0) {
    return recompress_tall_batched<T>(id.c, nullptr, nullptr, id.z, &id.ranks, (int32_t)id.ranks.size(), k, tol);
}
// the same for factor pairs with both factors tall (m, n <= 65536; rc_lowrank_recompress_large_batched_f64 / _f32 for the real scalars): rounded
// addition, ID -> SVD conversion and re-truncation of blocks large on both sides.  For n <= 512 the result is recompress_tall_batched's bit for bit.
inline BatchedSVD<double> recompress_large_batched(const DeviceMatrix<double> &left, const DeviceMatrix<double> *mid, const DeviceBuffer<double> *s,
                                                   const DeviceMatrix<double> &right, const DeviceIndex *ranks, int32_t count, int64_t k, double tol = 0.0) {
    return recompress_batched_through<double, double>(rc_lowrank_recompress_large_batched_f64, left, mid, s, right, ranks, count, k, tol);
}
inline BatchedSVD<float> recompress_large_batched(const DeviceMatrix<float> &left, const DeviceMatrix<float> *mid, const DeviceBuffer<float> *s,
                                                  const DeviceMatrix<float> &right, const DeviceIndex *ranks, int32_t count, int64_t k, double tol = 0.0) {
    return recompress_batched_through<float, double>(rc_lowrank_recompress_large_batched_f32, left, mid, s, right, ranks, count, k, tol);
}
// the complex pair (rc_lowrank_recompress_complex_large_batched_c64 / _c32: "complex" before "large", see the C header): s and the singular
// values real, vt = V^H, tol in the real type of the data.  For n <= 512 the result is recompress_tall_batched's bit for bit.
inline BatchedSVD<c64> recompress_large_batched(const DeviceMatrix<c64> &left, const DeviceMatrix<c64> *mid, const DeviceBuffer<double> *s,
                                                const DeviceMatrix<c64> &right, const DeviceIndex *ranks, int32_t count, int64_t k, double tol = 0.0) {
    return recompress_batched_through<c64, double>(rc_lowrank_recompress_complex_large_batched_c64, left, mid, s, right, ranks, count, k, tol);
}
inline BatchedSVD<c32> recompress_large_batched(const DeviceMatrix<c32> &left, const DeviceMatrix<c32> *mid, const DeviceBuffer<float> *s,
                                                const DeviceMatrix<c32> &right, const DeviceIndex *ranks, int32_t count, int64_t k, double tol = 0.0) {
    return recompress_batched_through<c32, float>(rc_lowrank_recompress_complex_large_batched_c32, left, mid, s, right, ranks, count, k, tol);
}
// one range step of a power iteration on `count` tall m x n blocks stacked in `a` (rc_sketch_range_step_batched_* for the real scalars,
// rc_sketch_range_step_complex_batched_* for c64 and c32): per block the sketch omega a_i (l x n), an orthonormal basis q_i (l x n) of its rows
// (q_i q_i^H = I) and the projection p_i = a_i q_i^H (m x l); q is count * l x n, p count * m x l, ranks[i] the number of nonzero rows of q_i.
// `sketch`, when given, receives the count * l x n sketches.  The _view form takes block 0's test matrix as a view and its batch stride
// (0: shared), so that a strided U^T can be the next omega without a copy.  conj_p (complex scalars; the real calls have nothing to
// conjugate and ignore it): p receives conj(p_i), whose orthonormal basis from recompress_tall is conj(U), so that its plain transpose is
// the U^H a power iteration continues with (see the C header).
template <typename T> struct RangeStepApi;
template <> struct RangeStepApi<double> {
    using tol_type = double;
    static rc_status range_step(rc_context *ctx, rc_matrix a, int64_t abs, rc_matrix omega, int64_t obs, int32_t count, rc_matrix y, int64_t ybs, rc_matrix q,
                                int64_t qbs, rc_matrix p, int64_t pbs, int64_t *ranks, int32_t) {
        return rc_sketch_range_step_batched_f64(ctx, a, abs, omega, obs, count, y, ybs, q, qbs, p, pbs, ranks);
    }
    static constexpr auto sketch_id = rc_sketch_column_id_rank_batched_f64;
    static constexpr auto recompress_tall = rc_lowrank_recompress_tall_batched_f64;
};
template <> struct RangeStepApi<float> {
    using tol_type = double;
    static rc_status range_step(rc_context *ctx, rc_matrix a, int64_t abs, rc_matrix omega, int64_t obs, int32_t count, rc_matrix y, int64_t ybs, rc_matrix q,
                                int64_t qbs, rc_matrix p, int64_t pbs, int64_t *ranks, int32_t) {
        return rc_sketch_range_step_batched_f32(ctx, a, abs, omega, obs, count, y, ybs, q, qbs, p, pbs, ranks);
    }
    static constexpr auto sketch_id = rc_sketch_column_id_rank_batched_f32;
    static constexpr auto recompress_tall = rc_lowrank_recompress_tall_batched_f32;
};
template <> struct RangeStepApi<c64> {
    using tol_type = double;
    static constexpr auto range_step = rc_sketch_range_step_complex_batched_c64;
    static constexpr auto sketch_id = rc_sketch_column_id_rank_complex_batched_c64;
    static constexpr auto recompress_tall = rc_lowrank_recompress_tall_complex_batched_c64;
};
template <> struct RangeStepApi<c32> {
    using tol_type = float;
    static constexpr auto range_step = rc_sketch_range_step_complex_batched_c32;
    static constexpr auto sketch_id = rc_sketch_column_id_rank_complex_batched_c32;
    static constexpr auto recompress_tall = rc_lowrank_recompress_tall_complex_batched_c32;
};
template <typename T>
struct BatchedRangeStep {
    DeviceMatrix<T> q, p;
    DeviceIndex ranks;
};
template <typename T>
BatchedRangeStep<T> range_step_batched_view(const DeviceMatrix<T> &a, rc_matrix omega, int64_t omega_batch_stride, int32_t count,
                                            DeviceMatrix<T> *sketch = nullptr, bool conj_p = false) {
    const Context &ctx = a.ctx();
    const int64_t m = count > 0 ? a.nrows() / count : 0, n = a.ncols(), l = omega.rows;
    BatchedRangeStep<T> out{DeviceMatrix<T>(ctx, (int64_t)count * l, n), DeviceMatrix<T>(ctx, (int64_t)count * m, l), DeviceIndex(ctx, (std::size_t)count)};
    if (sketch) *sketch = DeviceMatrix<T>(ctx, (int64_t)count * l, n);
    ctx.check(RangeStepApi<T>::range_step(ctx.raw(), rc_matrix{a.view().data, m, n, n, 1}, m * n, omega, omega_batch_stride, count,
                                          sketch ? rc_matrix{sketch->view().data, l, n, n, 1} : rc_matrix{nullptr, 0, 0, 0, 0}, l * n,
                                          rc_matrix{out.q.view().data, l, n, n, 1}, l * n, rc_matrix{out.p.view().data, m, l, l, 1}, m * l,
                                          out.ranks.data(), conj_p ? 1 : 0));
    return out;
}
template <typename T>
BatchedRangeStep<T> range_step_batched(const DeviceMatrix<T> &a, const DeviceMatrix<T> &omega, int32_t count, DeviceMatrix<T> *sketch = nullptr,
                                       bool conj_p = false) {
    return range_step_batched_view(a, omega.view(), 0, count, sketch, conj_p);
}
// the sketched column_id_rank_batched after `iterations` rounds of power iteration on the shared test matrix omega (l x m), both half-steps
// orthonormalised as in sample_range_power_iteration (src/random_sampling.rs:131-158): per round the range step (with conj_p, which only the
// complex scalars act on), then p orthonormalised by rc_lowrank_recompress_tall_batched_* / _tall_complex_batched_* with right = I at the
// step's ranks, whose u^T (a strided view; U^H of p's basis for complex scalars) is the next, per-block, omega; two
// launches per round and one for the ID.  The C calls never synchronise; this mirror owns the intermediate buffers, so it waits once per
// round before it releases them.  iterations = 0 is column_id_rank_batched(a, omega, ...).
template <typename T>
BatchedColumnID<T> column_id_rank_power_batched(const DeviceMatrix<T> &a, const DeviceMatrix<T> &omega, int32_t count, int64_t k, double tol = 0.0,
                                                int iterations = 1, DeviceMatrix<T> *sketch = nullptr) {
    if (iterations <= 0) return column_id_rank_batched(a, omega, count, k, tol, sketch);
    const Context &ctx = a.ctx();
    const int64_t m = count > 0 ? a.nrows() / count : 0, n = a.ncols(), l = omega.nrows();
    std::vector<T> heye((std::size_t)(l * l), (T)0);
    for (int64_t i = 0; i < l; ++i) heye[(std::size_t)(i * l + i)] = (T)1;
    const DeviceMatrix<T> eye = DeviceMatrix<T>::from_host(ctx, heye.data(), l, l);
    DeviceMatrix<T> u(ctx, (int64_t)count * m, l), vt(ctx, (int64_t)count * l, l);
    DeviceBuffer<typename Scalar<T>::real> s(ctx, (std::size_t)count * (std::size_t)l);
    DeviceIndex uranks(ctx, (std::size_t)count);
    rc_matrix om = omega.view();
    int64_t obs = 0;
    for (int it = 0; it < iterations; ++it) {
        const BatchedRangeStep<T> step = range_step_batched_view<T>(a, om, obs, count, nullptr, true);
        DeviceMatrix<T> un(ctx, (int64_t)count * m, l);
        ctx.check(RangeStepApi<T>::recompress_tall(ctx.raw(), rc_matrix{step.p.view().data, m, l, l, 1}, m * l, rc_matrix{nullptr, 0, 0, 0, 0}, 0, nullptr, 0,
                                                   rc_matrix{eye.view().data, l, l, l, 1}, 0, step.ranks.data(), count, l, (typename RangeStepApi<T>::tol_type)0,
                                                   rc_matrix{un.view().data, m, l, l, 1}, m * l, s.data(), rc_matrix{vt.view().data, l, l, l, 1}, l * l,
                                                   uranks.data()));
        ctx.synchronize();  // step's buffers and the previous u are released here
        u = std::move(un);
        om = rc_matrix{u.view().data, l, m, 1, l};
        obs = m * l;
    }
    const int64_t ln = l < n ? l : n, kk = k < ln ? k : ln;
    BatchedColumnID<T> out{DeviceMatrix<T>(ctx, (int64_t)count * m, kk), DeviceMatrix<T>(ctx, (int64_t)count * kk, n),
                           DeviceIndex(ctx, (std::size_t)count * (std::size_t)n), DeviceIndex(ctx, (std::size_t)count)};
    if (sketch) *sketch = DeviceMatrix<T>(ctx, (int64_t)count * l, n);
    ctx.check(RangeStepApi<T>::sketch_id(ctx.raw(), rc_matrix{a.view().data, m, n, n, 1}, m * n, om, obs, count, k, tol,
                                         sketch ? rc_matrix{sketch->view().data, l, n, n, 1} : rc_matrix{nullptr, 0, 0, 0, 0}, l * n,
                                         rc_matrix{out.c.view().data, m, kk, kk, 1}, m * kk, rc_matrix{out.z.view().data, kk, n, n, 1}, kk * n,
                                         out.col_ind.data(), out.ranks.data()));
    ctx.synchronize();  // u, the last omega, is released on return
    return out;
}
// the sketch omega a_i of `count` m x n blocks stacked in `a` and nothing else (rc_sketch_product_batched_f64 / _f32, real scalars only), for
// blocks of up to 65536 columns: count * l x n, with the bits of the sketch the two calls above form (see the C header).  The _view form takes
// block 0 of every operand as a view with its batch stride, so that the projection p = a q^T is the same call on transposed views.
template <typename T> struct SketchProductApi;
template <> struct SketchProductApi<double> {
    static constexpr auto product = rc_sketch_product_batched_f64;
    static constexpr auto recompress_tall = rc_lowrank_recompress_tall_batched_f64;
};
template <> struct SketchProductApi<float> {
    static constexpr auto product = rc_sketch_product_batched_f32;
    static constexpr auto recompress_tall = rc_lowrank_recompress_tall_batched_f32;
};
template <typename T>
void sketch_product_batched_view(const Context &ctx, rc_matrix a, int64_t a_batch_stride, rc_matrix omega, int64_t omega_batch_stride, int32_t count,
                                 rc_matrix y, int64_t y_batch_stride) {
    ctx.check(SketchProductApi<T>::product(ctx.raw(), a, a_batch_stride, omega, omega_batch_stride, count, y, y_batch_stride));
}
template <typename T>
DeviceMatrix<T> sketch_product_batched(const DeviceMatrix<T> &a, const DeviceMatrix<T> &omega, int32_t count) {
    const Context &ctx = a.ctx();
    const int64_t m = count > 0 ? a.nrows() / count : 0, n = a.ncols(), l = omega.nrows();
    DeviceMatrix<T> y(ctx, (int64_t)count * l, n);
    sketch_product_batched_view<T>(ctx, rc_matrix{a.view().data, m, n, n, 1}, m * n, omega.view(), 0, count, rc_matrix{y.view().data, l, n, n, 1}, l * n);
    return y;
}
// the l x l identity on the device (the `right` of an orthonormalising tall recompression)
template <typename T>
DeviceMatrix<T> device_identity(const Context &ctx, int64_t l) {
    std::vector<T> heye((std::size_t)(l * l), (T)0);
    for (int64_t i = 0; i < l; ++i) heye[(std::size_t)(i * l + i)] = (T)1;
    return DeviceMatrix<T>::from_host(ctx, heye.data(), l, l);
}
// range_step_batched for blocks of any width (m, n <= 65536, l <= min(128, m, n); real scalars): n <= 512 is range_step_batched_view; above
// it three launches: the sketch by sketch_product_batched, its row basis by rc_lowrank_recompress_tall_batched_* on the transposed view of the
// sketch with right = I, k = l, tol = 0 (u written through the transposed view of q, the ranks that call's), and p = a q^T by the product on
// transposed views.  The mirror owns the sketch, so it waits once before it releases it.  `identity`, when given, is the l x l identity of a
// caller that makes several steps (else one is made here).
template <typename T>
BatchedRangeStep<T> range_step_large_batched_view(const DeviceMatrix<T> &a, rc_matrix omega, int64_t omega_batch_stride, int32_t count,
                                                  const DeviceMatrix<T> *identity = nullptr) {
    const Context &ctx = a.ctx();
    const int64_t m = count > 0 ? a.nrows() / count : 0, n = a.ncols(), l = omega.rows;
    if (n <= 512) return range_step_batched_view<T>(a, omega, omega_batch_stride, count);
    BatchedRangeStep<T> out{DeviceMatrix<T>(ctx, (int64_t)count * l, n), DeviceMatrix<T>(ctx, (int64_t)count * m, l), DeviceIndex(ctx, (std::size_t)count)};
    DeviceMatrix<T> y(ctx, (int64_t)count * l, n), vt(ctx, (int64_t)count * l, l);
    DeviceBuffer<T> s(ctx, (std::size_t)count * (std::size_t)l);
    DeviceMatrix<T> own;
    if (!identity) own = device_identity<T>(ctx, l);
    const DeviceMatrix<T> &eye = identity ? *identity : own;
    const rc_matrix av{a.view().data, m, n, n, 1}, none{nullptr, 0, 0, 0, 0};
    sketch_product_batched_view<T>(ctx, av, m * n, omega, omega_batch_stride, count, rc_matrix{y.view().data, l, n, n, 1}, l * n);
    ctx.check(SketchProductApi<T>::recompress_tall(ctx.raw(), rc_matrix{y.view().data, n, l, 1, n}, l * n, none, 0, nullptr, 0,
                                                   rc_matrix{eye.view().data, l, l, l, 1}, 0, nullptr, count, l, 0.0, rc_matrix{out.q.view().data, n, l, 1, n}, l * n,
                                                   s.data(), rc_matrix{vt.view().data, l, l, l, 1}, l * l, out.ranks.data()));
    sketch_product_batched_view<T>(ctx, rc_matrix{a.view().data, n, m, 1, n}, m * n, rc_matrix{out.q.view().data, l, n, n, 1}, l * n, count,
                                   rc_matrix{out.p.view().data, l, m, 1, l}, m * l);
    ctx.synchronize();  // y, vt, s and eye are released on return
    return out;
}
template <typename T>
BatchedRangeStep<T> range_step_large_batched(const DeviceMatrix<T> &a, const DeviceMatrix<T> &omega, int32_t count) {
    return range_step_large_batched_view<T>(a, omega.view(), 0, count);
}
// batched randomized SVDs of blocks of any width with `steps` >= 1 range steps on the shared test matrix omega (l x m): per step
// range_step_large_batched; between steps p orthonormalised by the tall recompression with right = I at the step's ranks, whose u^T (a
// strided view) is the next, per-block, omega; then recompress_large_batched(p, q, ranks, k, tol).  n <= 512 takes the same calls with the
// one-launch range step, as the Python sketch_svd_rank_power_batched does.
template <typename T>
BatchedSVD<T> svd_rank_large_batched(const DeviceMatrix<T> &a, const DeviceMatrix<T> &omega, int32_t count, int64_t k, double tol = 0.0, int steps = 1) {
    const Context &ctx = a.ctx();
    if (steps < 1) throw std::invalid_argument("svd_rank_large_batched: steps must be >= 1 (the one-pass column ID route needs n <= 512)");
    const int64_t m = count > 0 ? a.nrows() / count : 0, l = omega.nrows();
    const DeviceMatrix<T> eye = device_identity<T>(ctx, l);
    DeviceMatrix<T> u;  // the orthonormalised p of the step before, whose transposed view is the next omega (none before the first step)
    rc_matrix om = omega.view();
    int64_t obs = 0;
    for (int it = 0;; ++it) {
        const BatchedRangeStep<T> step = range_step_large_batched_view<T>(a, om, obs, count, &eye);
        if (it + 1 == steps) {
            BatchedSVD<T> out = recompress_large_batched(step.p, nullptr, nullptr, step.q, &step.ranks, count, k, tol);
            ctx.synchronize();  // step's buffers and u, the last omega, are released on return
            return out;
        }
        DeviceMatrix<T> un(ctx, (int64_t)count * m, l), vt(ctx, (int64_t)count * l, l);
        DeviceBuffer<T> s(ctx, (std::size_t)count * (std::size_t)l);
        DeviceIndex uranks(ctx, (std::size_t)count);
        ctx.check(SketchProductApi<T>::recompress_tall(ctx.raw(), rc_matrix{step.p.view().data, m, l, l, 1}, m * l, rc_matrix{nullptr, 0, 0, 0, 0}, 0, nullptr, 0,
                                                       rc_matrix{eye.view().data, l, l, l, 1}, 0, step.ranks.data(), count, l, 0.0,
                                                       rc_matrix{un.view().data, m, l, l, 1}, m * l, s.data(), rc_matrix{vt.view().data, l, l, l, 1}, l * l,
                                                       uranks.data()));
        ctx.synchronize();  // step's buffers, vt, s and the previous u are released here
        u = std::move(un);
        om = rc_matrix{u.view().data, l, m, 1, l};
        obs = m * l;
    }
}
// a batched column ID, a batched two-sided ID as truncated SVDs, each block from its own rank
template <typename T>
BatchedSVD<T> recompress_batched(const BatchedColumnID<T> &id, int64_t k, double tol = 0.0) {
    return recompress_batched<T>(id.c, nullptr, nullptr, id.z, &id.ranks, (int32_t)id.ranks.size(), k, tol);
}
template <typename T>
BatchedSVD<T> recompress_batched(const BatchedTwoSidedID<T> &id, int64_t k, double tol = 0.0) {
    return recompress_batched<T>(id.c, &id.x, nullptr, id.r, &id.ranks, (int32_t)id.ranks.size(), k, tol);
}
// rounded addition: the truncated SVD of a_i + b_i per block, from the factors [U_a U_b] diag(s_a, s_b) [Vt_a; Vt_b] of inner width
// k_a + k_b (<= min(m, n)).  The three concatenations are batched strided copies on the device (the batched apply with an identity
// factor copies bit for bit; the real s of complex factors goes through the real apply); the zero columns the batched SVD leaves past a
// block's rank come out as exactly zero singular values.
template <typename T>
BatchedSVD<T> recompress_batched(const BatchedSVD<T> &a, const BatchedSVD<T> &b, int64_t k, double tol = 0.0) {
    const Context &ctx = a.u.ctx();
    const int32_t count = (int32_t)a.ranks.size();
    const int64_t m = count > 0 ? a.u.nrows() / count : 0, n = a.vt.ncols(), ka = a.u.ncols(), kb = b.u.ncols(), kin = ka + kb;
    const int64_t pa = count > 0 ? (int64_t)(a.s.size() / (std::size_t)count) : 0, pb = count > 0 ? (int64_t)(b.s.size() / (std::size_t)count) : 0;
    const int64_t ke = ka > kb ? ka : kb;
    std::vector<T> heye((std::size_t)(ke * ke), (T)0);
    for (int64_t i = 0; i < ke; ++i) heye[(std::size_t)(i * ke + i)] = (T)1;
    const auto eye = DeviceMatrix<T>::from_host(ctx, heye.data(), ke, ke);
    DeviceMatrix<T> left(ctx, (int64_t)count * m, kin), right(ctx, (int64_t)count * kin, n);
    using Real = typename Scalar<T>::real;
    const Real hone = (Real)1;
    const auto one = DeviceMatrix<Real>::from_host(ctx, &hone, 1, 1);
    DeviceBuffer<Real> s(ctx, (std::size_t)count * (std::size_t)kin);
    const rc_matrix none{nullptr, 0, 0, 0, 0};
    // dst block (rows x cols, row stride drs, batch stride dbs) = lf (rows x r) rt (r x cols): one of the two is the identity
    auto copy = [&](rc_matrix lf, int64_t lbs, rc_matrix rt, int64_t rbs, T *dst, int64_t drs, int64_t dbs) {
        ctx.check(Api<T>::lowrank_apply_batched(ctx.raw(), lf, lbs, none, 0, nullptr, 0, rt, rbs, nullptr, count, none, 0,
                                                rc_matrix{dst, lf.rows, rt.cols, drs, 1}, dbs));
    };
    auto copy_s = [&](const Real *src, int64_t ks, int64_t ps, Real *dst) {  // dst row (1 x ks of kin) = [1] src row (1 x ks of ps)
        ctx.check(Api<Real>::lowrank_apply_batched(ctx.raw(), rc_matrix{one.view().data, 1, 1, 1, 1}, 0, none, 0, nullptr, 0,
                                                   rc_matrix{const_cast<Real *>(src), 1, ks, ps, 1}, ps, nullptr, count, none, 0,
                                                   rc_matrix{dst, 1, ks, kin, 1}, kin));
    };
    auto id = [&](int64_t r) { return rc_matrix{eye.view().data, r, r, ke, 1}; };
    T *lp = static_cast<T *>(left.view().data), *rp = static_cast<T *>(right.view().data);
    copy(rc_matrix{a.u.view().data, m, ka, ka, 1}, m * ka, id(ka), 0, lp, kin, m * kin);
    copy(rc_matrix{b.u.view().data, m, kb, kb, 1}, m * kb, id(kb), 0, lp + ka, kin, m * kin);
    copy(id(ka), 0, rc_matrix{a.vt.view().data, ka, n, n, 1}, ka * n, rp, n, kin * n);
    copy(id(kb), 0, rc_matrix{b.vt.view().data, kb, n, n, 1}, kb * n, rp + ka * n, n, kin * n);
    copy_s(a.s.data(), ka, pa, s.data());
    copy_s(b.s.data(), kb, pb, s.data() + ka);
    auto out = recompress_batched<T>(left, nullptr, &s, right, nullptr, count, k, tol);
    ctx.synchronize();  // eye, one, left, right and s are freed on return
    return out;
}
// the residual of every block of a batch against its stacked factors in one rank-aware call (rc_lowrank_residual_batched_*): per block the
// reference's rel_diff_fro(x.to_mat(), a) without the rebuilt block, on the domain of the sketched column ID (m <= 65536, n <= 512, K <= 128).
// a is count * m x n, the factors as in lowrank_apply_batched.  err[i] = ||a_i - left_i mid_i diag(s_i) right_i||_F at the block's rank,
// nrm[i] = ||a_i||_F, and with want_residual e (count * m x n) holds the residual blocks (else it is empty).  Every scalar type: for c64 and c32
// s, err and nrm are of the real type and nothing is conjugated (vt is V^H, as svd_rank_batched returns it).  The entry point is reached through
// its own dispatch, like the recompression's: Api<T> keeps the members every scalar type has had from the start.
template <typename T> struct ResidualApi;
template <> struct ResidualApi<double> { static constexpr auto lowrank_residual_batched = rc_lowrank_residual_batched_f64; };
template <> struct ResidualApi<float> { static constexpr auto lowrank_residual_batched = rc_lowrank_residual_batched_f32; };
template <> struct ResidualApi<c64> { static constexpr auto lowrank_residual_batched = rc_lowrank_residual_batched_c64; };
template <> struct ResidualApi<c32> { static constexpr auto lowrank_residual_batched = rc_lowrank_residual_batched_c32; };
template <typename T>
struct BatchedResidual {
    DeviceBuffer<typename Scalar<T>::real> err, nrm;
    DeviceMatrix<T> e;
    bool has_e = false;
};
template <typename T>
BatchedResidual<T> lowrank_residual_batched(const DeviceMatrix<T> &a, const DeviceMatrix<T> &left, const DeviceMatrix<T> *mid,
                                            const DeviceBuffer<typename Scalar<T>::real> *s, const DeviceMatrix<T> &right, const DeviceIndex *ranks,
                                            int32_t count, bool want_residual = false) {
    using Real = typename Scalar<T>::real;
    const Context &ctx = a.ctx();
    const int64_t m = count > 0 ? a.nrows() / count : 0, n = a.ncols(), k = left.ncols();
    const int64_t p = s && count > 0 ? (int64_t)(s->size() / (std::size_t)count) : 0;
    BatchedResidual<T> out{DeviceBuffer<Real>(ctx, (std::size_t)count), DeviceBuffer<Real>(ctx, (std::size_t)count),
                           want_residual ? DeviceMatrix<T>(ctx, (int64_t)count * m, n) : DeviceMatrix<T>(), want_residual};
    if (count == 0) return out;  // an empty batch is a no-op (the block shape cannot be read off an empty stack)
    const rc_matrix none{nullptr, 0, 0, 0, 0};
    ctx.check(ResidualApi<T>::lowrank_residual_batched(ctx.raw(), rc_matrix{a.view().data, m, n, n, 1}, m * n, rc_matrix{left.view().data, m, k, k, 1},
                                                       m * k, mid ? rc_matrix{mid->view().data, k, k, k, 1} : none, k * k, s ? s->data() : nullptr, p,
                                                       rc_matrix{right.view().data, k, n, n, 1}, k * n, ranks ? ranks->data() : nullptr, count,
                                                       want_residual ? rc_matrix{out.e.view().data, m, n, n, 1} : none, m * n, out.err.data(),
                                                       out.nrm.data()));
    return out;
}
// the three batched decompositions against the blocks they were computed from, each block at its own rank
template <typename T>
BatchedResidual<T> residual_batched(const BatchedColumnID<T> &id, const DeviceMatrix<T> &a, bool want_residual = false) {
    return lowrank_residual_batched<T>(a, id.c, nullptr, nullptr, id.z, &id.ranks, (int32_t)id.ranks.size(), want_residual);
}
template <typename T>
BatchedResidual<T> residual_batched(const BatchedTwoSidedID<T> &id, const DeviceMatrix<T> &a, bool want_residual = false) {
    return lowrank_residual_batched<T>(a, id.c, &id.x, nullptr, id.r, &id.ranks, (int32_t)id.ranks.size(), want_residual);
}
template <typename T>
BatchedResidual<T> residual_batched(const BatchedSVD<T> &svd, const DeviceMatrix<T> &a, bool want_residual = false) {
    return lowrank_residual_batched<T>(a, svd.u, nullptr, &svd.s, svd.vt, &svd.ranks, (int32_t)svd.ranks.size(), want_residual);
}
// The block-sparse operator such a batch describes, applied in one launch (rc_block_operator_apply_*): MatMat / ConjMatMat
// (src/types.rs:40-101) for a BLR / hierarchical matrix whose blocks the batched calls compressed.  Entry e places block block_ids[e]
// (ids below count: the low-rank blocks left_i [mid_i] [diag(s_i)] right_i of the stacked factors, as in lowrank_apply_batched; ids from
// count on: block id - count of the stacked dense m x n blocks) with its top-left corner at (rows[e], cols[e]) of the nrows x ncols
// matrix.  The operands are borrowed and must outlive the operator; the two block-CSR patterns (by row for A x, by column for A^H x on
// the swapped, transposed views with the conj flag) are built on the host and owned.  Distinct values of rows must tile [0, nrows) in
// steps of m and distinct values of cols [0, ncols) in steps of n, so that every product writes every row of its result; within a group
// the entries are summed in the order given.  mid and s together are rejected: (L M diag(s) R)^T is not the kernel's chain.
// BlockOperator<T, S> with S = Mixed<T>::storage (MixedBlockOperator<T>) keeps left, mid and right in storage precision
// (rc_block_operator_apply_mixed_*): dense, s, x and y stay in T, and the products have the bits of BlockOperator<T> on promoted factors.
template <typename T, typename S = T> struct BlockOperatorApi;
template <> struct BlockOperatorApi<double, float> { static constexpr auto apply = rc_block_operator_apply_mixed_f64; static constexpr bool conj = false; };
template <> struct BlockOperatorApi<c64, c32> { static constexpr auto apply = rc_block_operator_apply_mixed_c64; static constexpr bool conj = true; };
template <> struct BlockOperatorApi<double> { static constexpr auto apply = rc_block_operator_apply_f64; static constexpr bool conj = false; };
template <> struct BlockOperatorApi<float> { static constexpr auto apply = rc_block_operator_apply_f32; static constexpr bool conj = false; };
template <> struct BlockOperatorApi<c64> { static constexpr auto apply = rc_block_operator_apply_c64; static constexpr bool conj = true; };
template <> struct BlockOperatorApi<c32> { static constexpr auto apply = rc_block_operator_apply_c32; static constexpr bool conj = true; };
template <typename T, typename S = T>
class BlockOperator {
  public:
    using Real = typename Scalar<T>::real;
    BlockOperator(const Context &ctx, int64_t nrows, int64_t ncols, const std::vector<int64_t> &rows, const std::vector<int64_t> &cols,
                  const std::vector<int64_t> &block_ids, int32_t count, const DeviceMatrix<S> *left, const DeviceMatrix<S> *mid,
                  const DeviceBuffer<Real> *s, const DeviceMatrix<S> *right, const DeviceIndex *ranks, int32_t dense_count = 0,
                  const DeviceMatrix<T> *dense = nullptr)
        : nrows_(nrows), ncols_(ncols), count_(count), dense_count_(dense ? dense_count : 0), left_(left), mid_(mid), right_(right), dense_(dense),
          s_(s), ranks_(ranks) {
        if (mid && s) throw AssertionFailed("BlockOperator: mid and s together do not transpose into the kernel's chain");
        if (!(count > 0 && left && right) && !(dense && dense_count > 0)) throw AssertionFailed("BlockOperator: needs a low-rank or a dense batch");
        if (rows.size() != cols.size() || rows.size() != block_ids.size()) throw AssertionFailed("BlockOperator: one row, column and id per entry");
        if (count > 0 && left && right) { m_ = left->nrows() / count; k_ = left->ncols(); n_ = right->ncols(); }
        else { m_ = dense->nrows() / dense_count; n_ = dense->ncols(); }
        p_ = s && count > 0 ? (int64_t)(s->size() / (std::size_t)count) : 0;
        by_row_ = Pattern(ctx, rows, cols, block_ids, m_, nrows);
        by_col_ = Pattern(ctx, cols, rows, block_ids, n_, ncols);
    }
    int64_t nrows() const { return nrows_; }
    int64_t ncols() const { return ncols_; }
    void matmat(const Context &ctx, rc_matrix x, rc_matrix y) const { call(ctx, by_row_, false, x, y); }
    void conj_matmat(const Context &ctx, rc_matrix x, rc_matrix y) const { call(ctx, by_col_, true, x, y); }
    DeviceMatrix<T> apply(const DeviceMatrix<T> &x) const {
        DeviceMatrix<T> y(x.ctx(), nrows_, x.ncols());
        matmat(x.ctx(), x.view(), y.view());
        return y;
    }
    DeviceMatrix<T> conj_apply(const DeviceMatrix<T> &x) const {
        DeviceMatrix<T> y(x.ctx(), ncols_, x.ncols());
        conj_matmat(x.ctx(), x.view(), y.view());
        return y;
    }

  private:
    struct Pattern {  // block-CSR on the device: group_ptr, group_row, entry_block, entry_col
        DeviceIndex ptr, row, block, col;
        int32_t groups = 0;
        Pattern() = default;
        Pattern(const Context &ctx, const std::vector<int64_t> &first, const std::vector<int64_t> &other, const std::vector<int64_t> &ids, int64_t extent,
                int64_t total) {
            std::vector<int64_t> heads(first);
            std::sort(heads.begin(), heads.end());
            heads.erase(std::unique(heads.begin(), heads.end()), heads.end());
            bool tiles = !heads.empty() && heads.front() == 0 && heads.back() + extent == total;
            for (std::size_t g = 1; g < heads.size(); ++g) tiles = tiles && heads[g] - heads[g - 1] == extent;
            if (!tiles) throw AssertionFailed("BlockOperator: the blocks' first rows (columns) must tile the matrix in steps of the block shape");
            std::vector<int64_t> hptr(heads.size() + 1, 0), hblock(ids.size()), hcol(ids.size());
            for (int64_t f : first) ++hptr[(std::size_t)(std::lower_bound(heads.begin(), heads.end(), f) - heads.begin()) + 1];
            for (std::size_t g = 0; g < heads.size(); ++g) hptr[g + 1] += hptr[g];
            std::vector<int64_t> next(hptr.begin(), hptr.end() - 1);
            for (std::size_t e = 0; e < first.size(); ++e) {  // input order inside a group
                const std::size_t at = (std::size_t)next[(std::size_t)(std::lower_bound(heads.begin(), heads.end(), first[e]) - heads.begin())]++;
                hblock[at] = ids[e];
                hcol[at] = other[e];
            }
            groups = (int32_t)heads.size();
            ptr = DeviceIndex(ctx, hptr.size()); ptr.from_host(hptr.data());
            row = DeviceIndex(ctx, heads.size()); row.from_host(heads.data());
            block = DeviceIndex(ctx, hblock.size() + 1); block.from_host(pad(hblock).data());
            col = DeviceIndex(ctx, hcol.size() + 1); col.from_host(pad(hcol).data());
        }
        static std::vector<int64_t> pad(std::vector<int64_t> v) { v.push_back(0); return v; }  // never a null pointer, also without entries
    };
    template <typename E>
    static rc_matrix block_view(const DeviceMatrix<E> *a, int64_t r, int64_t c, bool transposed) {
        if (!a) return rc_matrix{nullptr, 0, 0, 0, 0};
        return transposed ? rc_matrix{a->view().data, c, r, 1, c} : rc_matrix{a->view().data, r, c, c, 1};
    }
    void call(const Context &ctx, const Pattern &pat, bool adjoint, rc_matrix x, rc_matrix y) const {
        const DeviceMatrix<S> *l = adjoint ? right_ : left_, *r = adjoint ? left_ : right_;
        const int64_t lr = adjoint ? k_ : m_, lc = adjoint ? n_ : k_, rr = adjoint ? m_ : k_, rcols = adjoint ? k_ : n_;  // stored shapes
        ctx.check(BlockOperatorApi<T, S>::apply(ctx.raw(), block_view(l, lr, lc, adjoint), lr * lc, block_view(mid_, k_, k_, adjoint), k_ * k_,
                                             s_ ? s_->data() : nullptr, p_, block_view(r, rr, rcols, adjoint), rr * rcols,
                                             ranks_ ? ranks_->data() : nullptr, left_ ? count_ : 0, block_view(dense_, m_, n_, adjoint), m_ * n_,
                                             dense_count_, pat.ptr.data(), pat.row.data(), pat.groups, pat.block.data(), pat.col.data(), x, y, 0,
                                             adjoint && BlockOperatorApi<T, S>::conj ? 1 : 0));
    }
    int64_t nrows_, ncols_, m_ = 0, n_ = 0, k_ = 0, p_ = 0;
    int32_t count_, dense_count_;
    const DeviceMatrix<S> *left_, *mid_, *right_;
    const DeviceMatrix<T> *dense_;
    const DeviceBuffer<Real> *s_;
    const DeviceIndex *ranks_;
    Pattern by_row_, by_col_;
};
template <typename T>
using MixedBlockOperator = BlockOperator<T, typename Mixed<T>::storage>;
template <typename T>
typename Scalar<T>::real max_col_norm(const DeviceMatrix<T> &y) {  // :184-191
    typename Scalar<T>::real out = 0;
    y.ctx().check(Api<T>::max_col_norm(y.ctx().raw(), y.view(), &out));
    return out;
}
template <typename T>
struct AdaptiveResult {
    DeviceMatrix<T> q;
    std::vector<std::pair<std::size_t, double>> residuals;  // Vec<(usize, f64)>
};
template <typename T>
AdaptiveResult<T> sample_range_adaptive(const DeviceMatrix<T> &op, double rel_tol, int64_t sample_size, uint64_t seed, int64_t max_rank = -1) {  // :223-274
    const int64_t m = op.nrows(), n = op.ncols();
    if (max_rank < 0) max_rank = (((m < n ? m : n) + sample_size - 1) / sample_size) * sample_size;
    DeviceMatrix<T> qcap(op.ctx(), m, max_rank);
    const int64_t hist_cap = max_rank / (sample_size < 1 ? 1 : sample_size) + 2;
    std::vector<int64_t> hrank((std::size_t)hist_cap);
    std::vector<double> hres((std::size_t)hist_cap);
    int64_t rank = 0, hlen = 0;
    op.ctx().check(Api<T>::sample_range_adaptive(op.ctx().raw(), op.view(), rel_tol, sample_size, rc_matrix{nullptr, 0, 0, 0, 0}, seed, qcap.view(),
                                                 &rank, hrank.data(), hres.data(), hist_cap, &hlen));
    AdaptiveResult<T> out{qcap.leading(m, rank), {}};
    for (int64_t i = 0; i < hlen; ++i) out.residuals.emplace_back((std::size_t)hrank[(std::size_t)i], hres[(std::size_t)i]);
    return out;
}

// ---- operators: MatVec / ConjMatVec / MatMat / ConjMatMat (src/types.rs:40-101) -------------------------------------------
// The reference implements its range finders for ANY operator (`impl<Op: MatMat<A = $scalar>> SampleRange for Op`,
// src/random_sampling.rs:102, :130, :222; compute_from_range_estimate<Op: ConjMatMat>, src/qr.rs:311-323, src/svd.rs:171-183).
// Here an operator is any class with
//     int64_t nrows() const;  int64_t ncols() const;                                   MatVec::nrows / ncols
//     void matmat(const Context &ctx, rc_matrix x, rc_matrix y) const;                 y (nrows x s) = A x     (MatMat)
//     void conj_matmat(const Context &ctx, rc_matrix x, rc_matrix y) const;  [optional] y (ncols x s) = A^H x  (ConjMatMat)
// x, y are strided DEVICE views; the products are enqueued on ctx (through this library or with the host's own kernels on
// rc_get_stream).  The overloads below hand the library an rc_operator whose callbacks forward to those members; everything
// else (Omega, pivoted QR, SVD, the adaptive loop) runs inside the library exactly as for a dense matrix.
template <typename T> struct ApiOp;
#define RC_API_OP(T, SUF)                                                                          \
    template <> struct ApiOp<T> {                                                                  \
        static constexpr auto sample_range_by_rank = rc_sample_range_by_rank_op_##SUF;             \
        static constexpr auto sample_range_power_iteration = rc_sample_range_power_iteration_op_##SUF; \
        static constexpr auto sample_range_adaptive = rc_sample_range_adaptive_op_##SUF;           \
        static constexpr auto qr_from_range_estimate = rc_qr_from_range_estimate_op_##SUF;         \
        static constexpr auto svd_from_range_estimate = rc_svd_from_range_estimate_op_##SUF;       \
    };
RC_API_OP(double, f64)
RC_API_OP(float, f32)
RC_API_OP(c64, c64)
RC_API_OP(c32, c32)
#undef RC_API_OP

namespace detail {
template <class Op, class = void> struct has_conj_matmat : std::false_type {};
template <class Op>
struct has_conj_matmat<Op, std::void_t<decltype(std::declval<const Op &>().conj_matmat(std::declval<const Context &>(), rc_matrix{}, rc_matrix{}))>> : std::true_type {};

inline int32_t status_of_current_exception() {  // a callback must not unwind into C: exceptions become the status the entry point returns
    try { throw; }
    catch (const CompressionError &) { return RC_COMPRESSION_ERROR; }
    catch (const LayoutError &) { return RC_LAYOUT_ERROR; }
    catch (const PivotedQRError &) { return RC_PIVOTED_QR_ERROR; }
    catch (const LinalgError &) { return RC_LINALG_ERROR; }
    catch (const AssertionFailed &) { return RC_INVALID_ARGUMENT; }
    catch (...) { return RC_RUNTIME_ERROR; }
}
}  // namespace detail

// rc_operator of a C++ operator object (borrowed: `op` and `ctx` must outlive the call it is passed to)
template <class Op>
class OperatorTable {
  public:
    OperatorTable(const Context &ctx, const Op &op) : ctx_(&ctx), op_(&op) {
        table_.rows = op.nrows();
        table_.cols = op.ncols();
        table_.matmat = &OperatorTable::matmat_cb;
        table_.conj_matmat = detail::has_conj_matmat<Op>::value ? &OperatorTable::conj_matmat_cb : nullptr;
        table_.user = this;
    }
    const rc_operator *get() const { return &table_; }

  private:
    static int32_t matmat_cb(void *user, rc_context *, rc_matrix x, rc_matrix y) {
        auto *self = static_cast<OperatorTable *>(user);
        try { self->op_->matmat(*self->ctx_, x, y); return RC_OK; } catch (...) { return detail::status_of_current_exception(); }
    }
    static int32_t conj_matmat_cb(void *user, rc_context *, rc_matrix x, rc_matrix y) {
        auto *self = static_cast<OperatorTable *>(user);
        try {
            if constexpr (detail::has_conj_matmat<Op>::value) self->op_->conj_matmat(*self->ctx_, x, y);
            return RC_OK;
        } catch (...) { return detail::status_of_current_exception(); }
    }
    const Context *ctx_;
    const Op *op_;
    rc_operator table_{};
};

// a dense device matrix behind the operator interface (each product is the library's own GEMM on the views it is handed)
template <typename T>
struct DenseOperator {
    const DeviceMatrix<T> *a;
    int64_t nrows() const { return a->nrows(); }
    int64_t ncols() const { return a->ncols(); }
    void matmat(const Context &ctx, rc_matrix x, rc_matrix y) const { ctx.check(Api<T>::matmat(ctx.raw(), a->view(), x, y)); }
    void conj_matmat(const Context &ctx, rc_matrix x, rc_matrix y) const { ctx.check(Api<T>::conj_matmat(ctx.raw(), a->view(), x, y)); }
};
// A = U V^H given by its factors (U: m x r, V: n x r) and never formed: two skinny GEMMs per product
template <typename T>
struct LowRankOperator {
    const DeviceMatrix<T> *u, *v;
    int64_t nrows() const { return u->nrows(); }
    int64_t ncols() const { return v->nrows(); }
    void matmat(const Context &ctx, rc_matrix x, rc_matrix y) const {
        DeviceMatrix<T> t(ctx, v->ncols(), x.cols);
        ctx.check(Api<T>::gemm(ctx.raw(), 2, 0, Scalar<T>::wire((T)1), v->view(), x, Scalar<T>::wire((T)0), t.view()));
        ctx.check(Api<T>::gemm(ctx.raw(), 0, 0, Scalar<T>::wire((T)1), u->view(), t.view(), Scalar<T>::wire((T)0), y));
        ctx.synchronize();  // t is freed on return
    }
    void conj_matmat(const Context &ctx, rc_matrix x, rc_matrix y) const {
        DeviceMatrix<T> t(ctx, u->ncols(), x.cols);
        ctx.check(Api<T>::gemm(ctx.raw(), 2, 0, Scalar<T>::wire((T)1), u->view(), x, Scalar<T>::wire((T)0), t.view()));
        ctx.check(Api<T>::gemm(ctx.raw(), 0, 0, Scalar<T>::wire((T)1), v->view(), t.view(), Scalar<T>::wire((T)0), y));
        ctx.synchronize();
    }
};

// impl<Op: MatMat> SampleRange for Op (src/random_sampling.rs:102-121)
template <typename T, class Op>
DeviceMatrix<T> sample_range_by_rank(const Context &ctx, const Op &op, int64_t k, int64_t p, uint64_t seed) {
    int64_t kk = k < op.nrows() ? k : op.nrows();
    if (k + p < kk) kk = k + p;
    DeviceMatrix<T> q(ctx, op.nrows(), kk);
    OperatorTable<Op> tab(ctx, op);
    ctx.check(ApiOp<T>::sample_range_by_rank(ctx.raw(), tab.get(), k, p, rc_matrix{nullptr, 0, 0, 0, 0}, seed, q.view()));
    return q;
}
// impl<Op: MatMat + ConjMatMat> SampleRangePowerIteration for Op (src/random_sampling.rs:130-163)
template <typename T, class Op>
DeviceMatrix<T> sample_range_power_iteration(const Context &ctx, const Op &op, int64_t k, int64_t p, int64_t it_count, uint64_t seed) {
    int64_t kk = k < op.nrows() ? k : op.nrows();
    if (k + p < kk) kk = k + p;
    if (op.ncols() < kk) kk = op.ncols();
    DeviceMatrix<T> q(ctx, op.nrows(), kk);
    OperatorTable<Op> tab(ctx, op);
    ctx.check(ApiOp<T>::sample_range_power_iteration(ctx.raw(), tab.get(), k, p, it_count, rc_matrix{nullptr, 0, 0, 0, 0}, seed, q.view()));
    return q;
}
// impl<Op: MatMat + ConjMatMat> AdaptiveSampling for Op (src/random_sampling.rs:222-277)
template <typename T, class Op>
AdaptiveResult<T> sample_range_adaptive(const Context &ctx, const Op &op, double rel_tol, int64_t sample_size, uint64_t seed, int64_t max_rank = -1) {
    const int64_t m = op.nrows(), n = op.ncols();
    if (max_rank < 0) max_rank = (((m < n ? m : n) + sample_size - 1) / sample_size) * sample_size;
    DeviceMatrix<T> qcap(ctx, m, max_rank);
    const int64_t hist_cap = max_rank / (sample_size < 1 ? 1 : sample_size) + 2;
    std::vector<int64_t> hrank((std::size_t)hist_cap);
    std::vector<double> hres((std::size_t)hist_cap);
    int64_t rank = 0, hlen = 0;
    OperatorTable<Op> tab(ctx, op);
    ctx.check(ApiOp<T>::sample_range_adaptive(ctx.raw(), tab.get(), rel_tol, sample_size, rc_matrix{nullptr, 0, 0, 0, 0}, seed, qcap.view(), &rank, hrank.data(),
                                              hres.data(), hist_cap, &hlen));
    AdaptiveResult<T> out{qcap.leading(m, rank), {}};
    for (int64_t i = 0; i < hlen; ++i) out.residuals.emplace_back((std::size_t)hrank[(std::size_t)i], hres[(std::size_t)i]);
    return out;
}
// QRTraits / SVDTraits::compute_from_range_estimate<Op: ConjMatMat> (src/qr.rs:311-323, src/svd.rs:171-183)
template <typename T, class Op>
QR<T> qr_from_range_estimate(const Context &ctx, const DeviceMatrix<T> &range, const Op &op) {
    const int64_t m = op.nrows(), n = op.ncols(), k = range.ncols() < n ? range.ncols() : n;
    QR<T> out{DeviceMatrix<T>(ctx, m, k), DeviceMatrix<T>(ctx, k, n), DeviceIndex(ctx, (std::size_t)n)};
    OperatorTable<Op> tab(ctx, op);
    ctx.check(ApiOp<T>::qr_from_range_estimate(ctx.raw(), range.view(), tab.get(), out.q.view(), out.r.view(), out.ind.data()));
    return out;
}
template <typename T, class Op>
SVD<T> svd_from_range_estimate(const Context &ctx, const DeviceMatrix<T> &range, const Op &op) {
    using Real = typename Scalar<T>::real;
    const int64_t m = op.nrows(), n = op.ncols(), r = range.ncols() < n ? range.ncols() : n;
    SVD<T> out{DeviceMatrix<T>(ctx, m, r), DeviceBuffer<Real>(ctx, (std::size_t)r), DeviceMatrix<T>(ctx, r, n)};
    OperatorTable<Op> tab(ctx, op);
    ctx.check(ApiOp<T>::svd_from_range_estimate(ctx.raw(), range.view(), tab.get(), out.u.view(), out.s.data(), out.vt.view()));
    return out;
}

// ---- one matrix sharded by rows over several ranks (rc_rsvd_id_row_sharded_*; the reference is single-process) ----------
// A communicator over RCCL (one process per GPU) or over the host's own communication layer (callbacks on host pointers).
class Comm {
  public:
    static Comm rccl(int32_t world, int32_t rank, const void *id128, int32_t device) {
        Comm c;
        if (rc_comm_init(&c.raw_, world, rank, id128, device) != RC_OK) throw HipRuntimeError(rc_comm_last_error_message(nullptr));
        return c;
    }
    static Comm host(int32_t world, int32_t rank, int32_t device, rc_host_all_gather_fn all_gather, rc_host_all_reduce_sum_fn all_reduce_sum, void *user) {
        Comm c;
        if (rc_comm_init_host(&c.raw_, world, rank, device, all_gather, all_reduce_sum, user) != RC_OK) throw AssertionFailed("rc_comm_init_host: bad arguments");
        return c;
    }
    Comm(Comm &&o) noexcept : raw_(o.raw_) { o.raw_ = nullptr; }
    Comm &operator=(Comm &&o) noexcept { if (this != &o) { rc_comm_destroy(raw_); raw_ = o.raw_; o.raw_ = nullptr; } return *this; }
    Comm(const Comm &) = delete;
    Comm &operator=(const Comm &) = delete;
    ~Comm() { rc_comm_destroy(raw_); }
    rc_comm *raw() const { return raw_; }

  private:
    Comm() = default;
    rc_comm *raw_ = nullptr;
};
// this rank's rows of the global factors (range_q, u, qr_q, c) and the replicated ones (s, vt, r, ind, z)
template <typename T>
struct ShardedRsvdId {
    DeviceMatrix<T> range_q, u;
    DeviceBuffer<T> s;
    DeviceMatrix<T> vt, qr_q, r;
    DeviceIndex ind;
    DeviceMatrix<T> c, z;
};
inline rc_status rsvd_id_row_sharded_raw(rc_comm *cm, rc_context *cx, rc_matrix a, int64_t k, int64_t p, uint64_t seed, const rc_rsvd_id_out *o, double) {
    return rc_rsvd_id_row_sharded_f64(cm, cx, a, k, p, seed, o);
}
inline rc_status rsvd_id_row_sharded_raw(rc_comm *cm, rc_context *cx, rc_matrix a, int64_t k, int64_t p, uint64_t seed, const rc_rsvd_id_out *o, float) {
    return rc_rsvd_id_row_sharded_f32(cm, cx, a, k, p, seed, o);
}
// a_local: the m_r x n row block of this rank (m_r >= k + p); comm == nullptr: one rank.  Real scalar types.
template <typename T>
ShardedRsvdId<T> rsvd_id_row_sharded(const Comm *comm, const DeviceMatrix<T> &a_local, int64_t k, int64_t p, uint64_t seed) {
    const Context &cx = a_local.ctx();
    const int64_t mr = a_local.nrows(), n = a_local.ncols();
    ShardedRsvdId<T> out{DeviceMatrix<T>(cx, mr, k), DeviceMatrix<T>(cx, mr, k), DeviceBuffer<T>(cx, (std::size_t)k), DeviceMatrix<T>(cx, k, n), DeviceMatrix<T>(cx, mr, k),
                         DeviceMatrix<T>(cx, k, n), DeviceIndex(cx, (std::size_t)n), DeviceMatrix<T>(cx, mr, k), DeviceMatrix<T>(cx, k, n)};
    rc_rsvd_id_out o{out.range_q.view(), out.u.view(), out.s.data(), out.vt.view(), out.qr_q.view(), out.r.view(), out.ind.data(), out.c.view(), out.z.view()};
    cx.check(rsvd_id_row_sharded_raw(comm ? comm->raw() : nullptr, cx.raw(), a_local.view(), k, p, seed, &o, T()));
    return out;
}

}  // namespace rusty_compression
