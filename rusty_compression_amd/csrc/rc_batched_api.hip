// The host layer of the batched family: the argument checks and every rc_*_batched_* / rc_block_operator_apply_* entry point of the C ABI, defined
// once for f64, f32, c64 and c32.  No kernel is defined or instantiated here: the launchers live in the kernels_*.hip files, each declared
// once over the element type of its typed views (rc_batched.hpp), and an entry point is "check, return when there is nothing to do, launch on
// from_c<E> views" under the call guard (rc_common.hpp).
#include "rc_common.hpp"

#include <algorithm>
#include <cmath>
#include <type_traits>

using namespace rc;

namespace {

// the domain of the batched small-matrix kernels (kernels_batched_id.hip); returns k clamped to min(m, n)
int64_t batched_domain(const char *who, const char *larger, const rc_matrix &a, int32_t count, int64_t k, double tol) {
    const int64_t m = a.rows, n = a.cols;
    RC_REQUIRE(count >= 0, RC_INVALID_ARGUMENT, "%s: count = %d < 0", who, (int)count);
    RC_REQUIRE(m >= 1 && m <= 512 && n >= 1 && n <= 512 && k >= 1 && k <= 128, RC_INVALID_ARGUMENT,
               "%s: needs 1 <= m, n <= 512 and 1 <= k <= 128 (got %lld x %lld, k = %lld); use %s for larger matrices", who, (long long)m, (long long)n,
               (long long)k, larger);
    RC_REQUIRE(tol < 1.0 && 0.0 <= tol, RC_INVALID_ARGUMENT, "Require 0 <= tol < 1.0");
    return std::min(k, std::min(m, n));
}
// one output view spans (rows - 1) |rs| + (cols - 1) |cs| + 1 elements; a smaller batch stride would overlap two matrices
void check_batch_stride(const char *who, const char *name, int64_t bs, const rc_matrix &v, int32_t count) {
    const int64_t span = (v.rows - 1) * std::abs(v.row_stride) + (v.cols - 1) * std::abs(v.col_stride) + 1;
    RC_REQUIRE(count <= 1 || bs >= span, RC_INVALID_ARGUMENT, "%s: %s_batch_stride %lld < %lld overlaps the outputs of two matrices", who, name,
               (long long)bs, (long long)span);
}

}  // namespace

namespace rc {
int64_t check_column_id_rank_batched(const rc_matrix &a, int32_t count, int64_t k, double tol, const rc_matrix &cm, int64_t cbs, const rc_matrix &z,
                                     int64_t zbs, const int64_t *col_ind, const int64_t *ranks) {
    const int64_t m = a.rows, n = a.cols;
    k = batched_domain("column_id_rank_batched", "rc_column_id_rank_* / rc_batch_column_id_*", a, count, k, tol);
    RC_REQUIRE(cm.rows == m && cm.cols == k && z.rows == k && z.cols == n, RC_INVALID_ARGUMENT,
               "column_id_rank_batched: c must be %lld x %lld and z %lld x %lld (k clamped to min(m, n))", (long long)m, (long long)k, (long long)k, (long long)n);
    check_batch_stride("column_id_rank_batched", "c", cbs, cm, count);
    check_batch_stride("column_id_rank_batched", "z", zbs, z, count);
    if (count > 0) RC_REQUIRE(a.data && cm.data && z.data && col_ind && ranks, RC_INVALID_ARGUMENT, "column_id_rank_batched: null pointer");
    return k;
}
int64_t check_two_sided_id_rank_batched(const rc_matrix &a, int32_t count, int64_t k, double tol, const rc_matrix &cm, int64_t cbs, const rc_matrix &x,
                                        int64_t xbs, const rc_matrix &r, int64_t rbs, const int64_t *row_ind, const int64_t *col_ind, const int64_t *ranks) {
    const int64_t m = a.rows, n = a.cols;
    const char *who = "two_sided_id_rank_batched";
    k = batched_domain(who, "rc_column_id_rank_* + rc_column_id_two_sided_*", a, count, k, tol);
    RC_REQUIRE(cm.rows == m && cm.cols == k && x.rows == k && x.cols == k && r.rows == k && r.cols == n, RC_INVALID_ARGUMENT,
               "two_sided_id_rank_batched: c must be %lld x %lld, x %lld x %lld and r %lld x %lld (k clamped to min(m, n))", (long long)m, (long long)k,
               (long long)k, (long long)k, (long long)k, (long long)n);
    check_batch_stride(who, "c", cbs, cm, count);
    check_batch_stride(who, "x", xbs, x, count);
    check_batch_stride(who, "r", rbs, r, count);
    if (count > 0) RC_REQUIRE(a.data && cm.data && x.data && r.data && row_ind && col_ind && ranks, RC_INVALID_ARGUMENT, "two_sided_id_rank_batched: null pointer");
    return k;
}
// the batched SVD's checks: the batched IDs' domain plus min(m, n) <= 128 (the core of one workgroup)
int64_t check_svd_rank_batched(const rc_matrix &a, int32_t count, int64_t k, double tol, const rc_matrix &u, int64_t ubs, const void *s, const rc_matrix &vt,
                               int64_t vbs, const int64_t *ranks) {
    const int64_t m = a.rows, n = a.cols;
    const char *who = "svd_rank_batched";
    k = batched_domain(who, "rc_compute_svd_*", a, count, k, tol);
    RC_REQUIRE(std::min(m, n) <= 128, RC_INVALID_ARGUMENT, "%s: needs min(m, n) <= 128 (got %lld x %lld); use rc_compute_svd_* for larger matrices", who,
               (long long)m, (long long)n);
    RC_REQUIRE(u.rows == m && u.cols == k && vt.rows == k && vt.cols == n, RC_INVALID_ARGUMENT,
               "svd_rank_batched: u must be %lld x %lld and vt %lld x %lld (k clamped to min(m, n))", (long long)m, (long long)k, (long long)k, (long long)n);
    check_batch_stride(who, "u", ubs, u, count);
    check_batch_stride(who, "vt", vbs, vt, count);
    if (count > 0) RC_REQUIRE(a.data && u.data && s && vt.data && ranks, RC_INVALID_ARGUMENT, "svd_rank_batched: null pointer");
    return k;
}

// rc_lowrank_apply_batched_*: the shapes of the factor chain left (m x k) [mid (k x k)] right (k x n) [b (n x nrhs)] -> y, the batched kernels' domain
// for m, n, k, and y's batch stride; mid and b take part only when their data pointer is set
void check_lowrank_apply_batched(const rc_matrix &left, const rc_matrix &mid, const rc_matrix &right, int32_t count, const rc_matrix &b, const rc_matrix &y,
                                 int64_t ybs) {
    const char *who = "lowrank_apply_batched";
    const int64_t m = left.rows, k = left.cols, n = right.cols;
    RC_REQUIRE(count >= 0, RC_INVALID_ARGUMENT, "%s: count = %d < 0", who, (int)count);
    RC_REQUIRE(m >= 1 && m <= 512 && n >= 1 && n <= 512 && k >= 1 && k <= 128, RC_INVALID_ARGUMENT,
               "%s: needs 1 <= m, n <= 512 and 1 <= k <= 128 (got left %lld x %lld, right %lld x %lld)", who, (long long)m, (long long)k,
               (long long)right.rows, (long long)n);
    RC_REQUIRE(right.rows == k, RC_INVALID_ARGUMENT, "%s: left is %lld x %lld but right has %lld rows", who, (long long)m, (long long)k, (long long)right.rows);
    RC_REQUIRE(!mid.data || (mid.rows == k && mid.cols == k), RC_INVALID_ARGUMENT, "%s: mid must be %lld x %lld (got %lld x %lld)", who, (long long)k,
               (long long)k, (long long)mid.rows, (long long)mid.cols);
    RC_REQUIRE(!b.data || (b.rows == n && b.cols >= 1 && b.cols <= INT32_MAX), RC_INVALID_ARGUMENT, "%s: b must be %lld x nrhs with nrhs >= 1 (got %lld x %lld)",
               who, (long long)n, (long long)b.rows, (long long)b.cols);
    const int64_t ncols = b.data ? b.cols : n;
    RC_REQUIRE(y.rows == m && y.cols == ncols, RC_INVALID_ARGUMENT, "%s: y must be %lld x %lld (got %lld x %lld)", who, (long long)m, (long long)ncols,
               (long long)y.rows, (long long)y.cols);
    check_batch_stride(who, "y", ybs, y, count);
    if (count > 0) RC_REQUIRE(left.data && right.data && y.data, RC_INVALID_ARGUMENT, "%s: null pointer", who);
}

// rc_lowrank_residual_batched_*: the shapes of a (m x n) against the factor chain left (m x K) [mid (K x K)] right (K x n), the sketched ID's domain
// for m, n, K, and e's shape and batch stride when it is asked for; mid and e take part only when their data pointer is set
void check_lowrank_residual_batched(const rc_matrix &a, const rc_matrix &left, const rc_matrix &mid, const rc_matrix &right, int32_t count, const rc_matrix &e,
                                    int64_t ebs, const void *err) {
    const char *who = "lowrank_residual_batched";
    const int64_t m = a.rows, n = a.cols, K = left.cols;
    RC_REQUIRE(count >= 0, RC_INVALID_ARGUMENT, "%s: count = %d < 0", who, (int)count);
    RC_REQUIRE(m >= 1 && m <= 65536 && n >= 1 && n <= 512 && K >= 1 && K <= 128, RC_INVALID_ARGUMENT,
               "%s: needs 1 <= m <= 65536, 1 <= n <= 512 and 1 <= K <= 128 (got a %lld x %lld, left %lld x %lld)", who, (long long)m, (long long)n,
               (long long)left.rows, (long long)K);
    RC_REQUIRE(left.rows == m && right.rows == K && right.cols == n, RC_INVALID_ARGUMENT,
               "%s: a is %lld x %lld but left is %lld x %lld and right %lld x %lld", who, (long long)m, (long long)n, (long long)left.rows, (long long)K,
               (long long)right.rows, (long long)right.cols);
    RC_REQUIRE(!mid.data || (mid.rows == K && mid.cols == K), RC_INVALID_ARGUMENT, "%s: mid must be %lld x %lld (got %lld x %lld)", who, (long long)K,
               (long long)K, (long long)mid.rows, (long long)mid.cols);
    if (e.data) {
        RC_REQUIRE(e.rows == m && e.cols == n, RC_INVALID_ARGUMENT, "%s: e must be %lld x %lld (got %lld x %lld)", who, (long long)m, (long long)n,
                   (long long)e.rows, (long long)e.cols);
        check_batch_stride(who, "e", ebs, e, count);
    }
    if (count > 0) RC_REQUIRE(a.data && left.data && right.data && err, RC_INVALID_ARGUMENT, "%s: null pointer", who);
}

// rc_block_operator_apply_*: the block shape m x n (and the inner width K of the low-rank batch, 0 without one) from left / right when there is a
// low-rank batch, else from dense; the batched kernels' domain for m, n, K; x and y as N x nrhs and M x nrhs.  Indices live on the device and are
// checked there.
BlockShape check_block_operator_apply(const rc_matrix &left, const rc_matrix &mid, const rc_matrix &right, int32_t count, const rc_matrix &dense,
                                      int32_t *dense_count, const BlockPattern &pat, const rc_matrix &x, const rc_matrix &y) {
    const char *who = "block_operator_apply";
    if (!dense.data) *dense_count = 0;
    RC_REQUIRE(count >= 0 && *dense_count >= 0 && pat.groups >= 0, RC_INVALID_ARGUMENT, "%s: count = %d, dense_count = %d, groups = %d: none may be negative", who,
               (int)count, (int)*dense_count, (int)pat.groups);
    const bool lowrank = count > 0 || left.data;
    BlockShape sh{0, 0, 0};
    if (lowrank) {
        const int64_t m = left.rows, k = left.cols, n = right.cols;
        RC_REQUIRE(m >= 1 && m <= 512 && n >= 1 && n <= 512 && k >= 1 && k <= 128, RC_INVALID_ARGUMENT,
                   "%s: needs 1 <= m, n <= 512 and 1 <= K <= 128 (got left %lld x %lld, right %lld x %lld)", who, (long long)m, (long long)k,
                   (long long)right.rows, (long long)n);
        RC_REQUIRE(right.rows == k, RC_INVALID_ARGUMENT, "%s: left is %lld x %lld but right has %lld rows", who, (long long)m, (long long)k,
                   (long long)right.rows);
        RC_REQUIRE(!mid.data || (mid.rows == k && mid.cols == k), RC_INVALID_ARGUMENT, "%s: mid must be %lld x %lld (got %lld x %lld)", who, (long long)k,
                   (long long)k, (long long)mid.rows, (long long)mid.cols);
        RC_REQUIRE(!dense.data || (dense.rows == m && dense.cols == n), RC_INVALID_ARGUMENT, "%s: dense must be %lld x %lld like the low-rank blocks (got %lld x %lld)",
                   who, (long long)m, (long long)n, (long long)dense.rows, (long long)dense.cols);
        if (count > 0) RC_REQUIRE(left.data && right.data, RC_INVALID_ARGUMENT, "%s: null pointer (left or right with count > 0)", who);
        sh = BlockShape{(int)m, (int)n, (int)k};
    } else if (dense.data) {
        RC_REQUIRE(dense.rows >= 1 && dense.rows <= 512 && dense.cols >= 1 && dense.cols <= 512, RC_INVALID_ARGUMENT,
                   "%s: needs 1 <= m, n <= 512 (got dense %lld x %lld)", who, (long long)dense.rows, (long long)dense.cols);
        sh = BlockShape{(int)dense.rows, (int)dense.cols, 0};
    } else {
        RC_REQUIRE(pat.groups == 0, RC_INVALID_ARGUMENT, "%s: neither a low-rank nor a dense batch: the block shape is unknown", who);
    }
    RC_REQUIRE(x.cols >= 1 && x.cols <= INT32_MAX && x.rows >= 0, RC_INVALID_ARGUMENT, "%s: x must be N x nrhs with nrhs >= 1 (got %lld x %lld)", who,
               (long long)x.rows, (long long)x.cols);
    RC_REQUIRE(y.cols == x.cols && y.rows >= 0, RC_INVALID_ARGUMENT, "%s: y must be M x %lld like x (got %lld x %lld)", who, (long long)x.cols,
               (long long)y.rows, (long long)y.cols);
    if (pat.groups > 0)
        RC_REQUIRE(pat.group_ptr && pat.group_row && pat.entry_block && pat.entry_col && x.data && y.data, RC_INVALID_ARGUMENT,
                   "%s: null pointer (an index array, x or y with groups > 0)", who);
    return sh;
}

// rc_lowrank_recompress_batched_* and its complex twin: the shapes of the factor chain left (m x K) [mid (K x K)] right (K x n) against u (m x min(k, K))
// and vt (min(k, K) x n)
void check_lowrank_recompress_batched(const rc_matrix &left, const rc_matrix &mid, const rc_matrix &right, int32_t count, int64_t k, double tol,
                                      const rc_matrix &u, int64_t ubs, const void *s_out, const rc_matrix &vt, int64_t vbs, const int64_t *ranks, int tall) {
    const char *who = tall == RC_LARGE_COMPLEX  ? "lowrank_recompress_complex_large_batched"
                      : tall == RC_LARGE        ? "lowrank_recompress_large_batched"
                      : tall == RC_TALL_COMPLEX ? "lowrank_recompress_tall_complex_batched"
                      : tall                    ? "lowrank_recompress_tall_batched"
                                                : "lowrank_recompress_batched";
    const int64_t m = left.rows, K = left.cols, n = right.cols;
    const bool large = tall == RC_LARGE || tall == RC_LARGE_COMPLEX;
    RC_REQUIRE(count >= 0, RC_INVALID_ARGUMENT, "%s: count = %d < 0", who, (int)count);
    RC_REQUIRE(m >= 1 && m <= (tall ? 65536 : 512) && n >= 1 && n <= (large ? 65536 : 512) && K >= 1 && K <= 128 && k >= 1, RC_INVALID_ARGUMENT,
               "%s: needs 1 <= m%s, inner width 1 <= K <= 128 and k >= 1 (got left %lld x %lld, right %lld x %lld, k = %lld)", who,
               large ? ", n <= 65536" : tall ? " <= 65536, 1 <= n <= 512" : ", n <= 512", (long long)m, (long long)K, (long long)right.rows, (long long)n,
               (long long)k);
    RC_REQUIRE(right.rows == K, RC_INVALID_ARGUMENT, "%s: left is %lld x %lld but right has %lld rows", who, (long long)m, (long long)K, (long long)right.rows);
    RC_REQUIRE(K <= std::min(m, n), RC_INVALID_ARGUMENT,
               "%s: needs K <= min(m, n) (got K = %lld for %lld x %lld blocks); rebuild the blocks with rc_lowrank_apply_batched_* and use rc_svd_rank_batched_*",
               who, (long long)K, (long long)m, (long long)n);
    RC_REQUIRE(tol < 1.0 && 0.0 <= tol, RC_INVALID_ARGUMENT, "Require 0 <= tol < 1.0");
    RC_REQUIRE(!mid.data || (mid.rows == K && mid.cols == K), RC_INVALID_ARGUMENT, "%s: mid must be %lld x %lld (got %lld x %lld)", who, (long long)K,
               (long long)K, (long long)mid.rows, (long long)mid.cols);
    const int64_t kk = std::min(k, K);
    RC_REQUIRE(u.rows == m && u.cols == kk && vt.rows == kk && vt.cols == n, RC_INVALID_ARGUMENT,
               "%s: u must be %lld x %lld and vt %lld x %lld (k clamped to K)", who, (long long)m, (long long)kk, (long long)kk, (long long)n);
    check_batch_stride(who, "u", ubs, u, count);
    check_batch_stride(who, "vt", vbs, vt, count);
    if (count > 0) RC_REQUIRE(left.data && right.data && u.data && s_out && vt.data && ranks, RC_INVALID_ARGUMENT, "%s: null pointer", who);
}

// rc_sketch_column_id_rank_batched_* and rc_sketch_column_id_rank_complex_batched_*.  Returns kk = min(k, l, n).
int64_t check_sketch_column_id_rank_batched(const rc_matrix &a, const rc_matrix &omega, int32_t count, int64_t k, double tol, const rc_matrix &y, int64_t ybs,
                                            const rc_matrix &cm, int64_t cbs, const rc_matrix &z, int64_t zbs, const int64_t *col_ind, const int64_t *ranks) {
    const char *who = "sketch_column_id_rank_batched";
    const int64_t m = a.rows, n = a.cols, l = omega.rows;
    RC_REQUIRE(count >= 0, RC_INVALID_ARGUMENT, "%s: count = %d < 0", who, (int)count);
    RC_REQUIRE(m >= 1 && m <= 65536 && n >= 1 && n <= 512 && l >= 1 && l <= 128 && k >= 1 && k <= 128, RC_INVALID_ARGUMENT,
               "%s: needs 1 <= m <= 65536, 1 <= n <= 512, 1 <= l <= 128 and 1 <= k <= 128 (got a %lld x %lld, omega %lld x %lld, k = %lld)", who, (long long)m,
               (long long)n, (long long)l, (long long)omega.cols, (long long)k);
    RC_REQUIRE(omega.cols == m, RC_INVALID_ARGUMENT, "%s: a has %lld rows but omega has %lld columns", who, (long long)m, (long long)omega.cols);
    RC_REQUIRE(tol < 1.0 && 0.0 <= tol, RC_INVALID_ARGUMENT, "Require 0 <= tol < 1.0");
    const int64_t kk = std::min(k, std::min(l, n));
    RC_REQUIRE(cm.rows == m && cm.cols == kk && z.rows == kk && z.cols == n, RC_INVALID_ARGUMENT,
               "%s: c must be %lld x %lld and z %lld x %lld (k clamped to min(l, n))", who, (long long)m, (long long)kk, (long long)kk, (long long)n);
    RC_REQUIRE(!y.data || (y.rows == l && y.cols == n), RC_INVALID_ARGUMENT, "%s: y must be %lld x %lld (got %lld x %lld)", who, (long long)l, (long long)n,
               (long long)y.rows, (long long)y.cols);
    check_batch_stride(who, "c", cbs, cm, count);
    check_batch_stride(who, "z", zbs, z, count);
    if (y.data) check_batch_stride(who, "y", ybs, y, count);
    if (count > 0) RC_REQUIRE(a.data && omega.data && cm.data && z.data && col_ind && ranks, RC_INVALID_ARGUMENT, "%s: null pointer", who);
    return kk;
}
// rc_sketch_range_step_batched_* and, with complex, rc_sketch_range_step_complex_batched_* under its own name
void check_sketch_range_step_batched(const rc_matrix &a, const rc_matrix &omega, int32_t count, const rc_matrix &y, int64_t ybs, const rc_matrix &q,
                                     int64_t qbs, const rc_matrix &p, int64_t pbs, const int64_t *ranks, bool complex) {
    const char *who = complex ? "sketch_range_step_complex_batched" : "sketch_range_step_batched";
    const int64_t m = a.rows, n = a.cols, l = omega.rows;
    RC_REQUIRE(count >= 0, RC_INVALID_ARGUMENT, "%s: count = %d < 0", who, (int)count);
    RC_REQUIRE(m >= 1 && m <= 65536 && n >= 1 && n <= 512 && l >= 1 && l <= 128 && l <= std::min(m, n), RC_INVALID_ARGUMENT,
               "%s: needs 1 <= m <= 65536, 1 <= n <= 512 and 1 <= l <= min(128, m, n) (got a %lld x %lld, omega %lld x %lld)", who, (long long)m,
               (long long)n, (long long)l, (long long)omega.cols);
    RC_REQUIRE(omega.cols == m, RC_INVALID_ARGUMENT, "%s: a has %lld rows but omega has %lld columns", who, (long long)m, (long long)omega.cols);
    RC_REQUIRE(!y.data || (y.rows == l && y.cols == n), RC_INVALID_ARGUMENT, "%s: y must be %lld x %lld (got %lld x %lld)", who, (long long)l, (long long)n,
               (long long)y.rows, (long long)y.cols);
    RC_REQUIRE(q.rows == l && q.cols == n && p.rows == m && p.cols == l, RC_INVALID_ARGUMENT, "%s: q must be %lld x %lld and p %lld x %lld", who,
               (long long)l, (long long)n, (long long)m, (long long)l);
    check_batch_stride(who, "q", qbs, q, count);
    check_batch_stride(who, "p", pbs, p, count);
    if (y.data) check_batch_stride(who, "y", ybs, y, count);
    if (count > 0) RC_REQUIRE(a.data && omega.data && q.data && p.data && ranks, RC_INVALID_ARGUMENT, "%s: null pointer", who);
}
// rc_sketch_product_batched_*: the sketched ID's checks on a, omega and y, with n up to 65536 and y required
void check_sketch_product_batched(const rc_matrix &a, const rc_matrix &omega, int32_t count, const rc_matrix &y, int64_t ybs) {
    const char *who = "sketch_product_batched";
    const int64_t m = a.rows, n = a.cols, l = omega.rows;
    RC_REQUIRE(count >= 0, RC_INVALID_ARGUMENT, "%s: count = %d < 0", who, (int)count);
    RC_REQUIRE(m >= 1 && m <= 65536 && n >= 1 && n <= 65536 && l >= 1 && l <= 128, RC_INVALID_ARGUMENT,
               "%s: needs 1 <= m, n <= 65536 and 1 <= l <= 128 (got a %lld x %lld, omega %lld x %lld)", who, (long long)m, (long long)n, (long long)l,
               (long long)omega.cols);
    RC_REQUIRE(omega.cols == m, RC_INVALID_ARGUMENT, "%s: a has %lld rows but omega has %lld columns", who, (long long)m, (long long)omega.cols);
    RC_REQUIRE(y.rows == l && y.cols == n, RC_INVALID_ARGUMENT, "%s: y must be %lld x %lld (got %lld x %lld)", who, (long long)l, (long long)n,
               (long long)y.rows, (long long)y.cols);
    check_batch_stride(who, "y", ybs, y, count);
    if (count > 0) RC_REQUIRE(a.data && omega.data && y.data, RC_INVALID_ARGUMENT, "%s: null pointer", who);
}
// rc_demote_batched_* / rc_promote_batched_*: one shape on both sides, the sketched ID's tall domain, and dst's batch stride
void check_convert_batched(const char *who, const rc_matrix &src, int32_t count, const rc_matrix &dst, int64_t dbs) {
    RC_REQUIRE(count >= 0, RC_INVALID_ARGUMENT, "%s: count = %d < 0", who, (int)count);
    RC_REQUIRE(src.rows >= 1 && src.rows <= 65536 && src.cols >= 1 && src.cols <= 65536, RC_INVALID_ARGUMENT,
               "%s: needs 1 <= rows, cols <= 65536 (got src %lld x %lld)", who, (long long)src.rows, (long long)src.cols);
    RC_REQUIRE(dst.rows == src.rows && dst.cols == src.cols, RC_INVALID_ARGUMENT, "%s: dst must be %lld x %lld like src (got %lld x %lld)", who,
               (long long)src.rows, (long long)src.cols, (long long)dst.rows, (long long)dst.cols);
    check_batch_stride(who, "dst", dbs, dst, count);
    if (count > 0) RC_REQUIRE(src.data && dst.data, RC_INVALID_ARGUMENT, "%s: null pointer", who);
}
}  // namespace rc

namespace {

// One scalar type of the family, as its entry points see it: the element E of its views (from_c<E>) and what really differs between the
// real and the complex entry points: the complex recompressions take their tolerance in the real type and check the tall form under a name
// of their own.  Conjugation is the identity on real data (the real block operator and range step ignore the flag).
template <typename E>
struct Scalar {
    static constexpr bool complex = !std::is_same<E, real_t<E>>::value;
    using recompress_tol = std::conditional_t<complex, real_t<E>, double>;
    static constexpr int tall = complex ? RC_TALL_COMPLEX : RC_TALL;
};

// One range step of a power iteration on every block of a batch (sample_range_power_iteration, src/random_sampling.rs:131-158): the sketch
// y = omega a, an orthonormal basis q of its rows by a pivoted Householder QR of y^H and the projection p = a q^H (or its conjugate, p_conj), in
// one launch; p is orthonormalised by the tall recompression with right = I before its transpose is the next omega.  Only the complex entry
// points carry p_conj, so they are written out below this body instead of in RC_DEFINE_BATCHED.
template <typename E>
rc_status sketch_range_step(rc_context *ctx, const rc_matrix &a, int64_t abs, const rc_matrix &omega, int64_t obs, int32_t count, const rc_matrix &y,
                            int64_t ybs, const rc_matrix &q, int64_t qbs, const rc_matrix &p, int64_t pbs, int64_t *ranks, bool p_conj) {
    return guarded(ctx, [&] {
        check_sketch_range_step_batched(a, omega, count, y, ybs, q, qbs, p, pbs, ranks, Scalar<E>::complex);
        if (count == 0) return;
        batched_sketch_range_step<E>(ctx, from_c<E>(a), abs, from_c<E>(omega), obs, count, from_c<E>(y), ybs, from_c<E>(q), qbs, from_c<E>(p), pbs, ranks,
                                     p_conj);
    });
}

// the tall recompressions' plans as numbers: host arithmetic only, no context, no device
rc_status recompress_tall_plan(bool complex, int64_t m, int64_t n, int64_t inner, int32_t real_bytes, int64_t resident, int64_t *stages, int64_t *slot_bytes,
                               int64_t *grid) {
    if (!(m >= 1 && m <= 65536 && n >= 1 && n <= 512 && inner >= 1 && inner <= 128 && inner <= std::min(m, n)) || (real_bytes != 4 && real_bytes != 8) ||
        resident < 1 || !stages || !slot_bytes || !grid)
        return RC_INVALID_ARGUMENT;
    try {
        const bool wide = real_bytes == 8;
        (complex ? (wide ? batched_lowrank_recompress_tall_plan<cplx<double>> : batched_lowrank_recompress_tall_plan<cplx<float>>)
                 : (wide ? batched_lowrank_recompress_tall_plan<double> : batched_lowrank_recompress_tall_plan<float>))(m, n, inner, resident, stages,
                                                                                                                        slot_bytes, grid);
        return RC_OK;
    } catch (const Error &e) {
        return e.code;
    }
}

// the large recompressions' plans as numbers, likewise
rc_status recompress_large_plan(bool complex, int64_t m, int64_t n, int64_t inner, int32_t elem_bytes, int64_t resident, int64_t *stages_left, int64_t *stages_right,
                                int64_t *slot_bytes, int64_t *grid) {
    if (!(m >= 1 && m <= 65536 && n >= 1 && n <= 65536 && inner >= 1 && inner <= 128 && inner <= std::min(m, n)) || (elem_bytes != 4 && elem_bytes != 8) ||
        resident < 1 || !stages_left || !stages_right || !slot_bytes || !grid)
        return RC_INVALID_ARGUMENT;
    try {
        const bool wide = elem_bytes == 8;
        (complex ? (wide ? batched_lowrank_recompress_large_plan<cplx<double>> : batched_lowrank_recompress_large_plan<cplx<float>>)
                 : (wide ? batched_lowrank_recompress_large_plan<double> : batched_lowrank_recompress_large_plan<float>))(m, n, inner, resident, stages_left,
                                                                                                                          stages_right, slot_bytes, grid);
        return RC_OK;
    } catch (const Error &e) {
        return e.code;
    }
}

}  // namespace

// ================================================================================================ extern "C"
extern "C" {

// The regular entry points of one scalar type: SUF its suffix, R its real type, E its element, CX empty or `complex_` for the
// four stems that carry the word.  Every body is the same three steps; the rank rule (tol, 0: fixed rank k) runs on the device, without a host
// round trip; one path, stream-ordered, capturable.
#define RC_DEFINE_BATCHED(SUF, R, E, CX)                                                                                                     \
    /* rank-revealing column IDs of many small same-shaped matrices (the unit of rc_column_id_rank_*) in one launch */                       \
    rc_status rc_column_id_rank_batched_##SUF(rc_context *ctx, rc_matrix a, int64_t a_batch_stride, int32_t count, int64_t k, double tol,    \
                                              rc_matrix c, int64_t c_batch_stride, rc_matrix z, int64_t z_batch_stride, int64_t *col_ind,    \
                                              int64_t *ranks) {                                                                              \
        return guarded(ctx, [&] {                                                                                                            \
            k = check_column_id_rank_batched(a, count, k, tol, c, c_batch_stride, z, z_batch_stride, col_ind, ranks);                        \
            if (count == 0) return;                                                                                                          \
            batched_column_id<E>(ctx, from_c<E>(a), a_batch_stride, count, k, tol, from_c<E>(c), c_batch_stride, from_c<E>(z),               \
                                 z_batch_stride, col_ind, ranks);                                                                            \
        });                                                                                                                                  \
    }                                                                                                                                        \
    /* the two-sided ID A ~ C X R of the same batch (ColumnID::two_sided_id after the column ID), in the same one launch */                  \
    rc_status rc_two_sided_id_rank_batched_##SUF(rc_context *ctx, rc_matrix a, int64_t a_batch_stride, int32_t count, int64_t k, double tol, \
                                                 rc_matrix c, int64_t c_batch_stride, rc_matrix x, int64_t x_batch_stride, rc_matrix r,      \
                                                 int64_t r_batch_stride, int64_t *row_ind, int64_t *col_ind, int64_t *ranks) {               \
        return guarded(ctx, [&] {                                                                                                            \
            k = check_two_sided_id_rank_batched(a, count, k, tol, c, c_batch_stride, x, x_batch_stride, r, r_batch_stride, row_ind, col_ind, \
                                                ranks);                                                                                      \
            if (count == 0) return;                                                                                                          \
            batched_two_sided_id<E>(ctx, from_c<E>(a), a_batch_stride, count, k, tol, from_c<E>(c), c_batch_stride, from_c<E>(x),            \
                                    x_batch_stride, from_c<E>(r), r_batch_stride, row_ind, col_ind, ranks);                                  \
        });                                                                                                                                  \
    }                                                                                                                                        \
    /* truncated SVDs of the same batch (SVD::compute_from -> compress(.) per matrix), rank chosen per matrix on the singular values, */     \
    /* which are real for every scalar type; u (m x k), vt = V^H (k x n) */                                                                  \
    rc_status rc_svd_rank_batched_##SUF(rc_context *ctx, rc_matrix a, int64_t a_batch_stride, int32_t count, int64_t k, double tol,          \
                                        rc_matrix u, int64_t u_batch_stride, R *s, rc_matrix vt, int64_t vt_batch_stride, int64_t *ranks) {  \
        return guarded(ctx, [&] {                                                                                                            \
            k = check_svd_rank_batched(a, count, k, tol, u, u_batch_stride, s, vt, vt_batch_stride, ranks);                                  \
            if (count == 0) return;                                                                                                          \
            batched_svd<E>(ctx, from_c<E>(a), a_batch_stride, count, k, tol, from_c<E>(u), u_batch_stride, s, from_c<E>(vt),                 \
                           vt_batch_stride, ranks);                                                                                          \
        });                                                                                                                                  \
    }                                                                                                                                        \
    /* apply (b given) or rebuild (b.data == nullptr) every block of a batch from its factors, reading the ranks on the device: one */       \
    /* launch, no workspace */                                                                                                               \
    rc_status rc_lowrank_apply_batched_##SUF(rc_context *ctx, rc_matrix left, int64_t left_batch_stride, rc_matrix mid,                      \
                                             int64_t mid_batch_stride, const R *s, int64_t s_stride, rc_matrix right,                        \
                                             int64_t right_batch_stride, const int64_t *ranks, int32_t count, rc_matrix b,                   \
                                             int64_t b_batch_stride, rc_matrix y, int64_t y_batch_stride) {                                  \
        return guarded(ctx, [&] {                                                                                                            \
            check_lowrank_apply_batched(left, mid, right, count, b, y, y_batch_stride);                                                      \
            if (count == 0) return;                                                                                                          \
            batched_lowrank_apply<E>(ctx, from_c<E>(left), left_batch_stride, from_c<E>(mid), mid_batch_stride, s, s_stride,                 \
                                     from_c<E>(right), right_batch_stride, ranks, count, from_c<E>(b), b_batch_stride, from_c<E>(y),         \
                                     y_batch_stride);                                                                                        \
        });                                                                                                                                  \
    }                                                                                                                                        \
    /* y = H x for the block-sparse operator made of a low-rank batch and a dense batch placed by a block-CSR pattern on the device: */      \
    /* one launch, no workspace; conj is ignored on real data, where conjugation is the identity */                                          \
    rc_status rc_block_operator_apply_##SUF(rc_context *ctx, rc_matrix left, int64_t left_batch_stride, rc_matrix mid,                       \
                                            int64_t mid_batch_stride, const R *s, int64_t s_stride, rc_matrix right,                         \
                                            int64_t right_batch_stride, const int64_t *ranks, int32_t count, rc_matrix dense,                \
                                            int64_t dense_batch_stride, int32_t dense_count, const int64_t *group_ptr,                       \
                                            const int64_t *group_row, int32_t groups, const int64_t *entry_block, const int64_t *entry_col,  \
                                            rc_matrix x, rc_matrix y, int32_t accumulate, int32_t conj) {                                    \
        return guarded(ctx, [&] {                                                                                                            \
            const BlockPattern pat{group_ptr, group_row, entry_block, entry_col, groups};                                                    \
            const BlockShape sh = check_block_operator_apply(left, mid, right, count, dense, &dense_count, pat, x, y);                       \
            if (groups == 0) return;                                                                                                         \
            block_operator_apply<E>(ctx, from_c<E>(left), left_batch_stride, from_c<E>(mid), mid_batch_stride, s, s_stride,                  \
                                    from_c<E>(right), right_batch_stride, ranks, count, from_c<E>(dense), dense_batch_stride, dense_count,   \
                                    pat, sh, from_c<E>(x), from_c<E>(y), accumulate != 0, conj != 0);                                        \
        });                                                                                                                                  \
    }                                                                                                                                        \
    /* recompress every factor pair left (m x K) [mid (K x K)] [diag(s)] right (K x n) of a batch to a truncated SVD of rank */              \
    /* <= min(k, K) without forming the m x n blocks (SVD::to_qr / compute_from_range_estimate's scheme, src/svd.rs:150-163, :171-, */       \
    /* with compress's rank rule, :60-101): one launch; s, s_out (and the complex call's tol) in the real type, vt = V^H */                  \
    rc_status rc_lowrank_recompress_##CX##batched_##SUF(rc_context *ctx, rc_matrix left, int64_t left_batch_stride, rc_matrix mid,           \
                                                        int64_t mid_batch_stride, const R *s, int64_t s_stride, rc_matrix right,             \
                                                        int64_t right_batch_stride, const int64_t *in_ranks, int32_t count, int64_t k,       \
                                                        Scalar<E>::recompress_tol tol, rc_matrix u, int64_t u_batch_stride, R *s_out,        \
                                                        rc_matrix vt, int64_t vt_batch_stride, int64_t *ranks) {                             \
        return guarded(ctx, [&] {                                                                                                            \
            check_lowrank_recompress_batched(left, mid, right, count, k, tol, u, u_batch_stride, s_out, vt, vt_batch_stride, ranks);         \
            if (count == 0) return;                                                                                                          \
            batched_lowrank_recompress<E>(ctx, from_c<E>(left), left_batch_stride, from_c<E>(mid), mid_batch_stride, s, s_stride,            \
                                          from_c<E>(right), right_batch_stride, in_ranks, count, k, (double)tol, from_c<E>(u),               \
                                          u_batch_stride, s_out, from_c<E>(vt), vt_batch_stride, ranks);                                     \
        });                                                                                                                                  \
    }                                                                                                                                        \
    /* the same for a tall left factor (m <= 65536): the same checks with that bound under the call's own name, the left factor by a */      \
    /* flat Householder TSQR inside the launch */                                                                                            \
    rc_status rc_lowrank_recompress_tall_##CX##batched_##SUF(rc_context *ctx, rc_matrix left, int64_t left_batch_stride, rc_matrix mid,      \
                                                             int64_t mid_batch_stride, const R *s, int64_t s_stride, rc_matrix right,        \
                                                             int64_t right_batch_stride, const int64_t *in_ranks, int32_t count, int64_t k,  \
                                                             Scalar<E>::recompress_tol tol, rc_matrix u, int64_t u_batch_stride, R *s_out,   \
                                                             rc_matrix vt, int64_t vt_batch_stride, int64_t *ranks) {                        \
        return guarded(ctx, [&] {                                                                                                            \
            check_lowrank_recompress_batched(left, mid, right, count, k, tol, u, u_batch_stride, s_out, vt, vt_batch_stride, ranks,          \
                                             Scalar<E>::tall);                                                                               \
            if (count == 0) return;                                                                                                          \
            batched_lowrank_recompress_tall<E>(ctx, from_c<E>(left), left_batch_stride, from_c<E>(mid), mid_batch_stride, s, s_stride,       \
                                               from_c<E>(right), right_batch_stride, in_ranks, count, k, (double)tol, from_c<E>(u),          \
                                               u_batch_stride, s_out, from_c<E>(vt), vt_batch_stride, ranks);                                \
        });                                                                                                                                  \
    }                                                                                                                                        \
    /* the one-pass randomized column ID of every block of a batch: the sketch y = omega a (l x n, nothing conjugated) and the column */     \
    /* ID of y in one launch, c gathered from a (sample_range_by_rank's projection, src/random_sampling.rs, then */                          \
    /* QR::compute_from_range_estimate + column_id, src/qr.rs:311-323, per block) */                                                         \
    rc_status rc_sketch_column_id_rank_##CX##batched_##SUF(rc_context *ctx, rc_matrix a, int64_t a_batch_stride, rc_matrix omega,            \
                                                           int64_t omega_batch_stride, int32_t count, int64_t k, double tol, rc_matrix y,    \
                                                           int64_t y_batch_stride, rc_matrix c, int64_t c_batch_stride, rc_matrix z,         \
                                                           int64_t z_batch_stride, int64_t *col_ind, int64_t *ranks) {                       \
        return guarded(ctx, [&] {                                                                                                            \
            const int64_t kk = check_sketch_column_id_rank_batched(a, omega, count, k, tol, y, y_batch_stride, c, c_batch_stride, z,         \
                                                                   z_batch_stride, col_ind, ranks);                                          \
            if (count == 0) return;                                                                                                          \
            batched_sketch_column_id<E>(ctx, from_c<E>(a), a_batch_stride, from_c<E>(omega), omega_batch_stride, count, kk, tol,             \
                                        from_c<E>(y), y_batch_stride, from_c<E>(c), c_batch_stride, from_c<E>(z), z_batch_stride, col_ind,   \
                                        ranks);                                                                                              \
        });                                                                                                                                  \
    }                                                                                                                                        \
    /* ||a_i - left_i mid_i diag(s_i) right_i||_F at each block's rank, ||a_i||_F and optionally the residual blocks, for the factors */     \
    /* of any batched compressor: the reference's rel_diff_fro(x.to_mat(), a) per block (src/lib.rs), in one launch and on the */            \
    /* sketched ID's domain; s, err and nrm in the real type */                                                                              \
    rc_status rc_lowrank_residual_batched_##SUF(rc_context *ctx, rc_matrix a, int64_t a_batch_stride, rc_matrix left,                        \
                                                int64_t left_batch_stride, rc_matrix mid, int64_t mid_batch_stride, const R *s,              \
                                                int64_t s_stride, rc_matrix right, int64_t right_batch_stride, const int64_t *ranks,         \
                                                int32_t count, rc_matrix e, int64_t e_batch_stride, R *err, R *nrm) {                        \
        return guarded(ctx, [&] {                                                                                                            \
            check_lowrank_residual_batched(a, left, mid, right, count, e, e_batch_stride, err);                                              \
            if (count == 0) return;                                                                                                          \
            batched_lowrank_residual<E>(ctx, from_c<E>(a), a_batch_stride, from_c<E>(left), left_batch_stride, from_c<E>(mid),               \
                                        mid_batch_stride, s, s_stride, from_c<E>(right), right_batch_stride, ranks, count, from_c<E>(e),     \
                                        e_batch_stride, err, nrm);                                                                           \
        });                                                                                                                                  \
    }

RC_DEFINE_BATCHED(f64, double, double, )
RC_DEFINE_BATCHED(f32, float, float, )
RC_DEFINE_BATCHED(c64, double, cplx<double>, complex_)
RC_DEFINE_BATCHED(c32, float, cplx<float>, complex_)

// the recompression with both factors tall (m, n <= 65536): the tall call's signature (the complex tol in the real type) and the pair's checks
// with those bounds under the call's own name (MODE), both factors by a flat Householder TSQR inside the launch.  The complex stem is
// rc_lowrank_recompress_complex_large_batched_, "complex" before "large", so the stanza stands outside RC_DEFINE_BATCHED: the names the real
// pair's section proposed for a complex twin (..._large_batched_c64 / _c32, ..._large_complex_batched_c64 / _c32) are pinned as absent by
// that pair's ABI test and stay absent.
#define RC_DEFINE_RECOMPRESS_LARGE(STEM, SUF, R, E, MODE)                                                                                    \
    rc_status STEM##SUF(rc_context *ctx, rc_matrix left, int64_t left_batch_stride, rc_matrix mid, int64_t mid_batch_stride, const R *s,     \
                        int64_t s_stride, rc_matrix right, int64_t right_batch_stride, const int64_t *in_ranks, int32_t count, int64_t k,    \
                        Scalar<E>::recompress_tol tol, rc_matrix u, int64_t u_batch_stride, R *s_out, rc_matrix vt, int64_t vt_batch_stride, \
                        int64_t *ranks) {                                                                                                    \
        return guarded(ctx, [&] {                                                                                                            \
            check_lowrank_recompress_batched(left, mid, right, count, k, tol, u, u_batch_stride, s_out, vt, vt_batch_stride, ranks, MODE);   \
            if (count == 0) return;                                                                                                          \
            batched_lowrank_recompress_large<E>(ctx, from_c<E>(left), left_batch_stride, from_c<E>(mid), mid_batch_stride, s, s_stride,      \
                                                from_c<E>(right), right_batch_stride, in_ranks, count, k, (double)tol, from_c<E>(u),         \
                                                u_batch_stride, s_out, from_c<E>(vt), vt_batch_stride, ranks);                               \
        });                                                                                                                                  \
    }
RC_DEFINE_RECOMPRESS_LARGE(rc_lowrank_recompress_large_batched_, f64, double, double, RC_LARGE)
RC_DEFINE_RECOMPRESS_LARGE(rc_lowrank_recompress_large_batched_, f32, float, float, RC_LARGE)
RC_DEFINE_RECOMPRESS_LARGE(rc_lowrank_recompress_complex_large_batched_, c64, double, cplx<double>, RC_LARGE_COMPLEX)
RC_DEFINE_RECOMPRESS_LARGE(rc_lowrank_recompress_complex_large_batched_, c32, float, cplx<float>, RC_LARGE_COMPLEX)

// the sketch y = omega a of every block of a batch and nothing else, for blocks of up to 65536 columns: the front end of a randomized SVD of
// wide or square blocks, and, on transposed views, its projection p = a q^T.  Real scalars only, like the large recompression.
#define RC_DEFINE_SKETCH_PRODUCT(SUF, R)                                                                                                     \
    rc_status rc_sketch_product_batched_##SUF(rc_context *ctx, rc_matrix a, int64_t a_batch_stride, rc_matrix omega,                         \
                                              int64_t omega_batch_stride, int32_t count, rc_matrix y, int64_t y_batch_stride) {              \
        return guarded(ctx, [&] {                                                                                                            \
            check_sketch_product_batched(a, omega, count, y, y_batch_stride);                                                                \
            if (count == 0) return;                                                                                                          \
            batched_sketch_product<R>(ctx, from_c<R>(a), a_batch_stride, from_c<R>(omega), omega_batch_stride, count, from_c<R>(y),          \
                                      y_batch_stride);                                                                                       \
        });                                                                                                                                  \
    }
RC_DEFINE_SKETCH_PRODUCT(f64, double)
RC_DEFINE_SKETCH_PRODUCT(f32, float)

#define RC_RANGE_STEP_PARAMS                                                                                                                           \
    rc_context *ctx, rc_matrix a, int64_t a_batch_stride, rc_matrix omega, int64_t omega_batch_stride, int32_t count, rc_matrix y, int64_t y_batch_stride, \
        rc_matrix q, int64_t q_batch_stride, rc_matrix p, int64_t p_batch_stride, int64_t *ranks
#define RC_RANGE_STEP_ARGS ctx, a, a_batch_stride, omega, omega_batch_stride, count, y, y_batch_stride, q, q_batch_stride, p, p_batch_stride, ranks
rc_status rc_sketch_range_step_batched_f64(RC_RANGE_STEP_PARAMS) { return sketch_range_step<double>(RC_RANGE_STEP_ARGS, false); }
rc_status rc_sketch_range_step_batched_f32(RC_RANGE_STEP_PARAMS) { return sketch_range_step<float>(RC_RANGE_STEP_ARGS, false); }
rc_status rc_sketch_range_step_complex_batched_c64(RC_RANGE_STEP_PARAMS, int32_t p_conj) {
    return sketch_range_step<cplx<double>>(RC_RANGE_STEP_ARGS, p_conj != 0);
}
rc_status rc_sketch_range_step_complex_batched_c32(RC_RANGE_STEP_PARAMS, int32_t p_conj) {
    return sketch_range_step<cplx<float>>(RC_RANGE_STEP_ARGS, p_conj != 0);
}

rc_status rc_lowrank_recompress_tall_batched_plan(int64_t m, int64_t n, int64_t inner, int32_t elem_bytes, int64_t resident, int64_t *stages,
                                                  int64_t *slot_bytes, int64_t *grid) {
    return recompress_tall_plan(false, m, n, inner, elem_bytes, resident, stages, slot_bytes, grid);
}
rc_status rc_lowrank_recompress_large_batched_plan(int64_t m, int64_t n, int64_t inner, int32_t elem_bytes, int64_t resident, int64_t *stages_left,
                                                   int64_t *stages_right, int64_t *slot_bytes, int64_t *grid) {
    return recompress_large_plan(false, m, n, inner, elem_bytes, resident, stages_left, stages_right, slot_bytes, grid);
}
// (real_bytes 8: c64, 4: c32)
rc_status rc_lowrank_recompress_tall_complex_batched_plan(int64_t m, int64_t n, int64_t inner, int32_t real_bytes, int64_t resident, int64_t *stages,
                                                          int64_t *slot_bytes, int64_t *grid) {
    return recompress_tall_plan(true, m, n, inner, real_bytes, resident, stages, slot_bytes, grid);
}
rc_status rc_lowrank_recompress_complex_large_batched_plan(int64_t m, int64_t n, int64_t inner, int32_t real_bytes, int64_t resident, int64_t *stages_left,
                                                           int64_t *stages_right, int64_t *slot_bytes, int64_t *grid) {
    return recompress_large_plan(true, m, n, inner, real_bytes, resident, stages_left, stages_right, slot_bytes, grid);
}

// f32 (c32) storage under f64 (c64) arithmetic (kernels_batched_apply.hip, kernels_block_operator.hip, kernels_convert.hip): the full-precision
// calls' checks on views of the same shapes; HI the suffix of the arithmetic, LO of the storage, COMPLEX what the launchers take as complex_data
#define RC_DEFINE_MIXED(HI, LO, COMPLEX)                                                                                                     \
    rc_status rc_lowrank_apply_mixed_batched_##HI(rc_context *ctx, rc_matrix left, int64_t left_batch_stride, rc_matrix mid,                 \
                                                  int64_t mid_batch_stride, const double *s, int64_t s_stride, rc_matrix right,              \
                                                  int64_t right_batch_stride, const int64_t *ranks, int32_t count, rc_matrix b,              \
                                                  int64_t b_batch_stride, rc_matrix y, int64_t y_batch_stride) {                             \
        return guarded(ctx, [&] {                                                                                                            \
            check_lowrank_apply_batched(left, mid, right, count, b, y, y_batch_stride);                                                      \
            if (count == 0) return;                                                                                                          \
            batched_lowrank_apply_mixed(ctx, COMPLEX, left, left_batch_stride, mid, mid_batch_stride, s, s_stride, right, right_batch_stride,\
                                        ranks, count, b, b_batch_stride, y, y_batch_stride);                                                 \
        });                                                                                                                                  \
    }                                                                                                                                        \
    /* conj is ignored on real data, where conjugation is the identity */                                                                    \
    rc_status rc_block_operator_apply_mixed_##HI(rc_context *ctx, rc_matrix left, int64_t left_batch_stride, rc_matrix mid,                  \
                                                 int64_t mid_batch_stride, const double *s, int64_t s_stride, rc_matrix right,               \
                                                 int64_t right_batch_stride, const int64_t *ranks, int32_t count, rc_matrix dense,           \
                                                 int64_t dense_batch_stride, int32_t dense_count, const int64_t *group_ptr,                  \
                                                 const int64_t *group_row, int32_t groups, const int64_t *entry_block,                       \
                                                 const int64_t *entry_col, rc_matrix x, rc_matrix y, int32_t accumulate, int32_t conj) {     \
        return guarded(ctx, [&] {                                                                                                            \
            const BlockPattern pat{group_ptr, group_row, entry_block, entry_col, groups};                                                    \
            const BlockShape sh = check_block_operator_apply(left, mid, right, count, dense, &dense_count, pat, x, y);                       \
            if (groups == 0) return;                                                                                                         \
            block_operator_apply_mixed(ctx, COMPLEX, left, left_batch_stride, mid, mid_batch_stride, s, s_stride, right, right_batch_stride, \
                                       ranks, count, dense, dense_batch_stride, dense_count, pat, sh, x, y, accumulate != 0,                 \
                                       COMPLEX && conj != 0);                                                                                \
        });                                                                                                                                  \
    }                                                                                                                                        \
    rc_status rc_demote_batched_##HI(rc_context *ctx, rc_matrix src, int64_t src_batch_stride, int32_t count, rc_matrix dst,                 \
                                     int64_t dst_batch_stride, int64_t *overflow) {                                                          \
        return guarded(ctx, [&] {                                                                                                            \
            check_convert_batched("demote_batched", src, count, dst, dst_batch_stride);                                                      \
            if (count == 0) return;                                                                                                          \
            batched_demote(ctx, COMPLEX, src, src_batch_stride, count, dst, dst_batch_stride, overflow);                                     \
        });                                                                                                                                  \
    }                                                                                                                                        \
    rc_status rc_promote_batched_##LO(rc_context *ctx, rc_matrix src, int64_t src_batch_stride, int32_t count, rc_matrix dst,                \
                                      int64_t dst_batch_stride) {                                                                            \
        return guarded(ctx, [&] {                                                                                                            \
            check_convert_batched("promote_batched", src, count, dst, dst_batch_stride);                                                     \
            if (count == 0) return;                                                                                                          \
            batched_promote(ctx, COMPLEX, src, src_batch_stride, count, dst, dst_batch_stride);                                              \
        });                                                                                                                                  \
    }

RC_DEFINE_MIXED(f64, f32, false)
RC_DEFINE_MIXED(c64, c32, true)

// The _f32 names of the three stems above are the header's rule that every _f64 entry point has an _f32 one.  They would be f32 arithmetic
// over 16-bit storage, which this library does not build: declared, exported and always refused, so that a caller finds out at the call.
static rc_status mixed_f32_not_built(rc_context *ctx, const char *who) {
    return guarded(ctx, [&] { fail(RC_INVALID_ARGUMENT, "%s: f32 arithmetic over 16-bit storage is not built; the mixed calls are the _f64 and _c64 ones", who); });
}
rc_status rc_lowrank_apply_mixed_batched_f32(rc_context *ctx, rc_matrix, int64_t, rc_matrix, int64_t, const float *, int64_t, rc_matrix, int64_t, const int64_t *,
                                             int32_t, rc_matrix, int64_t, rc_matrix, int64_t) {
    return mixed_f32_not_built(ctx, "lowrank_apply_mixed_batched_f32");
}
rc_status rc_block_operator_apply_mixed_f32(rc_context *ctx, rc_matrix, int64_t, rc_matrix, int64_t, const float *, int64_t, rc_matrix, int64_t, const int64_t *,
                                            int32_t, rc_matrix, int64_t, int32_t, const int64_t *, const int64_t *, int32_t, const int64_t *, const int64_t *,
                                            rc_matrix, rc_matrix, int32_t, int32_t) {
    return mixed_f32_not_built(ctx, "block_operator_apply_mixed_f32");
}
rc_status rc_demote_batched_f32(rc_context *ctx, rc_matrix, int64_t, int32_t, rc_matrix, int64_t, int64_t *) { return mixed_f32_not_built(ctx, "demote_batched_f32"); }

}  // extern "C"
