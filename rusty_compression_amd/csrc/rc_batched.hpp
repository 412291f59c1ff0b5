// The batched family (many small or tall same-shaped blocks in one launch): its kernel launchers (kernels_batched_*.hip,
// kernels_block_operator.hip, kernels_convert.hip) and the argument checks of its entry points (rc_batched_api.hip).  rc_common.hpp ends by
// including this header, so every translation unit sees it.
#pragma once

#include "rc_common.hpp"

namespace rc {

// rank-revealing column IDs of `count` same-shaped small matrices in one launch (kernels_batched_id.hip): matrix i is a, cm, z moved by
// i * abs, i * cbs, i * zbs elements; col_ind count x n, ranks count (arguments checked by the caller)
template <typename T> void batched_column_id(rc_context *c, Mat<T> a, int64_t abs, int32_t count, int64_t k, double tol, Mat<T> cm, int64_t cbs, Mat<T> z,
                                             int64_t zbs, int64_t *col_ind, int64_t *ranks);
// the two-sided ID of the same batch (kernels_batched_id.hip): matrix i is a, cm (m x k), x (k x k), z (k x n) moved by i * abs, i * cbs,
// i * xbs, i * zbs elements; row_ind count x m, col_ind count x n, ranks count (arguments checked by the caller)
template <typename T> void batched_two_sided_id(rc_context *c, Mat<T> a, int64_t abs, int32_t count, int64_t k, double tol, Mat<T> cm, int64_t cbs, Mat<T> x,
                                                int64_t xbs, Mat<T> z, int64_t zbs, int64_t *row_ind, int64_t *col_ind, int64_t *ranks);
// truncated SVDs of the same kind of batch (kernels_batched_id.hip): matrix i is a, u (m x k), vt (k x n) moved by i * abs, i * ubs,
// i * vbs elements; s count x min(m, n), ranks count (arguments checked by the caller)
template <typename T> void batched_svd(rc_context *c, Mat<T> a, int64_t abs, int32_t count, int64_t k, double tol, Mat<T> u, int64_t ubs, T *s, Mat<T> vt,
                                       int64_t vbs, int64_t *ranks);
// the complex twins (kernels_batched_id_c.hip), R = double (c64) or float (c32): the same layout with interleaved-complex views
template <typename R> void batched_column_id_c(rc_context *c, const rc_matrix &a, int64_t abs, int32_t count, int64_t k, double tol, const rc_matrix &cm,
                                               int64_t cbs, const rc_matrix &z, int64_t zbs, int64_t *col_ind, int64_t *ranks);
template <typename R> void batched_two_sided_id_c(rc_context *c, const rc_matrix &a, int64_t abs, int32_t count, int64_t k, double tol, const rc_matrix &cm,
                                                  int64_t cbs, const rc_matrix &x, int64_t xbs, const rc_matrix &z, int64_t zbs, int64_t *row_ind,
                                                  int64_t *col_ind, int64_t *ranks);
template <typename R> void batched_svd_c(rc_context *c, const rc_matrix &a, int64_t abs, int32_t count, int64_t k, double tol, const rc_matrix &u, int64_t ubs,
                                         R *s, const rc_matrix &vt, int64_t vbs, int64_t *ranks);
// the argument checks of rc_column_id_rank_batched_* / rc_two_sided_id_rank_batched_* / rc_svd_rank_batched_* (rc_batched_api.hip), one for every
// scalar type: the views carry the shapes and strides (in elements of the scalar type), they and the pointers only their null-ness.  Return k
// clamped to min(m, n); the caller returns when count == 0.
int64_t check_column_id_rank_batched(const rc_matrix &a, int32_t count, int64_t k, double tol, const rc_matrix &cm, int64_t cbs, const rc_matrix &z,
                                     int64_t zbs, const int64_t *col_ind, const int64_t *ranks);
int64_t check_two_sided_id_rank_batched(const rc_matrix &a, int32_t count, int64_t k, double tol, const rc_matrix &cm, int64_t cbs, const rc_matrix &x,
                                        int64_t xbs, const rc_matrix &r, int64_t rbs, const int64_t *row_ind, const int64_t *col_ind, const int64_t *ranks);
int64_t check_svd_rank_batched(const rc_matrix &a, int32_t count, int64_t k, double tol, const rc_matrix &u, int64_t ubs, const void *s, const rc_matrix &vt,
                               int64_t vbs, const int64_t *ranks);
// apply or rebuild the factors of such a batch in one rank-aware launch (kernels_batched_apply.hip): block i is left (m x k), mid (k x k, p == nullptr:
// none), right (k x n), b (n x nrhs, p == nullptr: reconstruct) and y each moved by i times its batch stride, s + i * s_stride its k real scales (nullptr:
// none), ranks count device values (nullptr: every rank is k); the complex twin takes interleaved-complex views (arguments checked by the caller)
template <typename T> void batched_lowrank_apply(rc_context *c, Mat<T> left, int64_t lbs, Mat<T> mid, int64_t mbs, const T *s, int64_t s_stride, Mat<T> right,
                                                 int64_t rbs, const int64_t *ranks, int32_t count, Mat<T> b, int64_t bbs, Mat<T> y, int64_t ybs);
template <typename R> void batched_lowrank_apply_c(rc_context *c, const rc_matrix &left, int64_t lbs, const rc_matrix &mid, int64_t mbs, const R *s,
                                                   int64_t s_stride, const rc_matrix &right, int64_t rbs, const int64_t *ranks, int32_t count,
                                                   const rc_matrix &b, int64_t bbs, const rc_matrix &y, int64_t ybs);
// the argument checks of rc_lowrank_apply_batched_* (rc_batched_api.hip), one for every scalar type like the three above; the caller returns when
// count == 0
void check_lowrank_apply_batched(const rc_matrix &left, const rc_matrix &mid, const rc_matrix &right, int32_t count, const rc_matrix &b, const rc_matrix &y,
                                 int64_t ybs);
// y = H x for the block-sparse operator whose blocks are the factors of such a batch and a batch of dense m x n blocks, placed by a block-CSR
// pattern on the device (kernels_block_operator.hip, rc_block_operator_apply_*): the low-rank operands as in batched_lowrank_apply, block ids
// count .. count + dense_count - 1 are dense (p == nullptr: none); shape holds m, n and k (0 without a low-rank batch) as the check returns them;
// the complex twin takes interleaved-complex views and conjugates the blocks on load when conj is set (arguments checked by the caller)
struct BlockPattern {
    const int64_t *group_ptr, *group_row, *entry_block, *entry_col;
    int32_t groups;
};
struct BlockShape {
    int m, n, k;
};
template <typename T> void block_operator_apply(rc_context *c, Mat<T> left, int64_t lbs, Mat<T> mid, int64_t mbs, const T *s, int64_t s_stride, Mat<T> right,
                                                int64_t rbs, const int64_t *ranks, int32_t count, Mat<T> dense, int64_t dbs, int32_t dense_count,
                                                const BlockPattern &pat, BlockShape shape, Mat<T> x, Mat<T> y, bool accumulate);
template <typename R> void block_operator_apply_c(rc_context *c, const rc_matrix &left, int64_t lbs, const rc_matrix &mid, int64_t mbs, const R *s,
                                                  int64_t s_stride, const rc_matrix &right, int64_t rbs, const int64_t *ranks, int32_t count,
                                                  const rc_matrix &dense, int64_t dbs, int32_t dense_count, const BlockPattern &pat, BlockShape shape,
                                                  const rc_matrix &x, const rc_matrix &y, bool accumulate, bool conj);
// the argument checks of rc_block_operator_apply_* (rc_batched_api.hip), one for every scalar type; dense_count is zeroed when dense.data == nullptr;
// the caller returns when pat.groups == 0
BlockShape check_block_operator_apply(const rc_matrix &left, const rc_matrix &mid, const rc_matrix &right, int32_t count, const rc_matrix &dense,
                                      int32_t *dense_count, const BlockPattern &pat, const rc_matrix &x, const rc_matrix &y);
// the mixed-storage forms of the two above (rc_lowrank_apply_mixed_batched_*, rc_block_operator_apply_mixed_*): left, mid and right are views of
// f32 (c32 when complex_data) data with strides in their own elements, b / dense / x / y are f64 (c64) and s is double; the bits are those of the
// full-precision call on promoted factors (arguments checked by the caller, on the shapes alone)
void batched_lowrank_apply_mixed(rc_context *c, bool complex_data, const rc_matrix &left, int64_t lbs, const rc_matrix &mid, int64_t mbs, const double *s,
                                 int64_t s_stride, const rc_matrix &right, int64_t rbs, const int64_t *ranks, int32_t count, const rc_matrix &b, int64_t bbs,
                                 const rc_matrix &y, int64_t ybs);
void block_operator_apply_mixed(rc_context *c, bool complex_data, const rc_matrix &left, int64_t lbs, const rc_matrix &mid, int64_t mbs, const double *s,
                                int64_t s_stride, const rc_matrix &right, int64_t rbs, const int64_t *ranks, int32_t count, const rc_matrix &dense, int64_t dbs,
                                int32_t dense_count, const BlockPattern &pat, BlockShape shape, const rc_matrix &x, const rc_matrix &y, bool accumulate, bool conj);
// strided batched conversion f64 -> f32 (c64 -> c32) and back (kernels_convert.hip): block i is src and dst moved by i times their batch strides;
// overflow (count device values, nullptr: not counted) receives the finite elements of each block that became non-finite
void batched_demote(rc_context *c, bool complex_data, const rc_matrix &src, int64_t sbs, int32_t count, const rc_matrix &dst, int64_t dbs, int64_t *overflow);
void batched_promote(rc_context *c, bool complex_data, const rc_matrix &src, int64_t sbs, int32_t count, const rc_matrix &dst, int64_t dbs);
// the argument checks of rc_demote_batched_* / rc_promote_batched_* (rc_batched_api.hip); the caller returns when count == 0
void check_convert_batched(const char *who, const rc_matrix &src, int32_t count, const rc_matrix &dst, int64_t dbs);
// recompress the factor pairs of such a batch to truncated SVDs without forming the blocks (kernels_batched_id.hip): block i is left (m x K), mid (K x K,
// p == nullptr: none), right (K x n), u (m x min(k, K)) and vt (min(k, K) x n) each moved by i times its batch stride, s + i * s_stride its K real scales
// (nullptr: none), in_ranks count device values (nullptr: every inner rank is K); s_out count x K, ranks count (arguments checked by the caller)
template <typename T> void batched_lowrank_recompress(rc_context *c, Mat<T> left, int64_t lbs, Mat<T> mid, int64_t mbs, const T *s, int64_t s_stride,
                                                      Mat<T> right, int64_t rbs, const int64_t *in_ranks, int32_t count, int64_t k, double tol, Mat<T> u,
                                                      int64_t ubs, T *s_out, Mat<T> vt, int64_t vbs, int64_t *ranks);
// the same with a tall left factor (m <= 65536): flat Householder TSQR of left in stages of 512 rows, stored in the workgroup's slot; and its plan
// as numbers: stages at inner width K, bytes of one slot, the grid its 2 GiB workspace bound leaves of `resident` workgroups
template <typename T> void batched_lowrank_recompress_tall(rc_context *c, Mat<T> left, int64_t lbs, Mat<T> mid, int64_t mbs, const T *s, int64_t s_stride,
                                                           Mat<T> right, int64_t rbs, const int64_t *in_ranks, int32_t count, int64_t k, double tol, Mat<T> u,
                                                           int64_t ubs, T *s_out, Mat<T> vt, int64_t vbs, int64_t *ranks);
void batched_lowrank_recompress_tall_plan(int64_t m, int64_t n, int64_t K, bool f64, int64_t resident, int64_t *stages, int64_t *slot_bytes, int64_t *grid);
// the same with both factors tall (m, n <= 65536; k_batched_recompress<T, true, true>): right^T by the same stages behind left's in the slot; n <= 512
// is the tall call bit for bit.  Its plan as numbers: the stages of both factors at inner width K, bytes of one slot, the grid
template <typename T> void batched_lowrank_recompress_large(rc_context *c, Mat<T> left, int64_t lbs, Mat<T> mid, int64_t mbs, const T *s, int64_t s_stride,
                                                            Mat<T> right, int64_t rbs, const int64_t *in_ranks, int32_t count, int64_t k, double tol, Mat<T> u,
                                                            int64_t ubs, T *s_out, Mat<T> vt, int64_t vbs, int64_t *ranks);
void batched_lowrank_recompress_large_plan(int64_t m, int64_t n, int64_t K, bool f64, int64_t resident, int64_t *stages_left, int64_t *stages_right,
                                           int64_t *slot_bytes, int64_t *grid);
// the complex twin (kernels_batched_id_c.hip), R = double (c64) or float (c32): interleaved-complex views, strides in complex elements, s and s_out
// real, vt = V^H
template <typename R> void batched_lowrank_recompress_c(rc_context *c, const rc_matrix &left, int64_t lbs, const rc_matrix &mid, int64_t mbs, const R *s,
                                                        int64_t s_stride, const rc_matrix &right, int64_t rbs, const int64_t *in_ranks, int32_t count, int64_t k,
                                                        double tol, const rc_matrix &u, int64_t ubs, R *s_out, const rc_matrix &vt, int64_t vbs, int64_t *ranks);
// the same with a tall left factor (m <= 65536; k_batched_recompress_c<R, true>), and its plan as numbers like the real one's (c64: else c32)
template <typename R> void batched_lowrank_recompress_tall_c(rc_context *c, const rc_matrix &left, int64_t lbs, const rc_matrix &mid, int64_t mbs, const R *s,
                                                             int64_t s_stride, const rc_matrix &right, int64_t rbs, const int64_t *in_ranks, int32_t count,
                                                             int64_t k, double tol, const rc_matrix &u, int64_t ubs, R *s_out, const rc_matrix &vt, int64_t vbs,
                                                             int64_t *ranks);
void batched_lowrank_recompress_tall_c_plan(int64_t m, int64_t n, int64_t K, bool c64, int64_t resident, int64_t *stages, int64_t *slot_bytes, int64_t *grid);
// the same with both factors tall (m, n <= 65536; k_batched_recompress_c<R, true, true>): right^T by the same stages behind left's in the slot;
// n <= 512 is the tall complex call bit for bit.  Its plan as numbers like the real large one's (c64: else c32)
template <typename R> void batched_lowrank_recompress_large_c(rc_context *c, const rc_matrix &left, int64_t lbs, const rc_matrix &mid, int64_t mbs, const R *s,
                                                              int64_t s_stride, const rc_matrix &right, int64_t rbs, const int64_t *in_ranks, int32_t count,
                                                              int64_t k, double tol, const rc_matrix &u, int64_t ubs, R *s_out, const rc_matrix &vt, int64_t vbs,
                                                              int64_t *ranks);
void batched_lowrank_recompress_large_c_plan(int64_t m, int64_t n, int64_t K, bool c64, int64_t resident, int64_t *stages_left, int64_t *stages_right,
                                             int64_t *slot_bytes, int64_t *grid);
// the argument checks of rc_lowrank_recompress_batched_* and rc_lowrank_recompress_complex_batched_* (rc_batched_api.hip), one for every scalar type
// like those above; the caller returns when count == 0.  tall: the bound m <= 65536 under rc_lowrank_recompress_tall_batched_*'s name (RC_TALL) or
// rc_lowrank_recompress_tall_complex_batched_*'s (RC_TALL_COMPLEX); RC_LARGE: m, n <= 65536 under rc_lowrank_recompress_large_batched_*'s, and
// RC_LARGE_COMPLEX the same under rc_lowrank_recompress_complex_large_batched_*'s
enum { RC_NOT_TALL = 0, RC_TALL = 1, RC_TALL_COMPLEX = 2, RC_LARGE = 3, RC_LARGE_COMPLEX = 4 };
void check_lowrank_recompress_batched(const rc_matrix &left, const rc_matrix &mid, const rc_matrix &right, int32_t count, int64_t k, double tol,
                                      const rc_matrix &u, int64_t ubs, const void *s_out, const rc_matrix &vt, int64_t vbs, const int64_t *ranks,
                                      int tall = RC_NOT_TALL);
// the column ID of the sketch omega a of every block of a batch (kernels_batched_id.hip): block i is a (m x n), omega (l x m, l <= 128), y (l x n,
// p == nullptr: not written), cm (m x kk) and z (kk x n) each moved by i times its batch stride (0 is legal for a and omega), kk = min(k, l, n) already
// clamped; col_ind count x n, ranks count (arguments checked by the caller)
template <typename T> void batched_sketch_column_id(rc_context *c, Mat<T> a, int64_t abs, Mat<T> omega, int64_t obs, int32_t count, int64_t kk, double tol,
                                                    Mat<T> y, int64_t ybs, Mat<T> cm, int64_t cbs, Mat<T> z, int64_t zbs, int64_t *col_ind, int64_t *ranks);
// the complex twin (kernels_batched_id_c.hip), R = double (c64) or float (c32): interleaved-complex views, strides in complex elements, nothing conjugated
template <typename R> void batched_sketch_column_id_c(rc_context *c, const rc_matrix &a, int64_t abs, const rc_matrix &omega, int64_t obs, int32_t count,
                                                      int64_t kk, double tol, const rc_matrix &y, int64_t ybs, const rc_matrix &cm, int64_t cbs,
                                                      const rc_matrix &z, int64_t zbs, int64_t *col_ind, int64_t *ranks);
// the argument checks of rc_sketch_column_id_rank_batched_* and rc_sketch_column_id_rank_complex_batched_* (rc_batched_api.hip), one for every scalar
// type like those above.  Return kk = min(k, l, n); the caller returns when count == 0.
int64_t check_sketch_column_id_rank_batched(const rc_matrix &a, const rc_matrix &omega, int32_t count, int64_t k, double tol, const rc_matrix &y, int64_t ybs,
                                            const rc_matrix &cm, int64_t cbs, const rc_matrix &z, int64_t zbs, const int64_t *col_ind, const int64_t *ranks);
// one range step of every block of a batch (kernels_batched_id.hip, k_batched_range_step): the sketch y = omega a (l x n, p == nullptr: not written), an
// orthonormal basis q (l x n, rows from the block's rank on zero) of its rows and the projection p = a q^T (m x l), each moved by i times its batch
// stride (0 is legal for a and omega); ranks count (arguments checked by the caller)
template <typename T> void batched_sketch_range_step(rc_context *c, Mat<T> a, int64_t abs, Mat<T> omega, int64_t obs, int32_t count, Mat<T> y, int64_t ybs,
                                                     Mat<T> q, int64_t qbs, Mat<T> p, int64_t pbs, int64_t *ranks);
// the complex twin (kernels_batched_id_c.hip, k_batched_range_step_c), R = double (c64) or float (c32): interleaved-complex views, strides in complex
// elements; y = omega a with nothing conjugated, q q^H = I on its first rank rows, p = a q^H, or its elementwise conjugate when p_conj
template <typename R> void batched_sketch_range_step_c(rc_context *c, const rc_matrix &a, int64_t abs, const rc_matrix &omega, int64_t obs, int32_t count,
                                                       const rc_matrix &y, int64_t ybs, const rc_matrix &q, int64_t qbs, const rc_matrix &p, int64_t pbs,
                                                       int64_t *ranks, bool p_conj);
// the argument checks of rc_sketch_range_step_batched_* and rc_sketch_range_step_complex_batched_* (rc_batched_api.hip; complex: under the latter's
// name), one for every scalar type like those above; the caller returns when count == 0
void check_sketch_range_step_batched(const rc_matrix &a, const rc_matrix &omega, int32_t count, const rc_matrix &y, int64_t ybs, const rc_matrix &q,
                                     int64_t qbs, const rc_matrix &p, int64_t pbs, const int64_t *ranks, bool complex = false);
// the sketch alone, for blocks wide as well as tall (kernels_batched_id.hip, k_batched_sketch_product): y = omega a (l x n, n <= 65536) with the
// bits of batched_sketch_column_id's y, one (block, 64-column panel) per work unit; block i is a (m x n), omega (l x m) and y each moved by i times
// its batch stride (0 is legal for a and omega).  Real scalars only (arguments checked by the caller)
template <typename T> void batched_sketch_product(rc_context *c, Mat<T> a, int64_t abs, Mat<T> omega, int64_t obs, int32_t count, Mat<T> y, int64_t ybs);
// the argument checks of rc_sketch_product_batched_* (rc_batched_api.hip); the caller returns when count == 0
void check_sketch_product_batched(const rc_matrix &a, const rc_matrix &omega, int32_t count, const rc_matrix &y, int64_t ybs);
// the residual of such factors against the blocks they approximate, in one rank-aware launch (kernels_batched_residual.hip): block i is a (m x n), left
// (m x K), mid (K x K, p == nullptr: none), right (K x n) and e (m x n, p == nullptr: not written) each moved by i times its batch stride, s + i * s_stride
// its K real scales (nullptr: none), ranks count device values (nullptr: every rank is K); err and nrm (nullptr: not written) count values: ||a_i - left
// mid diag(s) right||_F at the block's rank and ||a_i||_F (arguments checked by the caller)
template <typename T> void batched_lowrank_residual(rc_context *c, Mat<T> a, int64_t abs, Mat<T> left, int64_t lbs, Mat<T> mid, int64_t mbs, const T *s,
                                                    int64_t s_stride, Mat<T> right, int64_t rbs, const int64_t *ranks, int32_t count, Mat<T> e, int64_t ebs,
                                                    T *err, T *nrm);
// the complex twin (kernels_batched_residual_c.hip), R = double (c64) or float (c32): interleaved-complex views, strides in complex elements, s, err
// and nrm real
template <typename R> void batched_lowrank_residual_c(rc_context *c, const rc_matrix &a, int64_t abs, const rc_matrix &left, int64_t lbs, const rc_matrix &mid,
                                                      int64_t mbs, const R *s, int64_t s_stride, const rc_matrix &right, int64_t rbs, const int64_t *ranks,
                                                      int32_t count, const rc_matrix &e, int64_t ebs, R *err, R *nrm);
// the argument checks of rc_lowrank_residual_batched_* (rc_batched_api.hip), one for every scalar type like those above; the caller returns when
// count == 0
void check_lowrank_residual_batched(const rc_matrix &a, const rc_matrix &left, const rc_matrix &mid, const rc_matrix &right, int32_t count, const rc_matrix &e,
                                    int64_t ebs, const void *err);
// (the batched kernels' dynamic-LDS cap, persistent grid and launch path: rc_batched_launch.hpp)

}  // namespace rc
