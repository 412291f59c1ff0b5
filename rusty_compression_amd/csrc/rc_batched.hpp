// The batched family (many small or tall same-shaped blocks in one launch): its kernel launchers (kernels_batched_*.hip,
// kernels_block_operator.hip, kernels_convert.hip) and the argument checks of its entry points (rc_batched_api.hip).  rc_common.hpp ends by
// including this header, so every translation unit sees it.
//
// Every launcher is declared once, over the element type E of its views: double, float, cplx<double> or cplx<float> (interleaved complex,
// strides in complex elements; rc_cplx.hpp).  Scales, singular values and norms are real_t<E>.  Each translation unit defines and
// instantiates the launchers of its own element types: kernels_batched_id.hip and kernels_batched_residual.hip the real two,
// kernels_batched_id_c.hip and kernels_batched_residual_c.hip the complex two, kernels_batched_apply.hip and kernels_block_operator.hip all four.
#pragma once

#include "rc_common.hpp"

namespace rc {

// the complex element (defined in rc_cplx.hpp) and the real type of an element
template <typename R> struct cplx;
template <typename E> struct real_of { using type = E; };
template <typename R> struct real_of<cplx<R>> { using type = R; };
template <typename E> using real_t = typename real_of<E>::type;

// rank-revealing column IDs of `count` same-shaped small matrices in one launch (kernels_batched_id*.hip): matrix i is a, cm, z moved by
// i * abs, i * cbs, i * zbs elements; col_ind count x n, ranks count (arguments checked by the caller)
template <typename E> void batched_column_id(rc_context *c, Mat<E> a, int64_t abs, int32_t count, int64_t k, double tol, Mat<E> cm, int64_t cbs, Mat<E> z,
                                             int64_t zbs, int64_t *col_ind, int64_t *ranks);
// the two-sided ID of the same batch (kernels_batched_id*.hip): matrix i is a, cm (m x k), x (k x k), z (k x n) moved by i * abs, i * cbs,
// i * xbs, i * zbs elements; row_ind count x m, col_ind count x n, ranks count (arguments checked by the caller)
template <typename E> void batched_two_sided_id(rc_context *c, Mat<E> a, int64_t abs, int32_t count, int64_t k, double tol, Mat<E> cm, int64_t cbs, Mat<E> x,
                                                int64_t xbs, Mat<E> z, int64_t zbs, int64_t *row_ind, int64_t *col_ind, int64_t *ranks);
// truncated SVDs of the same kind of batch (kernels_batched_id*.hip): matrix i is a, u (m x k), vt = V^H (k x n) moved by i * abs, i * ubs,
// i * vbs elements; s count x min(m, n), ranks count (arguments checked by the caller)
template <typename E> void batched_svd(rc_context *c, Mat<E> a, int64_t abs, int32_t count, int64_t k, double tol, Mat<E> u, int64_t ubs, real_t<E> *s,
                                       Mat<E> vt, int64_t vbs, int64_t *ranks);
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
// none), ranks count device values (nullptr: every rank is k); nothing is conjugated (arguments checked by the caller)
template <typename E> void batched_lowrank_apply(rc_context *c, Mat<E> left, int64_t lbs, Mat<E> mid, int64_t mbs, const real_t<E> *s, int64_t s_stride,
                                                 Mat<E> right, int64_t rbs, const int64_t *ranks, int32_t count, Mat<E> b, int64_t bbs, Mat<E> y, int64_t ybs);
// the argument checks of rc_lowrank_apply_batched_* (rc_batched_api.hip), one for every scalar type like the three above; the caller returns when
// count == 0
void check_lowrank_apply_batched(const rc_matrix &left, const rc_matrix &mid, const rc_matrix &right, int32_t count, const rc_matrix &b, const rc_matrix &y,
                                 int64_t ybs);
// y = H x for the block-sparse operator whose blocks are the factors of such a batch and a batch of dense m x n blocks, placed by a block-CSR
// pattern on the device (kernels_block_operator.hip, rc_block_operator_apply_*): the low-rank operands as in batched_lowrank_apply, block ids
// count .. count + dense_count - 1 are dense (p == nullptr: none); shape holds m, n and k (0 without a low-rank batch) as the check returns them;
// complex blocks are conjugated on load when conj is set, which real elements ignore (arguments checked by the caller)
struct BlockPattern {
    const int64_t *group_ptr, *group_row, *entry_block, *entry_col;
    int32_t groups;
};
struct BlockShape {
    int m, n, k;
};
template <typename E> void block_operator_apply(rc_context *c, Mat<E> left, int64_t lbs, Mat<E> mid, int64_t mbs, const real_t<E> *s, int64_t s_stride,
                                                Mat<E> right, int64_t rbs, const int64_t *ranks, int32_t count, Mat<E> dense, int64_t dbs, int32_t dense_count,
                                                const BlockPattern &pat, BlockShape shape, Mat<E> x, Mat<E> y, bool accumulate, bool conj);
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
// recompress the factor pairs of such a batch to truncated SVDs without forming the blocks (kernels_batched_id*.hip): block i is left (m x K), mid (K x K,
// p == nullptr: none), right (K x n), u (m x min(k, K)) and vt = V^H (min(k, K) x n) each moved by i times its batch stride, s + i * s_stride its K real
// scales (nullptr: none), in_ranks count device values (nullptr: every inner rank is K); s_out count x K, ranks count (arguments checked by the caller)
template <typename E> void batched_lowrank_recompress(rc_context *c, Mat<E> left, int64_t lbs, Mat<E> mid, int64_t mbs, const real_t<E> *s, int64_t s_stride,
                                                      Mat<E> right, int64_t rbs, const int64_t *in_ranks, int32_t count, int64_t k, double tol, Mat<E> u,
                                                      int64_t ubs, real_t<E> *s_out, Mat<E> vt, int64_t vbs, int64_t *ranks);
// the same with a tall left factor (m <= 65536): flat Householder TSQR of left in stages of 512 rows, stored in the workgroup's slot; and its plan
// as numbers: stages at inner width K, bytes of one slot, the grid its 2 GiB workspace bound leaves of `resident` workgroups
template <typename E> void batched_lowrank_recompress_tall(rc_context *c, Mat<E> left, int64_t lbs, Mat<E> mid, int64_t mbs, const real_t<E> *s,
                                                           int64_t s_stride, Mat<E> right, int64_t rbs, const int64_t *in_ranks, int32_t count, int64_t k,
                                                           double tol, Mat<E> u, int64_t ubs, real_t<E> *s_out, Mat<E> vt, int64_t vbs, int64_t *ranks);
template <typename E> void batched_lowrank_recompress_tall_plan(int64_t m, int64_t n, int64_t K, int64_t resident, int64_t *stages, int64_t *slot_bytes,
                                                                int64_t *grid);
// the same with both factors tall (m, n <= 65536): right^T by the same stages behind left's in the slot; n <= 512 is the tall call bit for bit.
// Its plan as numbers: the stages of both factors at inner width K, bytes of one slot, the grid
template <typename E> void batched_lowrank_recompress_large(rc_context *c, Mat<E> left, int64_t lbs, Mat<E> mid, int64_t mbs, const real_t<E> *s,
                                                            int64_t s_stride, Mat<E> right, int64_t rbs, const int64_t *in_ranks, int32_t count, int64_t k,
                                                            double tol, Mat<E> u, int64_t ubs, real_t<E> *s_out, Mat<E> vt, int64_t vbs, int64_t *ranks);
template <typename E> void batched_lowrank_recompress_large_plan(int64_t m, int64_t n, int64_t K, int64_t resident, int64_t *stages_left,
                                                                 int64_t *stages_right, int64_t *slot_bytes, int64_t *grid);
// the argument checks of rc_lowrank_recompress_batched_* and rc_lowrank_recompress_complex_batched_* (rc_batched_api.hip), one for every scalar type
// like those above; the caller returns when count == 0.  tall: the bound m <= 65536 under rc_lowrank_recompress_tall_batched_*'s name (RC_TALL) or
// rc_lowrank_recompress_tall_complex_batched_*'s (RC_TALL_COMPLEX); RC_LARGE: m, n <= 65536 under rc_lowrank_recompress_large_batched_*'s, and
// RC_LARGE_COMPLEX the same under rc_lowrank_recompress_complex_large_batched_*'s
enum { RC_NOT_TALL = 0, RC_TALL = 1, RC_TALL_COMPLEX = 2, RC_LARGE = 3, RC_LARGE_COMPLEX = 4 };
void check_lowrank_recompress_batched(const rc_matrix &left, const rc_matrix &mid, const rc_matrix &right, int32_t count, int64_t k, double tol,
                                      const rc_matrix &u, int64_t ubs, const void *s_out, const rc_matrix &vt, int64_t vbs, const int64_t *ranks,
                                      int tall = RC_NOT_TALL);
// the column ID of the sketch omega a of every block of a batch (kernels_batched_id*.hip): block i is a (m x n), omega (l x m, l <= 128), y (l x n,
// p == nullptr: not written), cm (m x kk) and z (kk x n) each moved by i times its batch stride (0 is legal for a and omega), kk = min(k, l, n) already
// clamped; col_ind count x n, ranks count; nothing is conjugated (arguments checked by the caller)
template <typename E> void batched_sketch_column_id(rc_context *c, Mat<E> a, int64_t abs, Mat<E> omega, int64_t obs, int32_t count, int64_t kk, double tol,
                                                    Mat<E> y, int64_t ybs, Mat<E> cm, int64_t cbs, Mat<E> z, int64_t zbs, int64_t *col_ind, int64_t *ranks);
// the argument checks of rc_sketch_column_id_rank_batched_* and rc_sketch_column_id_rank_complex_batched_* (rc_batched_api.hip), one for every scalar
// type like those above.  Return kk = min(k, l, n); the caller returns when count == 0.
int64_t check_sketch_column_id_rank_batched(const rc_matrix &a, const rc_matrix &omega, int32_t count, int64_t k, double tol, const rc_matrix &y, int64_t ybs,
                                            const rc_matrix &cm, int64_t cbs, const rc_matrix &z, int64_t zbs, const int64_t *col_ind, const int64_t *ranks);
// one range step of every block of a batch (kernels_batched_id*.hip, k_batched_range_step / _c): the sketch y = omega a (l x n, p == nullptr: not
// written, nothing conjugated), an orthonormal basis q (l x n, q q^H = I on its first rank rows, the others zero) of its rows and the projection
// p = a q^H (m x l), or its elementwise conjugate when p_conj, which real elements ignore; each moved by i times its batch stride (0 is legal for a
// and omega); ranks count (arguments checked by the caller)
template <typename E> void batched_sketch_range_step(rc_context *c, Mat<E> a, int64_t abs, Mat<E> omega, int64_t obs, int32_t count, Mat<E> y, int64_t ybs,
                                                     Mat<E> q, int64_t qbs, Mat<E> p, int64_t pbs, int64_t *ranks, bool p_conj);
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
// the residual of such factors against the blocks they approximate, in one rank-aware launch (kernels_batched_residual.hip, kernels_batched_residual_c.hip):
// block i is a (m x n), left (m x K), mid (K x K, p == nullptr: none), right (K x n) and e (m x n, p == nullptr: not written) each moved by i times its
// batch stride, s + i * s_stride its K real scales (nullptr: none), ranks count device values (nullptr: every rank is K); err and nrm (nullptr: not
// written) count real values: ||a_i - left mid diag(s) right||_F at the block's rank and ||a_i||_F (arguments checked by the caller)
template <typename E> void batched_lowrank_residual(rc_context *c, Mat<E> a, int64_t abs, Mat<E> left, int64_t lbs, Mat<E> mid, int64_t mbs, const real_t<E> *s,
                                                    int64_t s_stride, Mat<E> right, int64_t rbs, const int64_t *ranks, int32_t count, Mat<E> e, int64_t ebs,
                                                    real_t<E> *err, real_t<E> *nrm);
// (one definition for the real elements; the complex ones, whose Args and image element differ, are explicit specialisations)
template <> void batched_lowrank_residual<cplx<double>>(rc_context *, Mat<cplx<double>>, int64_t, Mat<cplx<double>>, int64_t, Mat<cplx<double>>, int64_t,
                                                        const double *, int64_t, Mat<cplx<double>>, int64_t, const int64_t *, int32_t, Mat<cplx<double>>,
                                                        int64_t, double *, double *);
template <> void batched_lowrank_residual<cplx<float>>(rc_context *, Mat<cplx<float>>, int64_t, Mat<cplx<float>>, int64_t, Mat<cplx<float>>, int64_t,
                                                       const float *, int64_t, Mat<cplx<float>>, int64_t, const int64_t *, int32_t, Mat<cplx<float>>, int64_t,
                                                       float *, float *);
// the argument checks of rc_lowrank_residual_batched_* (rc_batched_api.hip), one for every scalar type like those above; the caller returns when
// count == 0
void check_lowrank_residual_batched(const rc_matrix &a, const rc_matrix &left, const rc_matrix &mid, const rc_matrix &right, int32_t count, const rc_matrix &e,
                                    int64_t ebs, const void *err);
// (the batched kernels' dynamic-LDS cap, persistent grid and launch path: rc_batched_launch.hpp)

}  // namespace rc
