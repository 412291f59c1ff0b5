// y = H x for a block-sparse operator whose blocks are a batch of low-rank factors and, optionally, a batch of dense blocks of the same
// m x n shape (rc_block_operator_apply_*): the gather of x, the batched apply of kernels_batched_apply.hip and the scatter-add into y in
// one launch, for the reference's MatMat / ConjMatMat (src/types.rs:40-101) on the outputs of the batched compressors.
//
// The pattern is block-CSR on the device: group g owns rows group_row[g] .. + m - 1 of y and sums the entries group_ptr[g] ..
// group_ptr[g + 1] - 1 in that order; entry e is block entry_block[e] (low-rank below count, dense from count on) applied to rows
// entry_col[e] .. + n - 1 of x.
//
// MI355X mapping.  The same persistent grid of 256-thread workgroups as the apply (bid_grid); a work unit is (group, tile of NBT columns
// of x).  The unit walks its entries: per entry the x segment is staged in LDS (ba_load_tile) and the apply's three-stage chain runs
// through ba_product with the intermediates in LDS, but the last stage's store adds into an m x NBT accumulator in LDS instead of
// writing y.  After the last entry the unit writes its rows of y once (reading y_old once when accumulating).  No workgroup touches the
// rows of another group: no atomics, no global read-modify-write shared between workgroups, no workspace.  A dense entry is the last
// product alone, on the staged x segment (inner extent n).
//
// Bits.  A contribution is computed by the very code of the apply (batched_apply.hpp), whose summation order depends on the inner extent
// and on which stride of the operand is the smaller alone; the accumulator takes one rounded add per entry, in list order, from +0.
// Neither depends on NBT, the tile, the grid or the other groups.  The adds into the accumulator are kept out of reach of FMA contraction.
//
// conj (complex instances only): a template flag on ba_product's loads of left, mid, right and dense; s is real and x is untouched.
//
// Mixed storage (rc_block_operator_apply_mixed_*): left, mid and right are stored in S (f32 under E = f64, c32 under c64) and widened as
// ba_product loads them; dense, x, y, s, LDS and every sum stay in E, so the bits are those of the E call on promoted factors.
#include "batched_apply.hpp"

namespace rc {

namespace {

constexpr int BOP_BAD_INDEX = 64;  // health bit: a block id, entry_col or group_row out of range

template <typename E, typename S = E>
struct BopArgs {
    BaView<const S> left, mid, right;  // stored in S
    BaView<const E> dense;             // dense.p == nullptr: no dense blocks
    const typename El<E>::real *s;
    int64_t s_stride;
    const int64_t *ranks;
    const int64_t *group_ptr, *group_row, *entry_block, *entry_col;
    const E *x;
    E *y;
    int64_t xrs, xcs, yrs, ycs;
    int64_t xrows, yrows;  // N, M
    int *health;
    int count, dense_count, groups, m, n, k, ncols, accumulate;
};

// dynamic LDS: Bs: NBT x (n|1), W0: NBT x (k|1) [W1: NBT x (k|1), with mid only], Acc: NBT x (m|1); k = 0 without a low-rank batch
template <typename E>
size_t bop_lds_bytes(int m, int n, int k, int nbt, bool has_mid) {
    return ((size_t)nbt * (size_t)(n | 1) + (size_t)(has_mid ? 2 : 1) * nbt * (size_t)(k | 1) + (size_t)nbt * (size_t)(m | 1)) * sizeof(E);
}

// a + b rounded once: written out under contract(off) (the pragma is lexical) so that it is never fused with the product that made b
template <typename R>
__device__ __forceinline__ R bop_add(R a, R b) {
#pragma clang fp contract(off)
    return a + b;
}
template <typename R>
__device__ __forceinline__ cplx<R> bop_add(cplx<R> a, cplx<R> b) {
#pragma clang fp contract(off)
    return {a.re + b.re, a.im + b.im};
}

template <typename E, int NBT, bool CJ, typename S = E>
__global__ __launch_bounds__(BA_THREADS) void k_block_operator(BopArgs<E, S> a) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const int m = a.m, n = a.n, k = a.k, ncols = a.ncols;
    const int ldn = n | 1, ldk = k | 1, ldm = m | 1;
    E *Bs = reinterpret_cast<E *>(smem_raw);
    E *W0 = Bs + (size_t)NBT * ldn;
    E *W1 = W0 + (size_t)NBT * ldk;
    E *Acc = W0 + (size_t)(a.mid.p ? 2 : 1) * NBT * ldk;
    const int tid = threadIdx.x;
    const int ntiles = (ncols + NBT - 1) / NBT;
    const int64_t nunits = (int64_t)a.groups * ntiles;
    const int64_t nblocks = (int64_t)a.count + a.dense_count;
    auto to_acc = [&](int row, int c, E v) { Acc[c * ldm + row] = bop_add(Acc[c * ldm + row], v); };

    for (int64_t unit = blockIdx.x; unit < nunits; unit += gridDim.x) {
        const int64_t g = unit / ntiles;
        const int c0 = (int)(unit % ntiles) * NBT;
        const int nb = ncols - c0 < NBT ? ncols - c0 : NBT;
        const int64_t row0 = a.group_row[g], e0 = a.group_ptr[g], e1 = a.group_ptr[g + 1];
        if (row0 < 0 || row0 > a.yrows - m || e0 < 0) {  // uniform over the workgroup: the group writes nothing
            if (tid == 0) atomicOr(a.health, BOP_BAD_INDEX);
            continue;
        }
        for (int idx = tid; idx < NBT * ldm; idx += BA_THREADS) Acc[idx] = El<E>::zero();
        __syncthreads();
        for (int64_t e = e0; e < e1; ++e) {
            const int64_t blk = a.entry_block[e], col = a.entry_col[e];
            if (blk < 0 || blk >= nblocks || col < 0 || col > a.xrows - n) {  // uniform: the entry is skipped
                if (tid == 0) atomicOr(a.health, BOP_BAD_INDEX);
                continue;
            }
            const bool lowrank = blk < a.count;
            int r = 0;
            if (lowrank) {
                r = k;
                if (a.ranks) {
                    const int64_t rv = a.ranks[blk];
                    r = rv < 0 ? 0 : rv > k ? k : (int)rv;
                }
                r = __builtin_amdgcn_readfirstlane(r);  // one value per entry, uniform by construction
                if (r == 0) continue;                   // contributes nothing; LDS is not touched
            }
            ba_load_tile<E, NBT>(Bs, ldn, a.x + col * a.xrs, a.xrs, a.xcs, n, c0, nb, tid);
            __syncthreads();
            if (!lowrank) {
                const int64_t d = blk - a.count;
                ba_product<E, NBT, CJ>(a.dense.p + d * a.dense.bs, a.dense.rs, a.dense.cs, m, n, Bs, ldn, to_acc, tid);
                __syncthreads();  // Bs is rewritten by the next entry, Acc by other threads
                continue;
            }
            // ---- the apply's chain (k_batched_apply), the last store adding into Acc ----------------------------------------------------
            ba_product<E, NBT, CJ, S>(a.right.p + blk * a.right.bs, a.right.rs, a.right.cs, r, n, Bs, ldn, [&](int row, int c, E v) { W0[c * ldk + row] = v; },
                                   tid);
            __syncthreads();
            if (a.s) {
                const typename El<E>::real *sb = a.s + blk * a.s_stride;
                for (int idx = tid; idx < r * NBT; idx += BA_THREADS) {
                    const int j = idx % r, c = idx / r;
                    W0[c * ldk + j] = El<E>::scale(sb[j], W0[c * ldk + j]);
                }
                __syncthreads();
            }
            const E *Wc = W0;
            if (a.mid.p) {
                ba_product<E, NBT, CJ, S>(a.mid.p + blk * a.mid.bs, a.mid.rs, a.mid.cs, r, r, W0, ldk, [&](int row, int c, E v) { W1[c * ldk + row] = v; }, tid);
                __syncthreads();
                Wc = W1;
            }
            ba_product<E, NBT, CJ, S>(a.left.p + blk * a.left.bs, a.left.rs, a.left.cs, m, r, Wc, ldk, to_acc, tid);
            __syncthreads();  // Bs, W0 and W1 are rewritten by the next entry, Acc by other threads
        }
        // ---- y[row0 : row0 + m, c0 : c0 + nb] = [y_old +] Acc, lanes along the fast index of y ------------------------------------------
        E *Y = a.y + row0 * a.yrs + (int64_t)c0 * a.ycs;
        const int total = m * nb;
        for (int idx = tid; idx < total; idx += BA_THREADS) {
            const int row = a.ycs <= a.yrs ? idx / nb : idx % m, c = a.ycs <= a.yrs ? idx % nb : idx / m;
            E *yp = Y + (int64_t)row * a.yrs + (int64_t)c * a.ycs;
            const E v = Acc[c * ldm + row];
            *yp = a.accumulate ? bop_add(*yp, v) : v;
        }
        __syncthreads();  // Acc is cleared by the next unit
    }
}

// the plan (at: the tile width): the apply's rule (the smallest of 1, 4, 8, 16 that covers the columns, at most the scalar type's NB),
// stepped down while the accumulator does not fit beside the apply's buffers (m = n = 512, k = 128 with mid: 16 columns of f64 need
// 164 352 B of the 162 816); no workspace.  The bits of an output element do not depend on it.
template <typename E>
BatchedPlan<int> bop_plan(int m, int n, int k, int ncols, bool has_mid) {
    constexpr int NB = ba_nb<E>();
    int nbt = ncols <= 1 ? 1 : ncols <= 4 ? 4 : ncols <= 8 ? 8 : 16;
    if (nbt > NB) nbt = NB;
    while (nbt > 1 && bop_lds_bytes<E>(m, n, k, nbt, has_mid) > BID_MAX_LDS) nbt = nbt == 4 ? 1 : nbt / 2;
    return {nbt, bop_lds_bytes<E>(m, n, k, nbt, has_mid), 0};
}

template <typename E, int NBT, bool CJ, typename S>
void bop_launch_nbt(rc_context *c, const BopArgs<E, S> &a, const char *tag, bool conj, size_t lds) {
    const int64_t ntiles = (a.ncols + NBT - 1) / NBT;
    const auto lch = batched_prepare(c, k_block_operator<E, NBT, CJ, S>, "block_operator_apply", lds, 0, (int64_t)a.groups * ntiles);
    // entries: the number of entries is group_ptr[groups], which only the device knows
    ProfScope ps(c, "op:batched_operator_apply%s %dx%d k=%d count=%d grid=%lld slots=%lld plan=nb:%d,tiles:%lld,cols:%d,entries:dev,lr:%d,dense:%d%s%s%s%s", tag,
                 a.m, a.n, a.k, a.groups, (long long)lch.grid, (long long)lch.slots, NBT, (long long)ntiles, a.ncols, a.count, a.dense_count,
                 a.mid.p ? ",mid" : "", a.s ? ",s" : "", a.accumulate ? ",acc" : "", conj ? ",conj" : "");
    lch.launch(a);
}

template <typename E, bool CJ, typename S>
void bop_launch(rc_context *c, const BopArgs<E, S> &a, const char *tag, bool conj) {
    const auto plan = bop_plan<E>(a.m, a.n, a.k, a.ncols, a.mid.p != nullptr);
    if (plan.at == 1) return bop_launch_nbt<E, 1, CJ, S>(c, a, tag, conj, plan.lds);
    if (plan.at == 4) return bop_launch_nbt<E, 4, CJ, S>(c, a, tag, conj, plan.lds);
    if constexpr (ba_nb<E>() >= 16) {
        if (plan.at == 16) return bop_launch_nbt<E, 16, CJ, S>(c, a, tag, conj, plan.lds);
    }
    bop_launch_nbt<E, 8, CJ, S>(c, a, tag, conj, plan.lds);
}

template <typename E, typename P>
BaView<E> bop_view(P *p, int64_t rs, int64_t cs, int64_t bs) { return BaView<E>{reinterpret_cast<E *>(p), rs, cs, bs}; }

template <typename E, typename S>
void bop_pattern(rc_context *c, BopArgs<E, S> &a, const BlockPattern &pat, BlockShape shape, int32_t count, int32_t dense_count, bool accumulate) {
    a.group_ptr = pat.group_ptr; a.group_row = pat.group_row; a.entry_block = pat.entry_block; a.entry_col = pat.entry_col; a.groups = pat.groups;
    a.count = count; a.dense_count = a.dense.p ? dense_count : 0;
    a.m = shape.m; a.n = shape.n; a.k = shape.k;
    a.accumulate = accumulate ? 1 : 0;
    a.health = c->health_word();
}

}  // namespace

template <typename E>
void block_operator_apply(rc_context *c, Mat<E> left, int64_t lbs, Mat<E> mid, int64_t mbs, const real_t<E> *s, int64_t s_stride, Mat<E> right, int64_t rbs,
                          const int64_t *ranks, int32_t count, Mat<E> dense, int64_t dbs, int32_t dense_count, const BlockPattern &pat, BlockShape shape,
                          Mat<E> x, Mat<E> y, bool accumulate, bool conj) {
    BopArgs<E> a;
    a.left = bop_view<const E>(left.p, left.rs, left.cs, lbs);
    a.mid = bop_view<const E>(count > 0 ? mid.p : nullptr, mid.rs, mid.cs, mbs);
    a.right = bop_view<const E>(right.p, right.rs, right.cs, rbs);
    a.dense = bop_view<const E>(dense.p, dense.rs, dense.cs, dbs);
    a.s = count > 0 ? s : nullptr; a.s_stride = s_stride; a.ranks = ranks;
    a.x = x.p; a.xrs = x.rs; a.xcs = x.cs; a.xrows = x.rows;
    a.y = y.p; a.yrs = y.rs; a.ycs = y.cs; a.yrows = y.rows;
    a.ncols = (int)y.cols;
    bop_pattern(c, a, pat, shape, count, dense_count, accumulate);
    // conjugation is the identity on real elements: they have no conjugating instance and ignore the flag
    if constexpr (std::is_same<E, real_t<E>>::value) {
        bop_launch<E, false, E>(c, a, "", false);
    } else {
        if (conj) bop_launch<E, true, E>(c, a, "<complex>", true);
        else bop_launch<E, false, E>(c, a, "<complex>", false);
    }
}

// the mixed calls: factor views of S (strides in elements of S), dense, x and y of E, s double
template <typename E, typename S>
static BopArgs<E, S> bop_mixed_args(rc_context *c, const rc_matrix &left, int64_t lbs, const rc_matrix &mid, int64_t mbs, const double *s, int64_t s_stride,
                                    const rc_matrix &right, int64_t rbs, const int64_t *ranks, int32_t count, const rc_matrix &dense, int64_t dbs,
                                    int32_t dense_count, const BlockPattern &pat, BlockShape shape, const rc_matrix &x, const rc_matrix &y, bool accumulate) {
    BopArgs<E, S> a;
    a.left = bop_view<const S>(left.data, left.row_stride, left.col_stride, lbs);
    a.mid = bop_view<const S>(count > 0 ? mid.data : nullptr, mid.row_stride, mid.col_stride, mbs);
    a.right = bop_view<const S>(right.data, right.row_stride, right.col_stride, rbs);
    a.dense = bop_view<const E>(dense.data, dense.row_stride, dense.col_stride, dbs);
    a.s = count > 0 ? s : nullptr; a.s_stride = s_stride; a.ranks = ranks;
    a.x = static_cast<const E *>(x.data); a.xrs = x.row_stride; a.xcs = x.col_stride; a.xrows = x.rows;
    a.y = static_cast<E *>(y.data); a.yrs = y.row_stride; a.ycs = y.col_stride; a.yrows = y.rows;
    a.ncols = (int)y.cols;
    bop_pattern(c, a, pat, shape, count, dense_count, accumulate);
    return a;
}

void block_operator_apply_mixed(rc_context *c, bool complex_data, const rc_matrix &left, int64_t lbs, const rc_matrix &mid, int64_t mbs, const double *s,
                                int64_t s_stride, const rc_matrix &right, int64_t rbs, const int64_t *ranks, int32_t count, const rc_matrix &dense, int64_t dbs,
                                int32_t dense_count, const BlockPattern &pat, BlockShape shape, const rc_matrix &x, const rc_matrix &y, bool accumulate, bool conj) {
    if (!complex_data) {
        const auto a = bop_mixed_args<double, float>(c, left, lbs, mid, mbs, s, s_stride, right, rbs, ranks, count, dense, dbs, dense_count, pat, shape, x, y,
                                                     accumulate);
        return bop_launch<double, false, float>(c, a, "<mixed>", false);
    }
    using E = cplx<double>;
    using S = cplx<float>;
    const auto a = bop_mixed_args<E, S>(c, left, lbs, mid, mbs, s, s_stride, right, rbs, ranks, count, dense, dbs, dense_count, pat, shape, x, y, accumulate);
    if (conj) bop_launch<E, true, S>(c, a, "<complex,mixed>", true);
    else bop_launch<E, false, S>(c, a, "<complex,mixed>", false);
}

#define RC_INSTANTIATE_BLOCK_OPERATOR(E)                                                                                                    \
    template void block_operator_apply<E>(rc_context *, Mat<E>, int64_t, Mat<E>, int64_t, const real_t<E> *, int64_t, Mat<E>, int64_t, const int64_t *, \
                                          int32_t, Mat<E>, int64_t, int32_t, const BlockPattern &, BlockShape, Mat<E>, Mat<E>, bool, bool);
RC_INSTANTIATE_BLOCK_OPERATOR(double)
RC_INSTANTIATE_BLOCK_OPERATOR(float)
RC_INSTANTIATE_BLOCK_OPERATOR(cplx<double>)
RC_INSTANTIATE_BLOCK_OPERATOR(cplx<float>)

}  // namespace rc
