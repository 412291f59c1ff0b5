// Apply or rebuild a batch of low-rank factorizations in one rank-aware launch (rc_lowrank_apply_batched_*).
//
// Per block i, with r = ranks[i] clamped to [0, k] (k when there are no ranks): W = right_i[:r, :] b_i (or right_i[:r, :] itself when
// reconstructing), W = diag(s_i[:r]) W, W = mid_i[:r, :r] W, y_i = left_i[:, :r] W -- the reference's Apply::dot and to_mat of the
// column ID (src/col_interp_decomp.rs:63-65, :134-154), the two-sided ID (src/two_sided_interp_decomp.rs:62-65, :159-170) and the
// SVD (src/svd.rs:42-55) on the factors the batched calls of kernels_batched_id.hip return.  Nothing at index >= r is read.
//
// MI355X mapping.  The path is bound by HBM: with one right-hand side it does two flops per factor element read.  A persistent grid
// of 256-thread workgroups (bid_grid) walks the work units, unit = blockIdx.x, blockIdx.x + G, ...; one unit is (block, tile of NBT
// columns of the right-hand side, or of `right` when reconstructing).  The staged b tile and the r x NBT intermediate W live in LDS
// for the whole chain, column by column (In[c * ld + j], odd ld: the lanes of a wave read consecutive j without bank conflicts, and
// a thread that walks j reads one broadcast address); W never goes to global memory and there is no workspace.
//
// All three products are the same operation, Out (rows x NBT) = M[:, :red] In with M read from global memory once and In in LDS
// (ba_product), run with the lanes along whichever index of the view M has the smaller stride, as bid_load does:
//   * red fast (the C-order factors the batched calls return: left m x k, mid k x k, right k x n): G = min(64, 2^ceil(log2 red))
//     lanes share one row and 64 / G rows share a wave, so a block of tolerance rank 5 still fills the wave; lane l accumulates
//     j = l, l + G, ... in ascending order and the group is summed by a butterfly in which every step also halves the columns a lane
//     keeps (NBT + log2 G shuffles per row instead of NBT log2 G);
//   * rows fast (transposed views, column-major factors): one thread per row, j ascending.
// Either way the summation order of an output element is a function of (red, which stride of M is the smaller) alone -- not of the
// column, the tile, NBT, the grid, count, the batch strides or the neighbours -- which is what the bit-independence clause of the
// contract rests on.  Plain FMAs: with one right-hand side the call runs at the memory bound; with 16 and when reconstructing the
// red-fast mapping is bound by its cross-lane sums, about one shuffle per FMA (tools/batched_apply_bench.py).
//
// The complex scalars run the same kernel on interleaved (re, im) pairs; nothing is conjugated.
//
// Mixed storage (rc_lowrank_apply_mixed_batched_*): S, the type left, mid and right are stored in, is f32 under E = f64 and c32 under c64.
// An element is widened exactly as it is loaded (ba_widen); LDS, b, y, s, the accumulators, the mapping and the summation trees are those
// of E, so the result has the bits of the E call on promoted factors while the launch moves half the factor bytes.
#include "batched_apply.hpp"

namespace rc {

namespace {

template <typename E, int NBT, typename S = E>
__global__ __launch_bounds__(BA_THREADS) void k_batched_apply(BaArgs<E, S> a) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const int m = a.m, n = a.n, k = a.k, ncols = a.ncols;
    const int ldn = n | 1, ldk = k | 1;
    E *Bs = reinterpret_cast<E *>(smem_raw);
    E *W0 = Bs + (a.b.p ? (size_t)NBT * ldn : 0);
    E *W1 = W0 + (size_t)NBT * ldk;
    const int tid = threadIdx.x;
    const int ntiles = (ncols + NBT - 1) / NBT;
    const int64_t nunits = (int64_t)a.count * ntiles;

    for (int64_t unit = blockIdx.x; unit < nunits; unit += gridDim.x) {
        const int64_t blk = unit / ntiles;
        const int c0 = (int)(unit % ntiles) * NBT;
        const int nb = ncols - c0 < NBT ? ncols - c0 : NBT;
        int r = k;
        if (a.ranks) {
            const int64_t rv = a.ranks[blk];
            r = rv < 0 ? 0 : rv > k ? k : (int)rv;
        }
        r = __builtin_amdgcn_readfirstlane(r);  // one value per unit, uniform by construction: keeps the loop bounds in scalar registers
        E *Y = a.y.p + blk * a.y.bs;
        auto to_y = [&](int row, int c, E v) {
            if (c < nb) Y[(int64_t)row * a.y.rs + (int64_t)(c0 + c) * a.y.cs] = v;
        };
        if (r == 0) {  // uniform over the workgroup; LDS is not touched
            for (int idx = tid; idx < m * nb; idx += BA_THREADS) to_y(idx / nb, idx % nb, El<E>::zero());
            continue;
        }
        // ---- stage 1: W0 = right[:r, :] b, or the tile of right[:r, :] itself -------------------------------------------------------
        const S *Rt = a.right.p + blk * a.right.bs;
        if (a.b.p) {
            ba_load_tile<E, NBT>(Bs, ldn, a.b.p + blk * a.b.bs, a.b.rs, a.b.cs, n, c0, nb, tid);
            __syncthreads();
            ba_product<E, NBT, false, S>(Rt, a.right.rs, a.right.cs, r, n, Bs, ldn, [&](int row, int c, E v) { W0[c * ldk + row] = v; }, tid);
        } else {
            ba_load_tile<E, NBT, S>(W0, ldk, Rt, a.right.rs, a.right.cs, r, c0, nb, tid);
        }
        __syncthreads();
        // ---- W0 = diag(s[:r]) W0 --------------------------------------------------------------------------------------------------------
        if (a.s) {
            const typename El<E>::real *sb = a.s + blk * a.s_stride;
            for (int idx = tid; idx < r * NBT; idx += BA_THREADS) {
                const int j = idx % r, c = idx / r;
                W0[c * ldk + j] = El<E>::scale(sb[j], W0[c * ldk + j]);
            }
            __syncthreads();
        }
        // ---- W1 = mid[:r, :r] W0 --------------------------------------------------------------------------------------------------------
        const E *Wc = W0;
        if (a.mid.p) {
            ba_product<E, NBT, false, S>(a.mid.p + blk * a.mid.bs, a.mid.rs, a.mid.cs, r, r, W0, ldk, [&](int row, int c, E v) { W1[c * ldk + row] = v; }, tid);
            __syncthreads();
            Wc = W1;
        }
        // ---- y = left[:, :r] W ----------------------------------------------------------------------------------------------------------
        ba_product<E, NBT, false, S>(a.left.p + blk * a.left.bs, a.left.rs, a.left.cs, m, r, Wc, ldk, to_y, tid);
        __syncthreads();  // Bs, W0 and W1 are rewritten by the next unit
    }
}

// the plan (at: the tile width): the smallest of 1, 4, 8, 16 that covers the columns, at most the scalar type's NB; no workspace.  The
// bits of an output element do not depend on it (see the head of this file).
template <typename E>
BatchedPlan<int> ba_plan(int n, int k, int ncols, bool has_b, bool has_mid) {
    constexpr int NB = ba_nb<E>();
    const int nbt = ncols <= 1 ? 1 : ncols <= 4 ? 4 : (NB >= 16 && ncols <= 8) ? 8 : NB;
    return {nbt, ba_lds_bytes<E>(n, k, nbt, has_b, has_mid), 0};
}

template <typename E, int NBT, typename S>
void ba_launch_nbt(rc_context *c, const BaArgs<E, S> &a, const char *tag, size_t lds) {
    const int64_t ntiles = (a.ncols + NBT - 1) / NBT;
    const auto lch = batched_prepare(c, k_batched_apply<E, NBT, S>, "lowrank_apply_batched", lds, 0, (int64_t)a.count * ntiles);
    ProfScope ps(c, "op:batched_apply%s %dx%d k=%d count=%d grid=%lld slots=%lld plan=nb:%d,tiles:%lld,cols:%d,%s%s%s", tag, a.m, a.n, a.k, a.count,
                 (long long)lch.grid, (long long)lch.slots, NBT, (long long)ntiles, a.ncols, a.b.p ? "apply" : "to_mat", a.mid.p ? ",mid" : "", a.s ? ",s" : "");
    lch.launch(a);
}

template <typename E, typename S>
void ba_launch(rc_context *c, const BaArgs<E, S> &a, const char *tag) {
    if (a.count <= 0) return;
    const auto plan = ba_plan<E>(a.n, a.k, a.ncols, a.b.p != nullptr, a.mid.p != nullptr);
    if (plan.at == 1) return ba_launch_nbt<E, 1, S>(c, a, tag, plan.lds);
    if (plan.at == 4) return ba_launch_nbt<E, 4, S>(c, a, tag, plan.lds);
    if constexpr (ba_nb<E>() >= 16) {
        if (plan.at == 8) return ba_launch_nbt<E, 8, S>(c, a, tag, plan.lds);
    }
    ba_launch_nbt<E, ba_nb<E>(), S>(c, a, tag, plan.lds);
}

template <typename E, typename P>
BaView<E> ba_view(P *p, int64_t rs, int64_t cs, int64_t bs) { return BaView<E>{reinterpret_cast<E *>(p), rs, cs, bs}; }

}  // namespace

template <typename E>
void batched_lowrank_apply(rc_context *c, Mat<E> left, int64_t lbs, Mat<E> mid, int64_t mbs, const real_t<E> *s, int64_t s_stride, Mat<E> right, int64_t rbs,
                           const int64_t *ranks, int32_t count, Mat<E> b, int64_t bbs, Mat<E> y, int64_t ybs) {
    BaArgs<E> a;
    a.left = ba_view<const E>(left.p, left.rs, left.cs, lbs);
    a.mid = ba_view<const E>(mid.p, mid.rs, mid.cs, mbs);
    a.right = ba_view<const E>(right.p, right.rs, right.cs, rbs);
    a.b = ba_view<const E>(b.p, b.rs, b.cs, bbs);
    a.y = ba_view<E>(y.p, y.rs, y.cs, ybs);
    a.s = s; a.s_stride = s_stride; a.ranks = ranks; a.count = count;
    a.m = (int)left.rows; a.n = (int)right.cols; a.k = (int)left.cols; a.ncols = (int)y.cols;
    ba_launch<E, E>(c, a, std::is_same<E, real_t<E>>::value ? "" : "<complex>");
}

// the mixed calls: factor views of S (strides in elements of S), b and y of E, s double
template <typename E, typename S>
static void ba_mixed(rc_context *c, const rc_matrix &left, int64_t lbs, const rc_matrix &mid, int64_t mbs, const double *s, int64_t s_stride,
                     const rc_matrix &right, int64_t rbs, const int64_t *ranks, int32_t count, const rc_matrix &b, int64_t bbs, const rc_matrix &y, int64_t ybs,
                     const char *tag) {
    BaArgs<E, S> a;
    a.left = ba_view<const S>(left.data, left.row_stride, left.col_stride, lbs);
    a.mid = ba_view<const S>(mid.data, mid.row_stride, mid.col_stride, mbs);
    a.right = ba_view<const S>(right.data, right.row_stride, right.col_stride, rbs);
    a.b = ba_view<const E>(b.data, b.row_stride, b.col_stride, bbs);
    a.y = ba_view<E>(y.data, y.row_stride, y.col_stride, ybs);
    a.s = s; a.s_stride = s_stride; a.ranks = ranks; a.count = count;
    a.m = (int)left.rows; a.n = (int)right.cols; a.k = (int)left.cols; a.ncols = (int)y.cols;
    ba_launch<E, S>(c, a, tag);
}

void batched_lowrank_apply_mixed(rc_context *c, bool complex_data, const rc_matrix &left, int64_t lbs, const rc_matrix &mid, int64_t mbs, const double *s,
                                 int64_t s_stride, const rc_matrix &right, int64_t rbs, const int64_t *ranks, int32_t count, const rc_matrix &b, int64_t bbs,
                                 const rc_matrix &y, int64_t ybs) {
    if (complex_data) ba_mixed<cplx<double>, cplx<float>>(c, left, lbs, mid, mbs, s, s_stride, right, rbs, ranks, count, b, bbs, y, ybs, "<complex,mixed>");
    else ba_mixed<double, float>(c, left, lbs, mid, mbs, s, s_stride, right, rbs, ranks, count, b, bbs, y, ybs, "<mixed>");
}

#define RC_INSTANTIATE_APPLY(E)                                                                                                             \
    template void batched_lowrank_apply<E>(rc_context *, Mat<E>, int64_t, Mat<E>, int64_t, const real_t<E> *, int64_t, Mat<E>, int64_t, const int64_t *, \
                                           int32_t, Mat<E>, int64_t, Mat<E>, int64_t);
RC_INSTANTIATE_APPLY(double)
RC_INSTANTIATE_APPLY(float)
RC_INSTANTIATE_APPLY(cplx<double>)
RC_INSTANTIATE_APPLY(cplx<float>)

}  // namespace rc
