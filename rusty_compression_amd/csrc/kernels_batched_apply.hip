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
#include "rc_common.hpp"
#include "rc_device.hpp"

namespace rc {

namespace {

constexpr int BA_THREADS = 256;
constexpr int BA_WAVES = BA_THREADS / 64;

template <typename R>
struct cpx {
    R re, im;
};

// element arithmetic shared by the real and the interleaved-complex instances
template <typename E>
struct El {
    using real = E;
    static __device__ __forceinline__ E zero() { return (E)0; }
    static __device__ __forceinline__ E fma(E a, E b, E acc) { return ::fma(a, b, acc); }
    static __device__ __forceinline__ E add(E a, E b) { return a + b; }
    static __device__ __forceinline__ E scale(E s, E v) { return s * v; }
    static __device__ __forceinline__ E shfl_xor(E v, int off) { return __shfl_xor(v, off, 64); }
};
template <typename R>
struct El<cpx<R>> {
    using real = R;
    using E = cpx<R>;
    static __device__ __forceinline__ E zero() { return {(R)0, (R)0}; }
    static __device__ __forceinline__ E fma(E a, E b, E acc) {
        acc.re = ::fma(a.re, b.re, acc.re);
        acc.re = ::fma(-a.im, b.im, acc.re);
        acc.im = ::fma(a.re, b.im, acc.im);
        acc.im = ::fma(a.im, b.re, acc.im);
        return acc;
    }
    static __device__ __forceinline__ E add(E a, E b) { return {a.re + b.re, a.im + b.im}; }
    static __device__ __forceinline__ E scale(R s, E v) { return {s * v.re, s * v.im}; }
    static __device__ __forceinline__ E shfl_xor(E v, int off) { return {__shfl_xor(v.re, off, 64), __shfl_xor(v.im, off, 64)}; }
};

// columns of a tile per scalar type, 16 for real and 8 for complex data: the staged b tile (n x NB) and two intermediates (k x NB)
// fit the LDS cap at n = 512, k = 128 in c64 (8 x (513 + 2 x 129) x 16 B = 96 KiB), and the NB accumulators, the NB values of In and the
// loads in flight of a thread stay in registers (f32 at 32 and c32 at 16 columns took all 256 VGPRs: one wave per SIMD)
template <typename E>
constexpr int ba_nb() { return sizeof(E) == sizeof(typename El<E>::real) ? 16 : 8; }

// strided view of one operand with its batch stride (all in elements of E)
template <typename E>
struct BaView {
    E *p;
    int64_t rs, cs, bs;
};

template <typename E>
struct BaArgs {
    BaView<const E> left, mid, right, b;
    BaView<E> y;
    const typename El<E>::real *s;
    int64_t s_stride;
    const int64_t *ranks;
    int count, m, n, k, ncols;  // ncols: nrhs, or n when reconstructing (b.p == nullptr)
};

// dynamic LDS: [Bs: NBT x (n|1), with b only] W0: NBT x (k|1) [W1: NBT x (k|1), with mid only]
template <typename E>
size_t ba_lds_bytes(int n, int k, int nbt, bool has_b, bool has_mid) {
    return ((has_b ? (size_t)nbt * (size_t)(n | 1) : 0) + (size_t)(has_mid ? 2 : 1) * nbt * (size_t)(k | 1)) * sizeof(E);
}

// sum of acc[] over the G lanes of a group (OFF = G / 2 on entry, CNT = the columns a lane still holds).  While a lane holds more
// than one column, a step keeps the lower half of them in the lanes whose bit OFF is clear and the upper half in the others, and
// adds the partner's partial sums of the kept half; a single column is summed by the plain butterfly.  Each sum is a + b of the two
// partners' values, the same bits on both sides.
template <int CNT, int OFF, typename E, int NBT>
__device__ __forceinline__ void ba_reduce(E (&acc)[NBT], int l) {
    if constexpr (OFF >= 1) {
        if constexpr (CNT > 1) {
            constexpr int H = CNT / 2;
            const bool up = (l & OFF) != 0;
#pragma unroll
            for (int i = 0; i < H; ++i) {
                const E send = up ? acc[i] : acc[i + H];
                const E keep = up ? acc[i + H] : acc[i];
                acc[i] = El<E>::add(keep, El<E>::shfl_xor(send, OFF));
            }
            ba_reduce<H, OFF / 2>(acc, l);
        } else {
            acc[0] = El<E>::add(acc[0], El<E>::shfl_xor(acc[0], OFF));
            ba_reduce<1, OFF / 2>(acc, l);
        }
    }
}

// after ba_reduce<NBT, G / 2>: lane l of the group holds the finished columns (l / SH) * CNTF + i, i < CNTF, where CNTF = NBT / G
// columns are left per lane when G < NBT, else one column shared by SH = G / NBT lanes (the first of them stores it)
template <int G, typename E, int NBT, typename Store>
__device__ __forceinline__ void ba_reduce_store(E (&acc)[NBT], int l, int row, bool rok, Store store) {
    ba_reduce<NBT, G / 2>(acc, l);
    constexpr int CNTF = G >= NBT ? 1 : NBT / G, SH = G >= NBT ? G / NBT : 1;
    if (rok && (l % SH) == 0) {
#pragma unroll
        for (int i = 0; i < CNTF; ++i) store(row, (l / SH) * CNTF + i, acc[i]);
    }
}

// store(row, c, sum_{j < red} M[row * rs + j * cs] * In[c * ldin + j]) for row < rows, c < NBT: M in global memory, read once and
// only at j < red; In in LDS, NBT columns of at least red elements, ldin apart
template <typename E, int NBT, typename Store>
__device__ __forceinline__ void ba_product(const E *__restrict__ M, int64_t rs, int64_t cs, int rows, int red, const E *In, int ldin, Store store, int tid) {
    const int lane = tid & 63, wv = tid >> 6;
    if (rs <= cs) {  // rows are the fast index: one thread per row, j ascending
        for (int row = tid; row < rows; row += BA_THREADS) {
            const E *mr = M + (int64_t)row * rs;
            E acc[NBT];
#pragma unroll
            for (int c = 0; c < NBT; ++c) acc[c] = El<E>::zero();
            for (int j = 0; j < red; ++j) {
                const E mv = mr[(int64_t)j * cs];
#pragma unroll
                for (int c = 0; c < NBT; ++c) acc[c] = El<E>::fma(mv, In[c * ldin + j], acc[c]);
            }
#pragma unroll
            for (int c = 0; c < NBT; ++c) store(row, c, acc[c]);
        }
        return;
    }
    // red is the fast index: G lanes per row (wave-uniform: red is)
    int lg = 0;
    while (lg < 6 && (1 << lg) < red) ++lg;
    const int G = 1 << lg, rpw = 64 >> lg, g = lane >> lg, l = lane & (G - 1);
    auto finish = [&](E(&acc)[NBT], int row, bool rok) {
        switch (lg) {
            case 0: ba_reduce_store<1>(acc, l, row, rok, store); break;
            case 1: ba_reduce_store<2>(acc, l, row, rok, store); break;
            case 2: ba_reduce_store<4>(acc, l, row, rok, store); break;
            case 3: ba_reduce_store<8>(acc, l, row, rok, store); break;
            case 4: ba_reduce_store<16>(acc, l, row, rok, store); break;
            case 5: ba_reduce_store<32>(acc, l, row, rok, store); break;
            default: ba_reduce_store<64>(acc, l, row, rok, store); break;
        }
    };
    // lanes past red or past the last row load nothing and multiply In[c][0] by zero
    if (red <= 64) {  // one j per lane: this lane's In values stay in registers, the loads of BA_U row groups are in flight together
        constexpr int BA_U = 4;
        const bool jok = l < red;
        E in[NBT];
#pragma unroll
        for (int c = 0; c < NBT; ++c) in[c] = In[c * ldin + (jok ? l : 0)];
        for (int rowb = wv * rpw; rowb < rows; rowb += BA_WAVES * rpw * BA_U) {
            E mv[BA_U];
#pragma unroll
            for (int u = 0; u < BA_U; ++u) {
                const int row = rowb + u * BA_WAVES * rpw + g;
                mv[u] = (jok && row < rows) ? M[(int64_t)row * rs + (int64_t)l * cs] : El<E>::zero();
            }
#pragma unroll
            for (int u = 0; u < BA_U; ++u) {
                if (rowb + u * BA_WAVES * rpw >= rows) break;  // wave-uniform
                const int row = rowb + u * BA_WAVES * rpw + g;
                E acc[NBT];
#pragma unroll
                for (int c = 0; c < NBT; ++c) acc[c] = El<E>::fma(mv[u], in[c], El<E>::zero());
                finish(acc, row, row < rows);
            }
        }
        return;
    }
    for (int row0 = wv; row0 < rows; row0 += BA_WAVES) {  // red > 64: G = 64, one row per wave
        const E *mr = M + (int64_t)row0 * rs;
        E acc[NBT];
#pragma unroll
        for (int c = 0; c < NBT; ++c) acc[c] = El<E>::zero();
#pragma unroll 4
        for (int j0 = 0; j0 < red; j0 += 64) {
            const int j = j0 + l;
            const bool ok = j < red;
            const E mv = ok ? mr[(int64_t)j * cs] : El<E>::zero();
            const E *ip = In + (ok ? j : 0);
#pragma unroll
            for (int c = 0; c < NBT; ++c) acc[c] = El<E>::fma(mv, ip[c * ldin], acc[c]);
        }
        ba_reduce_store<64>(acc, l, row0, true, store);
    }
}

// T[c * ld + i] = src[i * rs + (c0 + c) * cs] for i < rows, c < nb, zero for nb <= c < NBT; lanes along the fast index of src
template <typename E, int NBT>
__device__ __forceinline__ void ba_load_tile(E *T, int ld, const E *__restrict__ src, int64_t rs, int64_t cs, int rows, int c0, int nb, int tid) {
    const int total = rows * NBT;
    if (cs <= rs) {
        for (int idx = tid; idx < total; idx += BA_THREADS) {
            const int c = idx % NBT, i = idx / NBT;
            T[c * ld + i] = c < nb ? src[(int64_t)i * rs + (int64_t)(c0 + c) * cs] : El<E>::zero();
        }
    } else {
        for (int idx = tid; idx < total; idx += BA_THREADS) {
            const int i = idx % rows, c = idx / rows;
            T[c * ld + i] = c < nb ? src[(int64_t)i * rs + (int64_t)(c0 + c) * cs] : El<E>::zero();
        }
    }
}

template <typename E, int NBT>
__global__ __launch_bounds__(BA_THREADS) void k_batched_apply(BaArgs<E> a) {
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
        const E *Rt = a.right.p + blk * a.right.bs;
        if (a.b.p) {
            ba_load_tile<E, NBT>(Bs, ldn, a.b.p + blk * a.b.bs, a.b.rs, a.b.cs, n, c0, nb, tid);
            __syncthreads();
            ba_product<E, NBT>(Rt, a.right.rs, a.right.cs, r, n, Bs, ldn, [&](int row, int c, E v) { W0[c * ldk + row] = v; }, tid);
        } else {
            ba_load_tile<E, NBT>(W0, ldk, Rt, a.right.rs, a.right.cs, r, c0, nb, tid);
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
            ba_product<E, NBT>(a.mid.p + blk * a.mid.bs, a.mid.rs, a.mid.cs, r, r, W0, ldk, [&](int row, int c, E v) { W1[c * ldk + row] = v; }, tid);
            __syncthreads();
            Wc = W1;
        }
        // ---- y = left[:, :r] W ----------------------------------------------------------------------------------------------------------
        ba_product<E, NBT>(a.left.p + blk * a.left.bs, a.left.rs, a.left.cs, m, r, Wc, ldk, to_y, tid);
        __syncthreads();  // Bs, W0 and W1 are rewritten by the next unit
    }
}

template <typename E, int NBT>
void ba_launch_nbt(rc_context *c, const BaArgs<E> &a, const char *tag) {
    const void *kern = reinterpret_cast<const void *>(k_batched_apply<E, NBT>);
    static bool attr_set[64] = {};
    if (!attr_set[c->device & 63]) {
        RC_HIP(hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)BID_MAX_LDS));
        attr_set[c->device & 63] = true;
    }
    const size_t lds = ba_lds_bytes<E>(a.n, a.k, NBT, a.b.p != nullptr, a.mid.p != nullptr);
    RC_REQUIRE(lds <= BID_MAX_LDS, RC_RUNTIME_ERROR, "lowrank_apply_batched: %zu bytes of LDS", lds);
    const int64_t ntiles = (a.ncols + NBT - 1) / NBT, nunits = (int64_t)a.count * ntiles;
    int64_t slots = 0;
    const int64_t grid = bid_grid(c, kern, lds, 0, (int32_t)std::min<int64_t>(nunits, INT32_MAX), &slots);
    ProfScope ps(c, "op:batched_apply%s %dx%d k=%d count=%d grid=%lld slots=%lld plan=nb:%d,tiles:%lld,cols:%d,%s%s%s", tag, a.m, a.n, a.k, a.count,
                 (long long)grid, (long long)slots, NBT, (long long)ntiles, a.ncols, a.b.p ? "apply" : "to_mat", a.mid.p ? ",mid" : "", a.s ? ",s" : "");
    hipLaunchKernelGGL((k_batched_apply<E, NBT>), dim3((unsigned)grid), dim3(BA_THREADS), lds, c->stream, a);
}

// the tile width: the smallest of 1, 4, 8, 16 that covers the columns, at most the scalar type's NB.  The bits of an output
// element do not depend on it (see the head of this file).
template <typename E>
void ba_launch(rc_context *c, const BaArgs<E> &a, const char *tag) {
    constexpr int NB = ba_nb<E>();
    if (a.count <= 0) return;
    if (a.ncols <= 1) return ba_launch_nbt<E, 1>(c, a, tag);
    if (a.ncols <= 4) return ba_launch_nbt<E, 4>(c, a, tag);
    if constexpr (NB >= 16) {
        if (a.ncols <= 8) return ba_launch_nbt<E, 8>(c, a, tag);
    }
    ba_launch_nbt<E, NB>(c, a, tag);
}

template <typename E, typename P>
BaView<E> ba_view(P *p, int64_t rs, int64_t cs, int64_t bs) { return BaView<E>{reinterpret_cast<E *>(p), rs, cs, bs}; }

}  // namespace

template <typename T>
void batched_lowrank_apply(rc_context *c, Mat<T> left, int64_t lbs, Mat<T> mid, int64_t mbs, const T *s, int64_t s_stride, Mat<T> right, int64_t rbs,
                           const int64_t *ranks, int32_t count, Mat<T> b, int64_t bbs, Mat<T> y, int64_t ybs) {
    BaArgs<T> a;
    a.left = ba_view<const T>(left.p, left.rs, left.cs, lbs);
    a.mid = ba_view<const T>(mid.p, mid.rs, mid.cs, mbs);
    a.right = ba_view<const T>(right.p, right.rs, right.cs, rbs);
    a.b = ba_view<const T>(b.p, b.rs, b.cs, bbs);
    a.y = ba_view<T>(y.p, y.rs, y.cs, ybs);
    a.s = s; a.s_stride = s_stride; a.ranks = ranks; a.count = count;
    a.m = (int)left.rows; a.n = (int)right.cols; a.k = (int)left.cols; a.ncols = (int)y.cols;
    ba_launch<T>(c, a, "");
}

template <typename R>
void batched_lowrank_apply_c(rc_context *c, const rc_matrix &left, int64_t lbs, const rc_matrix &mid, int64_t mbs, const R *s, int64_t s_stride,
                             const rc_matrix &right, int64_t rbs, const int64_t *ranks, int32_t count, const rc_matrix &b, int64_t bbs, const rc_matrix &y,
                             int64_t ybs) {
    using E = cpx<R>;
    BaArgs<E> a;
    a.left = ba_view<const E>(left.data, left.row_stride, left.col_stride, lbs);
    a.mid = ba_view<const E>(mid.data, mid.row_stride, mid.col_stride, mbs);
    a.right = ba_view<const E>(right.data, right.row_stride, right.col_stride, rbs);
    a.b = ba_view<const E>(b.data, b.row_stride, b.col_stride, bbs);
    a.y = ba_view<E>(y.data, y.row_stride, y.col_stride, ybs);
    a.s = s; a.s_stride = s_stride; a.ranks = ranks; a.count = count;
    a.m = (int)left.rows; a.n = (int)right.cols; a.k = (int)left.cols; a.ncols = (int)y.cols;
    ba_launch<E>(c, a, "<complex>");
}

template void batched_lowrank_apply<double>(rc_context *, Mat<double>, int64_t, Mat<double>, int64_t, const double *, int64_t, Mat<double>, int64_t,
                                            const int64_t *, int32_t, Mat<double>, int64_t, Mat<double>, int64_t);
template void batched_lowrank_apply<float>(rc_context *, Mat<float>, int64_t, Mat<float>, int64_t, const float *, int64_t, Mat<float>, int64_t,
                                           const int64_t *, int32_t, Mat<float>, int64_t, Mat<float>, int64_t);
template void batched_lowrank_apply_c<double>(rc_context *, const rc_matrix &, int64_t, const rc_matrix &, int64_t, const double *, int64_t,
                                              const rc_matrix &, int64_t, const int64_t *, int32_t, const rc_matrix &, int64_t, const rc_matrix &, int64_t);
template void batched_lowrank_apply_c<float>(rc_context *, const rc_matrix &, int64_t, const rc_matrix &, int64_t, const float *, int64_t,
                                             const rc_matrix &, int64_t, const int64_t *, int32_t, const rc_matrix &, int64_t, const rc_matrix &, int64_t);

}  // namespace rc
