// Residual norms of a batch of low-rank factorizations against their blocks in one rank-aware launch (rc_lowrank_residual_batched_*).
//
// Per block i, with r = ranks[i] clamped to [0, K] (K when there are no ranks) and Ah = left_i[:, :r] mid_i[:r, :r] diag(s_i[:r])
// right_i[:r, :] (absent factors omitted): err[i] = ||a_i - Ah||_F, nrm[i] = ||a_i||_F and, when asked for, e_i = a_i - Ah: the
// reference's rel_diff_fro(x.to_mat(), a) for the outputs of every batched compressor, without the m x n temporary of to_mat and for the
// tall blocks of the sketched column ID (m <= 65536).  Nothing at an index >= r is read.
//
// MI355X mapping.  The persistent grid of 256-thread workgroups (bid_grid), one workgroup per block from start to finish, nothing
// crossing workgroups, no atomics.  Two phases per block:
//   1. W (r x n), the factor the rebuild multiplies left by, produced only when mid or s is present (without either W is right itself and
//      the MFMA's B operand is read straight from right in phase 2, zero at an inner index >= r or a column >= n: no image, no workspace).
//      W0 = diag(s[:r]) right[:r, :], read with the lanes along right's smaller stride; with mid, W1 = mid[:r, :r] W0, one thread per
//      element, plain FMAs over the ascending inner index.  The image has the column index fastest (pitch BR: 16 modulo 32, the MFMA's B-operand read is then free of bank
//      conflicts); rows r .. 4 ceil(r / 4) - 1 and columns n .. 64 ceil(n / 64) - 1 are zeros written here, never values of a factor.
//      The images live in LDS when they fit BID_MAX_LDS next to the chunk images, else in the workgroup's slot of the grid-bounded
//      workspace (L2 resident: at most 128 x 528 elements, twice with mid); the plan only moves base pointers, so it cannot change a bit.
//      right (and mid, s) are read from memory once per block.
//   2. Row chunks of BR_ROWS = 32 rows against the resident W.  left's chunk (32 x 4 ceil(r / 4), zeros past m and past r) is staged
//      in LDS once per chunk -- left is read from HBM once -- and a's chunk streams through LDS in tiles of BR_COLS = 64 columns,
//      each element read from HBM once, both with the lanes along the operand's smaller stride (bid_load's rule) and that index
//      fastest in the image.  Per tile each wave owns a 16-column strip and both 16-row tiles: ceil(r / 4) MFMAs per tile
//      (v_mfma_f64_16x16x4_f64 / v_mfma_f32_16x16x4_f32, Acc<T> of rc_gemm.hpp) from zero accumulators, then e = a - acc on the a
//      values read back from LDS in the accumulator layout.  W is re-read ceil(m / 32) times, from LDS or L2.  Rows past m and columns
//      past n are zeros in LDS: the MFMA loop has no edge branch and, with finite factors, the padding adds +0 to the sums (a factor
//      that holds inf or NaN makes 0 x inf = NaN there, so that block's err is NaN where inf might be expected: it stays in its block).  When e is requested the tile
//      goes back into a's image and is stored with the lanes along e's smaller stride.
// Squares of e and of a are accumulated in f64 by each thread over its 8 elements of every tile, tiles in (row chunk, column tile)
// order; the 64 lanes are then summed by a butterfly and the four waves as (w0 + w1) + (w2 + w3).  The longest chain of additions a
// sum passes through is L(m, n) = 8 ceil(m / 32) ceil(n / 64) + 8.  Every order above is a function of (m, n, r) alone, which is what
// the bit-independence clause of the contract rests on.
// Scale (f64): a thread watches the exponent fields of the 8 elements it squares in a tile (ssq_watch, rc_device.hpp); while all lie in
// [2^-511, 2^486) the two sums above are the whole story, bit for bit.  A tile with a component outside takes its squares back and bins them
// as ?lassq does (ssq_add: med, big times 2^-538, sml times 2^537), each bin summed over the lanes and waves in the order above and the
// three combined once per block (ssq_norm).  The f32 instance keeps the single f64 sums: an f32 square cannot leave the f64 range.
#include <algorithm>

#include "rc_batched_launch.hpp"
#include "rc_common.hpp"
#include "rc_device.hpp"
#include "rc_gemm.hpp"

namespace rc {

namespace {

constexpr int BR_THREADS = BATCHED_THREADS;
constexpr int BR_ROWS = 32;  // rows of a and of left per chunk: two 16-row MFMA tiles
constexpr int BR_COLS = 64;  // columns of a per tile: one 16-column strip per wave
constexpr int BR_PER = BR_ROWS * BR_COLS / BR_THREADS;  // 8 elements of a tile per thread, staged and computed
constexpr int BR_PAR = BR_ROWS + 4;   // pitch of a's image with the row index fastest
constexpr int BR_PLR = BR_ROWS + 16;  // pitch of left's image with the row index fastest (16 modulo 32)
// pitch of a's image with the column index fastest: the accumulator-layout read has lanes 16 columns x 4 rows, the rows 1 (f64) or 4 (f32) apart
template <typename T>
constexpr int br_pac() { return sizeof(T) == 8 ? 80 : 68; }
template <typename T>
constexpr int br_a_elems() { return BR_ROWS * br_pac<T>() > BR_COLS * BR_PAR ? BR_ROWS * br_pac<T>() : BR_COLS * BR_PAR; }
__host__ __device__ constexpr int br_k4(int k) { return (k + 3) & ~3; }
__host__ __device__ constexpr int br_plk(int k) { return ((k + 31) & ~31) + 4; }  // pitch of left's image with the inner index fastest
__host__ __device__ constexpr int br_l_elems(int k) { return BR_ROWS * br_plk(k) > br_k4(k) * BR_PLR ? BR_ROWS * br_plk(k) : br_k4(k) * BR_PLR; }
__host__ __device__ constexpr int br_np(int n) { return (n + BR_COLS - 1) & ~(BR_COLS - 1); }
__host__ __device__ constexpr int br_pw(int n) { return br_np(n) + 16; }  // pitch of W's image
__host__ __device__ constexpr size_t br_w_elems(int k, int n, bool has_mid) { return (size_t)(has_mid ? 2 : 1) * br_k4(k) * br_pw(n); }

// dynamic LDS: red[8] (f64) | [W0 [W1, with mid]: K4 x pw(n), LDS plan only] a's tile image | left's chunk image
template <typename T>
size_t br_lds_bytes(int k, int n, bool has_mid, bool w_lds) {
    return 64 + ((w_lds ? br_w_elems(k, n, has_mid) : 0) + (size_t)br_a_elems<T>() + (size_t)br_l_elems(k)) * sizeof(T);
}

template <typename T>
struct BrArgs {
    Mat<T> a, left, mid, right, e;  // mid.p == nullptr: none; e.p == nullptr: the residual is not written
    int64_t abs, lbs, mbs, rbs, ebs, s_stride;
    const T *s;
    const int64_t *ranks;
    T *err, *nrm, *ws;
    int count;
    bool w_lds;   // W's images in LDS (else in the workgroup's workspace slot)
    bool direct;  // neither mid nor s: W is right itself, read in place
};

template <typename T>
__global__ __launch_bounds__(BR_THREADS) void k_batched_residual(BrArgs<T> g) {
    // f64 squares leave the range inside the domain of the compressors: ?lassq's three accumulators (rc_device.hpp).  f32 keeps the single
    // f64 accumulator: the square of an f32 component lies in [2^-298, 2^256] and cannot overflow or vanish there.
    constexpr bool WIDE = sizeof(T) == 8;
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const int m = (int)g.a.rows, n = (int)g.a.cols, K = (int)g.left.cols;
    const int np = br_np(n), pw = br_pw(n);
    const bool has_mid = g.mid.p != nullptr;
    const size_t wel = (size_t)br_k4(K) * pw;
    double *red = reinterpret_cast<double *>(smem_raw);
    T *lds = reinterpret_cast<T *>(smem_raw + 64);
    T *W0 = g.w_lds ? lds : g.direct ? lds : g.ws + (size_t)blockIdx.x * br_w_elems(K, n, has_mid);  // unused when direct
    T *W1 = W0 + wel;
    T *As = lds + (g.w_lds ? br_w_elems(K, n, has_mid) : 0);
    T *Ls = As + br_a_elems<T>();
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, r16 = lane & 15, k4 = lane >> 4;
    // the lanes of every staging loop run along the operand's smaller stride, and that index is the fastest one of the LDS image
    const bool a_rows = g.a.rs <= g.a.cs, l_rows = g.left.rs <= g.left.cs, r_rows = g.right.rs <= g.right.cs, e_rows = g.e.rs <= g.e.cs;
    const int as_sr = a_rows ? 1 : br_pac<T>(), as_sc = a_rows ? BR_PAR : 1;  // As[row * as_sr + col * as_sc]
    const int ls_sr = l_rows ? 1 : br_plk(K), ls_sk = l_rows ? BR_PLR : 1;    // Ls[row * ls_sr + k * ls_sk]
    // this thread's BR_PER elements of a tile when staging a (row0 + drow * q, col0 + dcol * q) and when storing e
    const int a_row0 = a_rows ? (tid & (BR_ROWS - 1)) : (tid / BR_COLS), a_col0 = a_rows ? (tid / BR_ROWS) : (tid & (BR_COLS - 1));
    const int a_drow = a_rows ? 0 : BR_THREADS / BR_COLS, a_dcol = a_rows ? BR_THREADS / BR_ROWS : 0;
    const int e_row0 = e_rows ? (tid & (BR_ROWS - 1)) : (tid / BR_COLS), e_col0 = e_rows ? (tid / BR_ROWS) : (tid & (BR_COLS - 1));
    const int e_drow = e_rows ? 0 : BR_THREADS / BR_COLS, e_dcol = e_rows ? BR_THREADS / BR_ROWS : 0;
    // and in the accumulator layout: rows i * 16 + Acc<T>::row(lane, reg) of column wv * 16 + r16
    const T *ls_ld = Ls + r16 * ls_sr + k4 * ls_sk;
    T *as_acc = As + (wv * 16 + r16) * as_sc;

    for (int b = blockIdx.x; b < g.count; b += gridDim.x) {
        int r = K;
        if (g.ranks) {
            const int64_t rv = g.ranks[b];
            r = rv < 0 ? 0 : rv > K ? K : (int)rv;
        }
        r = __builtin_amdgcn_readfirstlane(r);  // one value per block, uniform by construction: the loop bounds stay in scalar registers
        const int r4 = br_k4(r);
        const T *__restrict__ A = g.a.p + (int64_t)b * g.abs;
        const T *__restrict__ Lf = g.left.p + (int64_t)b * g.lbs;
        const T *__restrict__ Rt = g.right.p + (int64_t)b * g.rbs;
        const T *sb = g.s ? g.s + (int64_t)b * g.s_stride : nullptr;
        T *E = g.e.p ? g.e.p + (int64_t)b * g.ebs : nullptr;

        // ---- phase 1: W0 = diag(s[:r]) right[:r, :], zero rows r .. r4 - 1 and zero columns n .. np - 1 ----------------------------------
        const int wtot = g.direct ? 0 : r4 * np;  // without mid and s there is nothing to produce
        for (int idx = tid; idx < wtot; idx += BR_THREADS) {
            int k, j;
            if (r_rows) { k = idx % r4; j = idx / r4; } else { j = idx % np; k = idx / np; }
            T v = (T)0;
            if (k < r && j < n) {
                v = Rt[(int64_t)k * g.right.rs + (int64_t)j * g.right.cs];
                if (sb) v = sb[k] * v;
            }
            W0[(size_t)k * pw + j] = v;
        }
        if (!g.direct) __syncthreads();  // uniform over the grid
        const T *Wp = W0;
        if (has_mid) {  // W1 = mid[:r, :r] W0: the 64 lanes of a wave share the row l (np is a multiple of 64) and read one element of mid
            const T *__restrict__ Md = g.mid.p + (int64_t)b * g.mbs;
            for (int idx = tid; idx < wtot; idx += BR_THREADS) {
                const int j = idx % np, l = idx / np;
                T acc = (T)0;
                if (l < r && j < n) {
                    const T *mr = Md + (int64_t)l * g.mid.rs;
                    for (int p = 0; p < r; ++p) acc = fma(mr[(int64_t)p * g.mid.cs], W0[(size_t)p * pw + j], acc);
                }
                W1[(size_t)l * pw + j] = acc;
            }
            __syncthreads();
            Wp = W1;
        }
        const T *w_ld = Wp + (size_t)k4 * pw + wv * 16 + r16;

        // ---- phase 2: row chunks of a and left against W ------------------------------------------------------------------------------
        SumSq3 se{0.0, 0.0, 0.0}, sa{0.0, 0.0, 0.0};  // f32: med alone
        for (int m0 = 0; m0 < m; m0 += BR_ROWS) {
            const int ltot = BR_ROWS * r4;
            for (int idx = tid; idx < ltot; idx += BR_THREADS) {
                int row, k;
                if (l_rows) { row = idx & (BR_ROWS - 1); k = idx / BR_ROWS; } else { k = idx % r4; row = idx / r4; }
                const bool ok = m0 + row < m && k < r;
                Ls[row * ls_sr + k * ls_sk] = ok ? Lf[(int64_t)(m0 + row) * g.left.rs + (int64_t)k * g.left.cs] : (T)0;
            }
            for (int c0 = 0; c0 < n; c0 += BR_COLS) {
                T av[BR_PER];
#pragma unroll
                for (int q = 0; q < BR_PER; ++q) {
                    const int row = a_row0 + a_drow * q, col = a_col0 + a_dcol * q;
                    const bool ok = m0 + row < m && c0 + col < n;
                    av[q] = ok ? A[(int64_t)(m0 + row) * g.a.rs + (int64_t)(c0 + col) * g.a.cs] : (T)0;
                }
#pragma unroll
                for (int q = 0; q < BR_PER; ++q) As[(a_row0 + a_drow * q) * as_sr + (a_col0 + a_dcol * q) * as_sc] = av[q];
                __syncthreads();
                typename Acc<T>::type acc[2];
                [[maybe_unused]] const double se0 = se.med, sa0 = sa.med;
                [[maybe_unused]] unsigned emx = 0u, emn = ~0u;
                acc[0] = typename Acc<T>::type{0, 0, 0, 0};
                acc[1] = typename Acc<T>::type{0, 0, 0, 0};
                const int bcol = c0 + wv * 16 + r16;
                for (int ks = 0; ks < r4; ks += 4) {
                    T bf;
                    if (g.direct)  // uniform over the grid: right in place, zero past the rank and past n
                        bf = (ks + k4 < r && bcol < n) ? Rt[(int64_t)(ks + k4) * g.right.rs + (int64_t)bcol * g.right.cs] : (T)0;
                    else
                        bf = w_ld[(size_t)ks * pw + c0];
                    acc[0] = Acc<T>::mfma(ls_ld[ks * ls_sk], bf, acc[0]);
                    acc[1] = Acc<T>::mfma(ls_ld[16 * ls_sr + ks * ls_sk], bf, acc[1]);
                }
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int reg = 0; reg < 4; ++reg) {
                        T *pa = as_acc + (i * 16 + Acc<T>::row(lane, reg)) * as_sr;
                        const T x = *pa;
                        const T ev = x - acc[i][reg];
                        se.med = fma((double)ev, (double)ev, se.med);
                        sa.med = fma((double)x, (double)x, sa.med);
                        if constexpr (WIDE) {
                            ssq_watch(emx, emn, ev);
                            ssq_watch(emx, emn, x);
                        } else {
                            if (E) *pa = ev;
                        }
                    }
                if constexpr (WIDE) {
                    // a component of this thread's 8 elements out of the plain range: the tile's squares are taken back and binned.
                    // a's image still holds x (e is stored behind this), and x - acc is the same rounding as above
                    if (!ssq_all_plain(emx, emn)) {
                        se.med = se0;
                        sa.med = sa0;
#pragma unroll
                        for (int i = 0; i < 2; ++i)
#pragma unroll
                            for (int reg = 0; reg < 4; ++reg) {
                                T x = as_acc[(i * 16 + Acc<T>::row(lane, reg)) * as_sr];
                                asm volatile("" : "+v"(x));  // read again, not kept: eight more live residuals cost a wave per SIMD
                                ssq_add(se, x - acc[i][reg]);
                                ssq_add(sa, x);
                            }
                    }
                    if (E) {
#pragma unroll
                        for (int i = 0; i < 2; ++i)
#pragma unroll
                            for (int reg = 0; reg < 4; ++reg) {
                                T *pa = as_acc + (i * 16 + Acc<T>::row(lane, reg)) * as_sr;
                                T x = *pa;
                                asm volatile("" : "+v"(x));  // likewise
                                *pa = x - acc[i][reg];
                            }
                    }
                }
                if (E) {  // uniform over the grid
                    __syncthreads();
#pragma unroll
                    for (int q = 0; q < BR_PER; ++q) {
                        const int row = e_row0 + e_drow * q, col = e_col0 + e_dcol * q;
                        if (m0 + row < m && c0 + col < n) E[(int64_t)(m0 + row) * g.e.rs + (int64_t)(c0 + col) * g.e.cs] = As[row * as_sr + col * as_sc];
                    }
                }
                __syncthreads();  // a's image is rewritten by the next tile, left's by the next chunk
            }
        }
        // ---- the two sums: 64 lanes by a butterfly, then the four waves ------------------------------------------------------------------
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            se.med += __shfl_xor(se.med, off, 64);
            sa.med += __shfl_xor(sa.med, off, 64);
            if constexpr (WIDE) {
                se.big += __shfl_xor(se.big, off, 64);
                se.sml += __shfl_xor(se.sml, off, 64);
                sa.big += __shfl_xor(sa.big, off, 64);
                sa.sml += __shfl_xor(sa.sml, off, 64);
            }
        }
        [[maybe_unused]] double *red2 = reinterpret_cast<double *>(As);  // a's image is free behind the last tile's barrier
        if (lane == 0) {
            red[wv] = se.med;
            red[4 + wv] = sa.med;
            if constexpr (WIDE) {
                red2[wv] = se.big;
                red2[4 + wv] = se.sml;
                red2[8 + wv] = sa.big;
                red2[12 + wv] = sa.sml;
            }
        }
        __syncthreads();
        if (tid == 0) {
            if constexpr (WIDE) {
                g.err[b] = (T)ssq_norm((red[0] + red[1]) + (red[2] + red[3]), (red2[0] + red2[1]) + (red2[2] + red2[3]), (red2[4] + red2[5]) + (red2[6] + red2[7]));
                if (g.nrm)
                    g.nrm[b] = (T)ssq_norm((red[4] + red[5]) + (red[6] + red[7]), (red2[8] + red2[9]) + (red2[10] + red2[11]), (red2[12] + red2[13]) + (red2[14] + red2[15]));
            } else {
                g.err[b] = (T)sqrt((red[0] + red[1]) + (red[2] + red[3]));
                if (g.nrm) g.nrm[b] = (T)sqrt((red[4] + red[5]) + (red[6] + red[7]));
            }
        }
        __syncthreads();  // red and W's images are rewritten by the next block
    }
}

// the plan (at: W's images in LDS): in LDS when they fit next to the chunk images, else in the workgroup's slot of the grid-bounded
// workspace; without mid and s W is right itself: no image, no workspace (plan=W:right)
template <typename T>
BatchedPlan<bool> br_plan(int K, int n, bool has_mid, bool has_s) {
    if (!has_mid && !has_s) return {false, br_lds_bytes<T>(K, n, false, false), 0};
    return batched_lds_or_ws([&](bool w_lds) { return br_lds_bytes<T>(K, n, has_mid, w_lds); }, br_w_elems(K, n, has_mid) * sizeof(T), "lowrank_residual_batched");
}

}  // namespace

// The plan only moves base pointers, so it cannot change a block's bits.  One kernel per scalar type.  (T real: the complex elements'
// launcher is specialised in kernels_batched_residual_c.hip.)
template <typename T>
void batched_lowrank_residual(rc_context *c, Mat<T> a, int64_t abs, Mat<T> left, int64_t lbs, Mat<T> mid, int64_t mbs, const real_t<T> *s, int64_t s_stride,
                              Mat<T> right, int64_t rbs, const int64_t *ranks, int32_t count, Mat<T> e, int64_t ebs, real_t<T> *err, real_t<T> *nrm) {
    const int m = (int)a.rows, n = (int)a.cols, K = (int)left.cols;
    if (count <= 0) return;
    const bool has_mid = mid.p != nullptr;
    const bool direct = !has_mid && !s;
    const auto plan = br_plan<T>(K, n, has_mid, s != nullptr);
    const auto lch = batched_prepare(c, k_batched_residual<T>, "lowrank_residual_batched", plan.lds, plan.ws, count);
    ProfScope ps(c, "op:batched_residual %dx%d k=%d count=%d grid=%lld slots=%lld plan=W:%s,rows=%d,cols=%d%s%s%s%s", m, n, K, (int)count, (long long)lch.grid,
                 (long long)lch.slots, direct ? "right" : plan.at ? "lds" : "ws", BR_ROWS, BR_COLS, has_mid ? ",mid" : "", s ? ",s" : "", e.p ? ",e" : "",
                 nrm ? ",nrm" : "");
    BrArgs<T> g;
    g.a = a; g.left = left; g.mid = mid; g.right = right; g.e = e;
    g.abs = abs; g.lbs = lbs; g.mbs = mbs; g.rbs = rbs; g.ebs = ebs; g.s_stride = s_stride;
    g.s = s; g.ranks = ranks; g.err = err; g.nrm = nrm;
    g.ws = lch.template workspace<T>();
    g.count = (int)count; g.w_lds = plan.at; g.direct = direct;
    lch.launch(g);
}

template void batched_lowrank_residual<double>(rc_context *, Mat<double>, int64_t, Mat<double>, int64_t, Mat<double>, int64_t, const double *, int64_t, Mat<double>,
                                               int64_t, const int64_t *, int32_t, Mat<double>, int64_t, double *, double *);
template void batched_lowrank_residual<float>(rc_context *, Mat<float>, int64_t, Mat<float>, int64_t, Mat<float>, int64_t, const float *, int64_t, Mat<float>,
                                              int64_t, const int64_t *, int32_t, Mat<float>, int64_t, float *, float *);

}  // namespace rc
