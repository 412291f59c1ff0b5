// Residual norms of a batch of complex low-rank factorizations against their blocks in one rank-aware launch
// (rc_lowrank_residual_batched_c64 / _c32): the complex twin of kernels_batched_residual.hip on interleaved (re, im) data.
//
// Per block i, with r = ranks[i] clamped to [0, K] (K when there are no ranks) and Ah = left_i[:, :r] mid_i[:r, :r] diag(s_i[:r])
// right_i[:r, :] (absent factors omitted, s real, nothing conjugated: vt is already V^H and the two-sided c already Z2^H, as in
// rc_lowrank_apply_batched_c*): err[i] = ||a_i - Ah||_F and nrm[i] = ||a_i||_F in the real type R and, when asked for, the complex
// e_i = a_i - Ah.  Nothing at an index >= r is read.
//
// MI355X mapping: that of the real kernel.  The persistent grid of 256-thread workgroups (bid_grid), one workgroup per block from
// start to finish, nothing crossing workgroups, no atomics.  Two phases per block:
//   1. W (r x n), produced only when mid or s is present (without either the MFMA's B operand is read straight from right in phase 2,
//      one complex load per lane feeding both components, zero at an inner index >= r or a column >= n: plan=W:right, no image).
//      W0 = diag(s[:r]) right[:r, :], one rounding per component; with mid, W1 = mid[:r, :r] W0, one thread per element, plain FMAs
//      over the ascending inner index p from zero, the four real products of a term in the order
//          re = fma(mid_re, w_re, re); re = fma(-mid_im, w_im, re); im = fma(mid_re, w_im, im); im = fma(mid_im, w_re, im).
//      The images hold interleaved complex elements with the column index fastest, pitch np + 16 elements (np = 64 ceil(n / 64)):
//      the B-operand read (16 consecutive elements per inner index, 4 inner indices) is free of bank conflicts both as 8-byte
//      elements (32-lane groups, rows 16 modulo 32 elements apart) and as 16-byte elements (the 16-lane groups of ds_read_b128, rows
//      0 modulo 16 elements apart).  They live in LDS when they fit BID_MAX_LDS next to the chunk images, else in the workgroup's slot
//      of the grid-bounded workspace; the plan only moves base pointers, so it cannot change a bit.
//   2. Row chunks of BREC_ROWS = 32 rows against the resident W; left's chunk (32 x 4 ceil(r / 4), zeros past m and past r) is staged
//      once per chunk and a's chunk streams through LDS in tiles of BREC_COLS = 64 columns, both with the lanes along the operand's
//      smaller stride and that index fastest in the image.  Per tile each wave owns a 16-column strip and both 16-row tiles.  The
//      rebuild runs on v_mfma_f64_16x16x4_f64 / v_mfma_f32_16x16x4_f32 (Acc<R> of rc_gemm.hpp) with the real and imaginary parts as
//      separate real operands: per output element each of Re Ah and Im Ah is one accumulator chain from zero over the ascending
//      inner index, four terms per instruction, and within a step
//          Re takes MFMA(L_re, W_re) then MFMA(-L_im, W_im);   Im takes MFMA(L_re, W_im) then MFMA(L_im, W_re)
//      (the negation is a sign flip in a register: exact).  Each component of e = a - acc is one rounding.  Conjugating every
//      operand negates the second product of Re's pair twice and every product of Im's chain once, and both MFMAs round a sum and
//      its negation to opposite values (measured on MI355X for f32 and f64), so err and nrm keep their bits and e comes out
//      conjugated, except that an Im e cancelled to zero exactly is +0 either way (x - x = +0 in IEEE arithmetic); operands with
//      +0 imaginary parts add only zeros to Re's chain, which then carries the real kernel's values; a column of right that is a unit vector leaves one non-zero product in the chain and e is exactly zero there.
//      The 32 accumulator registers of c64 (two tiles x (re, im) x 4 x f64) leave the kernel far from the register limit.
// Squares of Re e, Im e (and of Re a, Im a) are accumulated in f64 by each thread over its 8 elements of every tile, re before im,
// tiles in (row chunk, column tile) order; the 64 lanes are then summed by a butterfly and the four waves as (w0 + w1) + (w2 + w3).
// The longest chain of additions is L_c(m, n) = 16 ceil(m / 32) ceil(n / 64) + 8.  Every order above is a function of (m, n, r)
// alone, which is what the bit-independence clause of the contract rests on.
// Scale (c64): a thread watches the exponent fields of the 8 elements it squares in a tile (ssq_watch, rc_device.hpp); while all lie in
// [2^-511, 2^486) the two sums above are the whole story, bit for bit.  A tile with a component outside takes its squares back and bins them
// as ?lassq does (ssq_add: med, big times 2^-538, sml times 2^537), each bin summed over the lanes and waves in the order above and the
// three combined once per block (ssq_norm).  The c32 instance keeps the single f64 sums: an f32 square cannot leave the f64 range.
#include <algorithm>

#include "rc_batched_launch.hpp"
#include "rc_common.hpp"
#include "rc_cplx.hpp"
#include "rc_device.hpp"
#include "rc_gemm.hpp"

namespace rc {

namespace {

constexpr int BREC_THREADS = BATCHED_THREADS;
constexpr int BREC_ROWS = 32;  // rows of a and of left per chunk: two 16-row MFMA tiles
constexpr int BREC_COLS = 64;  // columns of a per tile: one 16-column strip per wave
constexpr int BREC_PER = BREC_ROWS * BREC_COLS / BREC_THREADS;  // 8 complex elements of a tile per thread, staged and computed
constexpr int BREC_PAR = BREC_ROWS + 2;  // pitch of a's image with the row index fastest (2 modulo 16: no conflict for 16-byte elements)

// an element of the LDS and workspace images: a cplx<R> over-aligned to one 8- or 16-byte load (the caller's memory holds cplx<R>,
// aligned as R)
template <typename R>
struct alignas(2 * sizeof(R)) img_cx {
    R re, im;
};

// pitch of left's image with the row index fastest: 16 modulo 32 elements (8-byte elements), 0 modulo 16 (16-byte elements)
template <typename R>
__host__ __device__ constexpr int brec_plr() { return sizeof(R) == 8 ? BREC_ROWS : BREC_ROWS + 16; }
// pitch of a's image with the column index fastest: the accumulator-layout read has lanes 16 columns x 4 rows, the rows 1 (f64) or 4 (f32) apart
template <typename R>
__host__ __device__ constexpr int brec_pac() { return sizeof(R) == 8 ? 80 : 68; }
template <typename R>
__host__ __device__ constexpr int brec_a_elems() { return BREC_ROWS * brec_pac<R>() > BREC_COLS * BREC_PAR ? BREC_ROWS * brec_pac<R>() : BREC_COLS * BREC_PAR; }
__host__ __device__ constexpr int brec_k4(int k) { return (k + 3) & ~3; }
// pitch of left's image with the inner index fastest (2 modulo 32: the A-operand read, 16 rows x 4 inner indices, is free of conflicts)
__host__ __device__ constexpr int brec_plk(int k) { return ((k + 31) & ~31) + 2; }
template <typename R>
__host__ __device__ constexpr int brec_l_elems(int k) {
    return BREC_ROWS * brec_plk(k) > brec_k4(k) * brec_plr<R>() ? BREC_ROWS * brec_plk(k) : brec_k4(k) * brec_plr<R>();
}
__host__ __device__ constexpr int brec_np(int n) { return (n + BREC_COLS - 1) & ~(BREC_COLS - 1); }
__host__ __device__ constexpr int brec_pw(int n) { return brec_np(n) + 16; }  // pitch of W's image
__host__ __device__ constexpr size_t brec_w_elems(int k, int n, bool has_mid) { return (size_t)(has_mid ? 2 : 1) * brec_k4(k) * brec_pw(n); }

// dynamic LDS: red[8] (f64) | [W0 [W1, with mid]: K4 x pw(n), LDS plan only] a's tile image | left's chunk image (complex elements)
template <typename R>
size_t brec_lds_bytes(int k, int n, bool has_mid, bool w_lds) {
    return 64 + ((w_lds ? brec_w_elems(k, n, has_mid) : 0) + (size_t)brec_a_elems<R>() + (size_t)brec_l_elems<R>(k)) * sizeof(img_cx<R>);
}

// strided view of block 0 of one operand (in complex elements); the shapes travel once, in BrecArgs, not per operand as in CV<R>
template <typename R>
struct BrecView {
    cplx<R> *p;
    int64_t rs, cs;
};

template <typename R>
struct BrecArgs {
    BrecView<R> a, left, mid, right, e;  // mid.p == nullptr: none; e.p == nullptr: the residual is not written
    int64_t abs, lbs, mbs, rbs, ebs, s_stride;
    const R *s;
    const int64_t *ranks;
    R *err, *nrm;
    img_cx<R> *ws;
    int m, n, k, count;
    bool w_lds;   // W's images in LDS (else in the workgroup's workspace slot)
    bool direct;  // neither mid nor s: W is right itself, read in place
};

template <typename R>
__global__ __launch_bounds__(BREC_THREADS) void k_batched_residual_c(BrecArgs<R> g) {
    using C = img_cx<R>;
    using G = cplx<R>;
    typedef typename Acc<R>::type acc_t;
    // c64 squares leave the range inside the domain of the compressors: ?lassq's three accumulators (rc_device.hpp).  c32 keeps the single
    // f64 accumulator: the square of an f32 component lies in [2^-298, 2^256] and cannot overflow or vanish there.
    constexpr bool WIDE = sizeof(R) == 8;
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const int m = g.m, n = g.n, K = g.k;
    const int np = brec_np(n), pw = brec_pw(n);
    const bool has_mid = g.mid.p != nullptr;
    const size_t wel = (size_t)brec_k4(K) * pw;
    double *red = reinterpret_cast<double *>(smem_raw);
    C *lds = reinterpret_cast<C *>(smem_raw + 64);
    C *W0 = g.w_lds ? lds : g.direct ? lds : g.ws + (size_t)blockIdx.x * brec_w_elems(K, n, has_mid);  // unused when direct
    C *W1 = W0 + wel;
    C *As = lds + (g.w_lds ? brec_w_elems(K, n, has_mid) : 0);
    C *Ls = As + brec_a_elems<R>();
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, r16 = lane & 15, k4 = lane >> 4;
    // the lanes of every staging loop run along the operand's smaller stride, and that index is the fastest one of the LDS image
    const bool a_rows = g.a.rs <= g.a.cs, l_rows = g.left.rs <= g.left.cs, r_rows = g.right.rs <= g.right.cs, e_rows = g.e.rs <= g.e.cs;
    const int as_sr = a_rows ? 1 : brec_pac<R>(), as_sc = a_rows ? BREC_PAR : 1;    // As[row * as_sr + col * as_sc]
    const int ls_sr = l_rows ? 1 : brec_plk(K), ls_sk = l_rows ? brec_plr<R>() : 1;  // Ls[row * ls_sr + k * ls_sk]
    // this thread's BREC_PER elements of a tile when staging a (row0 + drow * q, col0 + dcol * q) and when storing e
    const int a_row0 = a_rows ? (tid & (BREC_ROWS - 1)) : (tid / BREC_COLS), a_col0 = a_rows ? (tid / BREC_ROWS) : (tid & (BREC_COLS - 1));
    const int a_drow = a_rows ? 0 : BREC_THREADS / BREC_COLS, a_dcol = a_rows ? BREC_THREADS / BREC_ROWS : 0;
    const int e_row0 = e_rows ? (tid & (BREC_ROWS - 1)) : (tid / BREC_COLS), e_col0 = e_rows ? (tid / BREC_ROWS) : (tid & (BREC_COLS - 1));
    const int e_drow = e_rows ? 0 : BREC_THREADS / BREC_COLS, e_dcol = e_rows ? BREC_THREADS / BREC_ROWS : 0;
    // and in the accumulator layout: rows i * 16 + Acc<R>::row(lane, reg) of column wv * 16 + r16
    const C *ls_ld = Ls + r16 * ls_sr + k4 * ls_sk;
    C *as_acc = As + (wv * 16 + r16) * as_sc;
    const C czero{(R)0, (R)0};

    for (int b = blockIdx.x; b < g.count; b += gridDim.x) {
        int r = K;
        if (g.ranks) {
            const int64_t rv = g.ranks[b];
            r = rv < 0 ? 0 : rv > K ? K : (int)rv;
        }
        r = __builtin_amdgcn_readfirstlane(r);  // one value per block, uniform by construction: the loop bounds stay in scalar registers
        const int r4 = brec_k4(r);
        const G *__restrict__ A = g.a.p + (int64_t)b * g.abs;
        const G *__restrict__ Lf = g.left.p + (int64_t)b * g.lbs;
        const G *__restrict__ Rt = g.right.p + (int64_t)b * g.rbs;
        const R *sb = g.s ? g.s + (int64_t)b * g.s_stride : nullptr;
        G *E = g.e.p ? g.e.p + (int64_t)b * g.ebs : nullptr;

        // ---- phase 1: W0 = diag(s[:r]) right[:r, :], zero rows r .. r4 - 1 and zero columns n .. np - 1 ----------------------------------
        const int wtot = g.direct ? 0 : r4 * np;  // without mid and s there is nothing to produce
        for (int idx = tid; idx < wtot; idx += BREC_THREADS) {
            int k, j;
            if (r_rows) { k = idx % r4; j = idx / r4; } else { j = idx % np; k = idx / np; }
            C v = czero;
            if (k < r && j < n) {
                const G x = Rt[(int64_t)k * g.right.rs + (int64_t)j * g.right.cs];
                v.re = x.re;
                v.im = x.im;
                if (sb) {
                    const R sk = sb[k];
                    v.re = sk * v.re;
                    v.im = sk * v.im;
                }
            }
            W0[(size_t)k * pw + j] = v;
        }
        if (!g.direct) __syncthreads();  // uniform over the grid
        const C *Wp = W0;
        if (has_mid) {  // W1 = mid[:r, :r] W0: the 64 lanes of a wave share the row l (np is a multiple of 64) and read one element of mid
            const G *__restrict__ Md = g.mid.p + (int64_t)b * g.mbs;
            for (int idx = tid; idx < wtot; idx += BREC_THREADS) {
                const int j = idx % np, l = idx / np;
                C acc = czero;
                if (l < r && j < n) {
                    const G *mr = Md + (int64_t)l * g.mid.rs;
                    for (int p = 0; p < r; ++p) {
                        const G mv = mr[(int64_t)p * g.mid.cs];
                        const C w = W0[(size_t)p * pw + j];
                        acc.re = fma(mv.re, w.re, acc.re);
                        acc.re = fma(-mv.im, w.im, acc.re);
                        acc.im = fma(mv.re, w.im, acc.im);
                        acc.im = fma(mv.im, w.re, acc.im);
                    }
                }
                W1[(size_t)l * pw + j] = acc;
            }
            __syncthreads();
            Wp = W1;
        }
        const C *w_ld = Wp + (size_t)k4 * pw + wv * 16 + r16;

        // ---- phase 2: row chunks of a and left against W ------------------------------------------------------------------------------
        SumSq3 se{0.0, 0.0, 0.0}, sa{0.0, 0.0, 0.0};  // c32: med alone
        for (int m0 = 0; m0 < m; m0 += BREC_ROWS) {
            const int ltot = BREC_ROWS * r4;
            for (int idx = tid; idx < ltot; idx += BREC_THREADS) {
                int row, k;
                if (l_rows) { row = idx & (BREC_ROWS - 1); k = idx / BREC_ROWS; } else { k = idx % r4; row = idx / r4; }
                C v = czero;
                if (m0 + row < m && k < r) {
                    const G x = Lf[(int64_t)(m0 + row) * g.left.rs + (int64_t)k * g.left.cs];
                    v.re = x.re;
                    v.im = x.im;
                }
                Ls[row * ls_sr + k * ls_sk] = v;
            }
            for (int c0 = 0; c0 < n; c0 += BREC_COLS) {
                G av[BREC_PER];
#pragma unroll
                for (int q = 0; q < BREC_PER; ++q) {
                    const int row = a_row0 + a_drow * q, col = a_col0 + a_dcol * q;
                    const bool ok = m0 + row < m && c0 + col < n;
                    av[q] = ok ? A[(int64_t)(m0 + row) * g.a.rs + (int64_t)(c0 + col) * g.a.cs] : G{(R)0, (R)0};
                }
#pragma unroll
                for (int q = 0; q < BREC_PER; ++q) As[(a_row0 + a_drow * q) * as_sr + (a_col0 + a_dcol * q) * as_sc] = C{av[q].re, av[q].im};
                __syncthreads();
                acc_t are[2], aim[2];
                [[maybe_unused]] const double se0 = se.med, sa0 = sa.med;
                [[maybe_unused]] unsigned emx = 0u, emn = ~0u;
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    are[i] = acc_t{0, 0, 0, 0};
                    aim[i] = acc_t{0, 0, 0, 0};
                }
                const int bcol = c0 + wv * 16 + r16;
                for (int ks = 0; ks < r4; ks += 4) {
                    C bf = czero;
                    if (g.direct) {  // uniform over the grid: right in place, zero past the rank and past n
                        if (ks + k4 < r && bcol < n) {
                            const G x = Rt[(int64_t)(ks + k4) * g.right.rs + (int64_t)bcol * g.right.cs];
                            bf.re = x.re;
                            bf.im = x.im;
                        }
                    } else {
                        bf = w_ld[(size_t)ks * pw + c0];
                    }
#pragma unroll
                    for (int i = 0; i < 2; ++i) {
                        const C lf = ls_ld[i * 16 * ls_sr + ks * ls_sk];
                        are[i] = Acc<R>::mfma(lf.re, bf.re, are[i]);
                        are[i] = Acc<R>::mfma(-lf.im, bf.im, are[i]);
                        aim[i] = Acc<R>::mfma(lf.re, bf.im, aim[i]);
                        aim[i] = Acc<R>::mfma(lf.im, bf.re, aim[i]);
                    }
                }
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int reg = 0; reg < 4; ++reg) {
                        C *pa = as_acc + (i * 16 + Acc<R>::row(lane, reg)) * as_sr;
                        const C x = *pa;
                        const R er = x.re - are[i][reg], ei = x.im - aim[i][reg];
                        se.med = fma((double)er, (double)er, se.med);
                        se.med = fma((double)ei, (double)ei, se.med);
                        sa.med = fma((double)x.re, (double)x.re, sa.med);
                        sa.med = fma((double)x.im, (double)x.im, sa.med);
                        if constexpr (WIDE) {
                            ssq_watch(emx, emn, er);
                            ssq_watch(emx, emn, ei);
                            ssq_watch(emx, emn, x.re);
                            ssq_watch(emx, emn, x.im);
                        } else {
                            if (E) *pa = C{er, ei};
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
                                C x = as_acc[(i * 16 + Acc<R>::row(lane, reg)) * as_sr];
                                asm volatile("" : "+v"(x.re), "+v"(x.im));  // read again, not kept: sixteen more live components cost registers
                                ssq_add(se, x.re - are[i][reg]);
                                ssq_add(se, x.im - aim[i][reg]);
                                ssq_add(sa, x.re);
                                ssq_add(sa, x.im);
                            }
                    }
                    if (E) {
#pragma unroll
                        for (int i = 0; i < 2; ++i)
#pragma unroll
                            for (int reg = 0; reg < 4; ++reg) {
                                C *pa = as_acc + (i * 16 + Acc<R>::row(lane, reg)) * as_sr;
                                C x = *pa;
                                asm volatile("" : "+v"(x.re), "+v"(x.im));  // likewise
                                *pa = C{x.re - are[i][reg], x.im - aim[i][reg]};
                            }
                    }
                }
                if (E) {  // uniform over the grid
                    __syncthreads();
#pragma unroll
                    for (int q = 0; q < BREC_PER; ++q) {
                        const int row = e_row0 + e_drow * q, col = e_col0 + e_dcol * q;
                        if (m0 + row < m && c0 + col < n) {
                            const C v = As[row * as_sr + col * as_sc];
                            E[(int64_t)(m0 + row) * g.e.rs + (int64_t)(c0 + col) * g.e.cs] = G{v.re, v.im};
                        }
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
                g.err[b] = (R)ssq_norm((red[0] + red[1]) + (red[2] + red[3]), (red2[0] + red2[1]) + (red2[2] + red2[3]), (red2[4] + red2[5]) + (red2[6] + red2[7]));
                if (g.nrm)
                    g.nrm[b] = (R)ssq_norm((red[4] + red[5]) + (red[6] + red[7]), (red2[8] + red2[9]) + (red2[10] + red2[11]), (red2[12] + red2[13]) + (red2[14] + red2[15]));
            } else {
                g.err[b] = (R)sqrt((red[0] + red[1]) + (red[2] + red[3]));
                if (g.nrm) g.nrm[b] = (R)sqrt((red[4] + red[5]) + (red[6] + red[7]));
            }
        }
        __syncthreads();  // red and W's images are rewritten by the next block
    }
}

template <typename R>
BrecView<R> brec_view(Mat<cplx<R>> v) { return BrecView<R>{v.p, v.rs, v.cs}; }

// the plan (at: W's images in LDS): the real kernel's rule (br_plan) on the over-aligned image elements
template <typename R>
BatchedPlan<bool> brec_plan(int K, int n, bool has_mid, bool has_s) {
    if (!has_mid && !has_s) return {false, brec_lds_bytes<R>(K, n, false, false), 0};
    return batched_lds_or_ws([&](bool w_lds) { return brec_lds_bytes<R>(K, n, has_mid, w_lds); }, brec_w_elems(K, n, has_mid) * sizeof(img_cx<R>),
                             "lowrank_residual_batched");
}

// The plan only moves base pointers, so it cannot change a block's bits.  One kernel per scalar type.  A body of its own, not the real
// launcher's (kernels_batched_residual.hip): the Args and the image element differ.  It stands inside this file's namespace, and
// batched_lowrank_residual<cplx<R>> below are explicit specialisations that call it.
template <typename R>
void brec_launch(rc_context *c, Mat<cplx<R>> a, int64_t abs, Mat<cplx<R>> left, int64_t lbs, Mat<cplx<R>> mid, int64_t mbs, const R *s, int64_t s_stride,
                 Mat<cplx<R>> right, int64_t rbs, const int64_t *ranks, int32_t count, Mat<cplx<R>> e, int64_t ebs, R *err, R *nrm) {
    const int m = (int)a.rows, n = (int)a.cols, K = (int)left.cols;
    if (count <= 0) return;
    const bool has_mid = mid.p != nullptr;
    const bool direct = !has_mid && !s;
    const auto plan = brec_plan<R>(K, n, has_mid, s != nullptr);
    const auto lch = batched_prepare(c, k_batched_residual_c<R>, "lowrank_residual_batched", plan.lds, plan.ws, count);
    ProfScope ps(c, "op:batched_residual<complex> %dx%d k=%d count=%d grid=%lld slots=%lld plan=W:%s,rows=%d,cols=%d%s%s%s%s", m, n, K, (int)count,
                 (long long)lch.grid, (long long)lch.slots, direct ? "right" : plan.at ? "lds" : "ws", BREC_ROWS, BREC_COLS, has_mid ? ",mid" : "", s ? ",s" : "",
                 e.p ? ",e" : "", nrm ? ",nrm" : "");
    BrecArgs<R> g;
    g.a = brec_view<R>(a); g.left = brec_view<R>(left); g.mid = brec_view<R>(mid); g.right = brec_view<R>(right); g.e = brec_view<R>(e);
    g.abs = abs; g.lbs = lbs; g.mbs = mbs; g.rbs = rbs; g.ebs = ebs; g.s_stride = s_stride;
    g.s = s; g.ranks = ranks; g.err = err; g.nrm = nrm;
    g.ws = lch.template workspace<img_cx<R>>();
    g.m = m; g.n = n; g.k = K; g.count = (int)count; g.w_lds = plan.at; g.direct = direct;
    lch.launch(g);
}

}  // namespace

#define RC_DEFINE_RESIDUAL(R)                                                                                                                   \
    template <>                                                                                                                                 \
    void batched_lowrank_residual<cplx<R>>(rc_context *c, Mat<cplx<R>> a, int64_t abs, Mat<cplx<R>> left, int64_t lbs, Mat<cplx<R>> mid, int64_t mbs, \
                                           const R *s, int64_t s_stride, Mat<cplx<R>> right, int64_t rbs, const int64_t *ranks, int32_t count,      \
                                           Mat<cplx<R>> e, int64_t ebs, R *err, R *nrm) {                                                           \
        brec_launch<R>(c, a, abs, left, lbs, mid, mbs, s, s_stride, right, rbs, ranks, count, e, ebs, err, nrm);                                    \
    }
RC_DEFINE_RESIDUAL(double)
RC_DEFINE_RESIDUAL(float)

}  // namespace rc
