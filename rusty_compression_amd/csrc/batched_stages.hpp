// The stages the batched kernels of kernels_batched_id.hip (f64 / f32) and kernels_batched_id_c.hip (c64 / c32) have in common, written once
// over the element type E (double, float, cplx<double>, cplx<float>); R = real_t<E> is the type of norms, thresholds and singular values.
// Each of the two translation units instantiates them for its own two element types; nothing here is exported.
//
// What stands here once: the fill, the column norms and their power-of-two normalisation, the step loop of the pivoted QR (bid_qrcp), the
// blocked back substitution for Z (bid_z), the column-ID and two-sided kernels with the carve-up of their LDS (bid_carve) and their plans,
// the Jacobi sweep schedule (bsv_jacobi) and the stack load of the tall recompressions (brt_stack_load).  The launcher bodies of both
// families stand in batched_launchers.hpp.  The per-element operations they are written in: elem<E> (zero, one), abs2, cj (the identity on reals), ediv, pow2_key_max, escale and
// submul -- the real ones below, the complex ones in rc_cplx.hpp.
//
// What stays per family, in the two .hip files, because its arithmetic or its register budget differs: the trailing update bid_apply /
// bic_apply (two columns in flight per wave for real, one for complex), the Jacobi rounds bsv_round / bsc_round, bsv_sign / bsc_phase, the
// form_u routines, *_reflect_back, brt_form_u / brtc_form_u / brl_form_vt, the core products, the bodies of the SVD and recompression
// kernels (their LDS and workspace placement differs by the complex G flag) with the sort of their singular values, the sketch and
// range-step kernels with their MFMA staging.  The two
// reflector formulas (?larfg) stand side by side inside bid_qrcp, and the shared loops call bid_apply / bic_apply and bsv_round /
// bsc_round directly, each under `if constexpr` on the element type.
//
// The spelling of the shared text decides whether a kernel's code object moves.  What moved instructions while this file was written:
// acc = acc - a * b where the real kernels have acc -= a * b; a run-time `ti < NB` guard for the 16 x 16 tile; the reflector formulas or
// the calls of bid_apply / bsv_round behind a function of their own (overloaded or not, results by value or by reference); the carve-up
// in byte offsets, or with int counts.  After any edit here compare the device assembly of both files with the parent's
// (tools/device_asm_diff.py).
#pragma once
#include <algorithm>
#include <type_traits>

#include "rc_batched_launch.hpp"
#include "rc_common.hpp"
#include "rc_cplx.hpp"
#include "rc_device.hpp"

namespace rc {

namespace {

constexpr int BID_THREADS = BATCHED_THREADS;
constexpr int BID_WAVES = BID_THREADS / 64;
constexpr int BID_NB = 16;  // back-substitution tile of the real kernels (k_id_z's)
constexpr int BIC_NB = 8;   // of the complex kernels (their register budget: every instance runs without scratch)

// ---- the element operations, real side ---------------------------------------------------------------------------------------------
template <typename E>
struct elem {
    static __host__ __device__ __forceinline__ E zero() { return (E)0; }
    static __host__ __device__ __forceinline__ E one() { return (E)1; }
};
template <typename E> constexpr bool is_real_elem = std::is_same<E, real_t<E>>::value;
template <typename E> constexpr int z_tile = is_real_elem<E> ? BID_NB : BIC_NB;
template <typename T> __device__ __forceinline__ T abs2(T v) { return v * v; }
template <typename T> __device__ __forceinline__ T cj(T v) { return v; }
template <typename T> __device__ __forceinline__ T ediv(T a, T b) { return a / b; }
template <typename T> __device__ __forceinline__ T pow2_key_max(T v) { return pow2_key(v); }
template <typename T> __device__ __forceinline__ T escale(T v, T s) { return v * s; }
template <typename T> __device__ __forceinline__ void submul(T &acc, T a, T b) { acc -= a * b; }

// ---- what the shared loops call of each family's own routines (defined in the two .hip files; a translation unit uses its own pair) ----
template <typename T, int NE>
__device__ __forceinline__ void bid_apply(T *W, int ldw, int m, int n, int j, const int *jp, T *vn1, T *vn2, T tj, int wv, int lane);
template <typename R, int NE>
__device__ __forceinline__ void bic_apply(cplx<R> *W, int ldw, int m, int n, int j, const int *jp, R *vn1, R *vn2, cplx<R> tj, int wv, int lane);
template <typename T, int NE>
__device__ __forceinline__ void bsv_round(T *G, int ldg, T *J, int ldj, int N, int p, int q, T tol, T tol2, int ll, int *flag);
template <typename R, int NE>
__device__ __forceinline__ void bsc_round(cplx<R> *G, int ldg, cplx<R> *J, int ldj, int N, int p, int q, R tol, R tol2, int ll, int *flag);

// ---- the three stages of one factorization, shared by k_batched_id and both phases of k_batched_two_sided ------------------------
// (m x n below is the matrix being factored: A for a column ID, C^H for the row side of a two-sided ID)

// the initial (real) column norms of the working copy W (m x n, column c at W + c * ldw) and the identity permutation
template <typename E>
__device__ __forceinline__ void bid_norms(const E *W, int ldw, int m, int n, real_t<E> *vn1, real_t<E> *vn2, int *jp, int wv, int lane) {
    using R = real_t<E>;
    for (int c = wv; c < n; c += BID_WAVES) {
        R acc = 0;
        for (int i = lane; i < m; i += 64) acc += abs2(W[(size_t)c * ldw + i]);
        acc = wave_sum_dpp(acc);
        if (lane == 0) { const R nr = sqrt(acc); vn1[c] = nr; vn2[c] = nr; jp[c] = c; }
    }
    __syncthreads();
}

// working copy W[c * ldw + i] = at(i, c), read with the lanes along i (lanes_on_rows) or along c (the input's fast direction)
template <typename E, typename At>
__device__ __forceinline__ void bid_fill(E *W, int ldw, int m, int n, bool lanes_on_rows, At at, int wv, int lane) {
    if (lanes_on_rows) {
        for (int c = wv; c < n; c += BID_WAVES)
            for (int i = lane; i < m; i += 64) W[(size_t)c * ldw + i] = at(i, c);
    } else {
        for (int i = wv; i < m; i += BID_WAVES)
            for (int c = lane; c < n; c += 64) W[(size_t)c * ldw + i] = at(i, c);
    }
    __syncthreads();
}

// the working copy as the caller's entries stand, then the initial column norms and the identity permutation (the recompression kernels)
template <typename E, typename At>
__device__ __forceinline__ void bid_load(E *W, int ldw, int m, int n, bool lanes_on_rows, At at, real_t<E> *vn1, real_t<E> *vn2, int *jp, int wv, int lane) {
    bid_fill(W, ldw, m, n, lanes_on_rows, at, wv, lane);
    bid_norms(W, ldw, m, n, vn1, vn2, jp, wv, lane);
}

// bid_norms on a working copy of any scale: W is first brought to a largest magnitude in [1, 2) by the exact power of two 2^-e
// (block_pow2_exponent, rc_device.hpp; e = 0 for a zero block and for one with a non-finite entry), so that neither these sums of squares
// nor those of bid_qrcp and the trailing update leave the normal range.  For complex elements the magnitude is the largest real or
// imaginary part (within sqrt 2 of the largest modulus, and never overflowing).  One more pass over W before the first step, none inside
// the step loop.  Returns e: W holds 2^-e times the block, and only an output that carries the block's scale and is produced from W (the
// singular values of the SVD kernels) multiplies 2^e back; pivots, ranks, Z, Q, U and V^T carry none, C, X and P are taken from the input
// itself.  stage: four elements no thread reads before the next barrier (red + 4).
template <typename E>
__device__ __forceinline__ int bid_norms_pow2(E *W, int ldw, int m, int n, real_t<E> *vn1, real_t<E> *vn2, int *jp, real_t<E> *stage, int wv, int lane) {
    using R = real_t<E>;
    R mx = 0;
    for (int c = wv; c < n; c += BID_WAVES)
        for (int i = lane; i < m; i += 64) mx = max(mx, pow2_key_max(W[(size_t)c * ldw + i]));
    const int e = block_pow2_exponent(mx, stage, wv, lane);
    const R sc = ldexp((R)1, -e);
    for (int c = wv; c < n; c += BID_WAVES) {  // bid_norms' sums on the scaled entries; a wave rewrites the columns it read above
        R acc = 0;
        for (int i = lane; i < m; i += 64) {
            const E v = escale(W[(size_t)c * ldw + i], sc);
            W[(size_t)c * ldw + i] = v;
            acc += abs2(v);
        }
        acc = wave_sum_dpp(acc);
        if (lane == 0) { const R nr = sqrt(acc); vn1[c] = nr; vn2[c] = nr; jp[c] = c; }
    }
    __syncthreads();
    return e;
}

// bid_load for a caller's block of any scale (the IDs and the SVD): the fill, then bid_norms_pow2.  Returns the block's exponent.
template <typename E, typename At>
__device__ __forceinline__ int bid_load_pow2(E *W, int ldw, int m, int n, bool lanes_on_rows, At at, real_t<E> *vn1, real_t<E> *vn2, int *jp, real_t<E> *stage,
                                             int wv, int lane) {
    bid_fill(W, ldw, m, n, lanes_on_rows, at, wv, lane);
    return bid_norms_pow2(W, ldw, m, n, vn1, vn2, jp, stage, wv, lane);
}

// truncated pivoted QR of the working copy, at most k steps: pivots in jp (?geqp3's rule), R and the Householder vectors in W (LAPACK
// format, physical column order).  Returns the rank: the first j < k with R_jj == 0 or (tol > 0 and |R_jj / R_00| < tol), else k.
// FULL (the batched SVD): no stopping rule, all k steps are taken (an exactly zero pivot column is a step with H = I) and tau_j goes
// to taus[j]; returns k.
template <typename E, bool FULL = false>
__device__ __forceinline__ int bid_qrcp(E *W, int ldw, int m, int n, int k, double tol, int *jp, real_t<E> *vn1, real_t<E> *vn2, real_t<E> *red, int tid, int wv,
                                        int lane, E *taus = nullptr) {
    using R = real_t<E>;
    int r = k;
    [[maybe_unused]] R r00 = 0;
    for (int j = 0; j < k; ++j) {
        if (wv == 0) {  // pivot: first maximum of the partial norms; NaN never wins (v > best), no valid index -> j
            R best = (R)-1;
            int bi = 0x7fffffff;
            for (int p = j + lane; p < n; p += 64) {
                const R v = fabs(vn1[p]);
                if (v > best) { best = v; bi = p; }
            }
            const R mx = wave_max_dpp(best);
            const int pv = wave_min_dpp(best == mx ? bi : 0x7fffffff);
            const int pvt = (pv >= j && pv < n) ? pv : j;
            if (lane == 0 && pvt != j) {  // ?laqp2: swap the indices, carry the norms of position j to pvt
                const int t = jp[pvt]; jp[pvt] = jp[j]; jp[j] = t;
                vn1[pvt] = vn1[j];
                vn2[pvt] = vn2[j];
            }
        }
        __syncthreads();
        // ?larfg on column jp[j], rows j..m-1: scales the rows below j, beta to col[j]; tau == 0 (H = I) leaves the column as it is
        E *col = W + (size_t)jp[j] * ldw;
        const E alpha = col[j];
        R acc = 0;
        for (int i = j + 1 + tid; i < m; i += BID_THREADS) acc += abs2(col[i]);
        acc = wave_sum_dpp(acc);
        if (lane == 0) red[wv] = acc;
        __syncthreads();  // also orders every thread's read of alpha before the write of beta below
        const R ssq = (red[0] + red[1]) + (red[2] + red[3]);
        const R xnorm = sqrt(ssq);
        R beta;
        E tj;
        if constexpr (is_real_elem<E>) {  // k_qr_pivot_reflect's formula
            beta = alpha, tj = 0;
            if (xnorm != (R)0) {
                beta = -copysign(hypot(alpha, xnorm), alpha);
                const R scal = (R)1 / (alpha - beta);
                for (int i = j + 1 + tid; i < m; i += BID_THREADS) col[i] *= scal;
                tj = (beta - alpha) / beta;
                if (tid == 0) col[j] = beta;
            }
        } else {  // k_c_qr_pivot_reflect's: beta real, tau complex, the scale 1 / (alpha - beta) by Smith division; H = I only when
                  // xnorm == 0 and alpha.im == 0
            beta = alpha.re;
            tj = czero<R>();
            if (xnorm != (R)0 || alpha.im != (R)0) {
                beta = -copysign(sqrt(alpha.re * alpha.re + alpha.im * alpha.im + ssq), alpha.re);  // ?lapy3
                const E scal = cdiv(cone<R>(), E{alpha.re - beta, alpha.im});
                for (int i = j + 1 + tid; i < m; i += BID_THREADS) col[i] = col[i] * scal;
                tj = E{(beta - alpha.re) / beta, -alpha.im / beta};
                if (tid == 0) col[j] = E{beta, (R)0};
            }
        }
        if constexpr (FULL) {
            if (tid == 0) taus[j] = tj;
        } else {
            // R_jj = beta (real) decides the rank (qr.rs:187-200 as a ratio; uniform across the workgroup)
            if (j == 0) r00 = beta;
            if (beta == (R)0 || (tol > 0.0 && (double)fabs(beta / r00) < tol)) { r = j; break; }
        }
        __syncthreads();
        if (j + 1 < n) {
            const int rem = m - j;
            if constexpr (is_real_elem<E>) {
                if (rem <= 128) bid_apply<E, 2>(W, ldw, m, n, j, jp, vn1, vn2, tj, wv, lane);
                else if (rem <= 256) bid_apply<E, 4>(W, ldw, m, n, j, jp, vn1, vn2, tj, wv, lane);
                else bid_apply<E, 8>(W, ldw, m, n, j, jp, vn1, vn2, tj, wv, lane);
            } else {
                if (rem <= 128) bic_apply<R, 2>(W, ldw, m, n, j, jp, vn1, vn2, tj, wv, lane);
                else if (rem <= 256) bic_apply<R, 4>(W, ldw, m, n, j, jp, vn1, vn2, tj, wv, lane);
                else bic_apply<R, 8>(W, ldw, m, n, j, jp, vn1, vn2, tj, wv, lane);
            }
        }
        __syncthreads();
    }
    __syncthreads();
    return r;
}

// Z = [I | R11^-1 R12] P^T (k x n, rows r..k-1 zero) into Zb[i * zrs + c * zcs], or its conjugate when CONJ (the row side's Z2^H):
// k_id_z's blocked back substitution with k -> r (z_tile<E> square tiles of R11 staged in LDS, one thread per right-hand side, Smith
// division on a complex diagonal), each column written straight to its final place
template <typename E, bool CONJ = false>
__device__ __forceinline__ void bid_z(const E *W, int ldw, int n, int r, int k, const int *jp, E (*tile)[z_tile<E> + 1], E *Zb, int64_t zrs, int64_t zcs, int tid) {
    constexpr int NB = z_tile<E>;
    const int nblk = (r + NB - 1) / NB;
    const int ti = tid / NB, tk = tid % NB;
    auto out = [](E v) { return CONJ ? cj(v) : v; };  // its own inverse
    for (int q0 = 0; q0 < n; q0 += BID_THREADS) {
        const int p = q0 + tid;  // position in the pivoted order
        const bool inside = p < n;
        const int dc = inside ? jp[p] : 0;  // where column p of [I | R11^-1 R12] goes
        const bool active = inside && p >= r;
        E *zc = Zb + (int64_t)dc * zcs;
        if (inside) {
            if (p < r)
                for (int i = 0; i < k; ++i) zc[i * zrs] = (i == p) ? elem<E>::one() : elem<E>::zero();
            else
                for (int i = r; i < k; ++i) zc[i * zrs] = elem<E>::zero();
        }
        const E *bcol = W + (size_t)dc * ldw;  // R12[:, p]: rows 0 .. r-1 of the physical column
        for (int bi = nblk - 1; bi >= 0; --bi) {
            const int r0 = bi * NB;
            E acc[NB];
#pragma unroll
            for (int ii = 0; ii < NB; ++ii) acc[ii] = (active && r0 + ii < r) ? bcol[r0 + ii] : elem<E>::zero();
            for (int bj = nblk - 1; bj >= bi; --bj) {
                const int c0 = bj * NB;
                __syncthreads();
                if (NB * NB == BID_THREADS || ti < NB) {  // every thread stages an entry of a 16 x 16 tile, the first 64 of an 8 x 8 one
                    const int i = r0 + ti, l = c0 + tk;
                    tile[ti][tk] = (i < r && l < r && i <= l) ? W[(size_t)jp[l] * ldw + i] : elem<E>::zero();
                }
                __syncthreads();
                if (bj > bi) {
                    E x[NB];
#pragma unroll
                    for (int jj = 0; jj < NB; ++jj) x[jj] = (active && c0 + jj < r) ? out(zc[(c0 + jj) * zrs]) : elem<E>::zero();  // this thread's own finished block
#pragma unroll
                    for (int jj = 0; jj < NB; ++jj)
#pragma unroll
                        for (int ii = 0; ii < NB; ++ii) submul(acc[ii], tile[ii][jj], x[jj]);
                } else {
#pragma unroll
                    for (int ii = NB - 1; ii >= 0; --ii) {
                        if (r0 + ii < r) {
                            acc[ii] = ediv(acc[ii], tile[ii][ii]);
#pragma unroll
                            for (int i2 = 0; i2 < ii; ++i2) submul(acc[i2], tile[i2][ii], acc[ii]);
                        }
                    }
                }
            }
            if (active) {
#pragma unroll
                for (int ii = 0; ii < NB; ++ii)
                    if (r0 + ii < r) zc[(r0 + ii) * zrs] = out(acc[ii]);
            }
        }
    }
}

// ---- the column-ID and two-sided kernels --------------------------------------------------------------------------------------------
// Their dynamic LDS carved up from its base (W, when it lives in LDS, stands first: w_elems elements), for the kernels and, from a
// null base, for the plans (bid_lds_bytes).  Each family keeps the order it had:
//   real     [W] vn1[nv] vn2[nv] tile[16 x 17] red[8] | jp[n] jp2[m2]   (ints last: the T arrays stay aligned)
//   complex  [W] tile[8 x 9] complex | vn1[nv] vn2[nv] red[8] real | jp[n] jp2[m2]
// nv = n for the column ID, max(m, n) for the two-sided ID, whose second permutation jp2 has m2 = m entries.
template <typename E>
struct BidLds {
    E (*tile)[z_tile<E> + 1];
    real_t<E> *vn1, *vn2, *red;
    int *jp, *jp2;
};
template <typename E>
__host__ __device__ __forceinline__ BidLds<E> bid_carve(E *lds, size_t nv, size_t n) {
    constexpr int NB = z_tile<E>;
    BidLds<E> o;
    if constexpr (is_real_elem<E>) {
        o.vn1 = lds;
        o.vn2 = o.vn1 + nv;
        o.tile = reinterpret_cast<E(*)[NB + 1]>(o.vn2 + nv);
        o.red = o.vn2 + nv + NB * (NB + 1);
    } else {
        o.tile = reinterpret_cast<E(*)[NB + 1]>(lds);
        o.vn1 = reinterpret_cast<real_t<E> *>(lds + NB * (NB + 1));
        o.vn2 = o.vn1 + nv;
        o.red = o.vn2 + nv;
    }
    o.jp = reinterpret_cast<int *>(o.red + 8);
    o.jp2 = o.jp + n;
    return o;
}
template <typename E>
size_t bid_lds_bytes(size_t w_elems, int nv, int n, int m2) {
    return w_elems * sizeof(E) + (size_t)(reinterpret_cast<char *>(bid_carve<E>(nullptr, nv, n).jp2 + m2) - static_cast<char *>(nullptr));
}
// W of the two-sided kernel in LDS: the larger of phase 1's n x (m|1) and phase 2's m x (k|1)
__host__ __device__ inline size_t bts_w_elems(int m, int n, int k) {
    const size_t w1 = (size_t)n * (size_t)(m | 1), w2 = (size_t)m * (size_t)(k | 1);
    return w1 > w2 ? w1 : w2;
}

template <typename E, bool IN_LDS>
__global__ __launch_bounds__(BID_THREADS) void k_batched_id(Mat<E> a, int64_t abs, int count, int k, double tol, Mat<E> cm, int64_t cbs, Mat<E> z,
                                                            int64_t zbs, int64_t *__restrict__ col_ind, int64_t *__restrict__ ranks, E *__restrict__ ws) {
    using R = real_t<E>;
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const int m = (int)a.rows, n = (int)a.cols;
    const int ldw = IN_LDS ? (m | 1) : m;
    E *lds = reinterpret_cast<E *>(smem_raw);
    E *W = IN_LDS ? lds : ws + (size_t)blockIdx.x * (size_t)m * (size_t)n;
    const BidLds<E> o = bid_carve(lds + (IN_LDS ? (size_t)n * ldw : 0), n, n);
    E(*tile)[z_tile<E> + 1] = o.tile;
    R *vn1 = o.vn1, *vn2 = o.vn2, *red = o.red;
    int *jp = o.jp;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;

    for (int b = blockIdx.x; b < count; b += gridDim.x) {
        const E *__restrict__ A = a.p + (int64_t)b * abs;
        bid_load_pow2(W, ldw, m, n, a.rs <= a.cs, [&](int i, int c) { return A[i * a.rs + c * a.cs]; }, vn1, vn2, jp, red + 4, wv, lane);
        const int r = bid_qrcp(W, ldw, m, n, k, tol, jp, vn1, vn2, red, tid, wv, lane);

        // ---- outputs: permutation, rank, C, Z -------------------------------------------------------------------
        for (int p = tid; p < n; p += BID_THREADS) col_ind[(int64_t)b * n + p] = jp[p];
        if (tid == 0) ranks[b] = r;
        E *Cb = cm.p + (int64_t)b * cbs;
        for (int j = wv; j < k; j += BID_WAVES) {
            const E *src = A + (int64_t)jp[j] * a.cs;
            for (int i = lane; i < m; i += 64) Cb[i * cm.rs + j * cm.cs] = j < r ? src[i * a.rs] : elem<E>::zero();
        }
        bid_z(W, ldw, n, r, k, jp, tile, z.p + (int64_t)b * zbs, z.rs, z.cs, tid);
        __syncthreads();  // W, jp and the norms are rewritten by the next matrix
    }
}

// Two-sided ID A ~ C X R per matrix: phase 1 is k_batched_id's column ID (R = its Z, col_ind, the rank r); phase 2 is the column
// ID of C^H = conj(A[:, col_ind[:r]])^T (r x m; C^T for real elements) at rank r with tol = 0, by the same three stages: its permutation
// is row_ind and its Z, conjugated and written through c's transposed view, is c = Z2^H; X = A[row_ind[:r], col_ind[:r]] is gathered
// from the input.  In the workspace variant phase 2's m x r copy (ldw = r) fits the m x n slot; the LDS variant reserves the larger of
// the two phases' needs.
template <typename E, bool IN_LDS>
__global__ __launch_bounds__(BID_THREADS) void k_batched_two_sided(Mat<E> a, int64_t abs, int count, int k, double tol, Mat<E> cm, int64_t cbs,
                                                                   Mat<E> xm, int64_t xbs, Mat<E> z, int64_t zbs, int64_t *__restrict__ row_ind,
                                                                   int64_t *__restrict__ col_ind, int64_t *__restrict__ ranks, E *__restrict__ ws) {
    using R = real_t<E>;
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const int m = (int)a.rows, n = (int)a.cols, mn = m > n ? m : n;
    const int ldw = IN_LDS ? (m | 1) : m;
    E *lds = reinterpret_cast<E *>(smem_raw);
    E *W = IN_LDS ? lds : ws + (size_t)blockIdx.x * (size_t)m * (size_t)n;
    const BidLds<E> o = bid_carve(lds + (IN_LDS ? bts_w_elems(m, n, k) : 0), mn, n);
    E(*tile)[z_tile<E> + 1] = o.tile;
    R *vn1 = o.vn1, *vn2 = o.vn2, *red = o.red;
    int *jp = o.jp;    // phase 1's column permutation: read until X is gathered
    int *jp2 = o.jp2;  // phase 2's row permutation
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;

    for (int b = blockIdx.x; b < count; b += gridDim.x) {
        const E *__restrict__ A = a.p + (int64_t)b * abs;
        // ---- phase 1: column ID of A -> r (= Z), col_ind, the rank --------------------------------------------------
        bid_load_pow2(W, ldw, m, n, a.rs <= a.cs, [&](int i, int c) { return A[i * a.rs + c * a.cs]; }, vn1, vn2, jp, red + 4, wv, lane);
        const int r = bid_qrcp(W, ldw, m, n, k, tol, jp, vn1, vn2, red, tid, wv, lane);
        for (int p = tid; p < n; p += BID_THREADS) col_ind[(int64_t)b * n + p] = jp[p];
        if (tid == 0) ranks[b] = r;
        bid_z(W, ldw, n, r, k, jp, tile, z.p + (int64_t)b * zbs, z.rs, z.cs, tid);
        __syncthreads();  // W and the norms are phase 2's from here

        // ---- phase 2: column ID of C^H (r x m), W2[p][i] = conj(A[p, col_ind[i]]) -> c = Z2^H, row_ind ------------------
        const int ldw2 = IN_LDS ? (r | 1) : r;
        bid_load_pow2(W, ldw2, r, m, a.cs < a.rs, [&](int i, int p) { return cj(A[p * a.rs + jp[i] * a.cs]); }, vn1, vn2, jp2, red + 4, wv, lane);
        const int r2 = bid_qrcp(W, ldw2, r, m, r, 0.0, jp2, vn1, vn2, red, tid, wv, lane);  // r2 < r only on an exactly zero pivot
        for (int p = tid; p < m; p += BID_THREADS) row_ind[(int64_t)b * m + p] = jp2[p];
        bid_z<E, true>(W, ldw2, m, r2, k, jp2, tile, cm.p + (int64_t)b * cbs, cm.cs, cm.rs, tid);  // Z2^H (m x k) through c's transposed view

        // ---- X = A[row_ind[:r], col_ind[:r]], rows and columns r..k-1 zero --------------------------------------------------
        E *Xb = xm.p + (int64_t)b * xbs;
        for (int j = wv; j < k; j += BID_WAVES) {
            const E *src = A + (int64_t)jp[j] * a.cs;
            for (int i = lane; i < k; i += 64) Xb[i * xm.rs + j * xm.cs] = (i < r && j < r) ? src[jp2[i] * a.rs] : elem<E>::zero();
        }
        __syncthreads();  // W, jp, jp2 and the norms are rewritten by the next matrix
    }
}

// their plans (rc_batched_launch.hpp): the working copy W (m x n) in LDS when it fits next to the small arrays, else in the workgroup's
// slot of the grid-bounded workspace; the two-sided ID chooses from the larger need of its two phases
template <typename E>
BatchedPlan<bool> bid_plan(int m, int n) {
    return batched_lds_or_ws([&](bool w_lds) { return bid_lds_bytes<E>(w_lds ? (size_t)n * (size_t)(m | 1) : 0, n, n, 0); },
                             (size_t)m * (size_t)n * sizeof(E), "column_id_rank_batched");
}
template <typename E>
BatchedPlan<bool> bts_plan(int m, int n, int k) {
    return batched_lds_or_ws([&](bool w_lds) { return bid_lds_bytes<E>(w_lds ? bts_w_elems(m, n, k) : 0, std::max(m, n), n, m); },
                             (size_t)m * (size_t)n * sizeof(E), "two_sided_id_rank_batched");
}

// (the bodies of their launchers: batched_launchers.hpp)

// ---- the Jacobi sweep schedule of the SVD and recompression kernels ---------------------------------------------------------------------
// one-sided Jacobi of the N x N core G (columns ldg apart) with the rotations accumulated in J (ldj); round-robin pairs, 16 lanes per pair (N <= 16 NE
// rows per lane), the 16 groups of the workgroup walk the N / 2 pair slots of a round; the round on one pair is the family's own (bsv_round /
// bsc_round).  Returns false when kMaxSweeps ran out before a quiet sweep.
template <typename E, int NE>
__device__ __forceinline__ bool bsv_jacobi(E *G, int ldg, E *J, int ldj, int N, int tid, int *flag) {
    using R = real_t<E>;
    const int ll = tid & 15, grp = tid >> 4;
    constexpr int NGRP = BID_THREADS / 16;
    const int N2 = (N + 1) & ~1, npairs = N2 / 2;
    const R tol = sqrt((R)N) * num<R>::eps(), tol2 = tol * tol;
    for (int sweep = 0; sweep < kMaxSweeps; ++sweep) {
        if (tid == 0) *flag = 0;
        __syncthreads();
        for (int r = 0; r < N2 - 1; ++r) {
            for (int pi = grp; pi < npairs; pi += NGRP) {
                int p, q;
                rr_pair(N2, r, pi, p, q);
                if (q < N) {  // q == N: the dummy column of an odd N
                    if constexpr (is_real_elem<E>) bsv_round<E, NE>(G, ldg, J, ldj, N, p, q, tol, tol2, ll, flag);
                    else bsc_round<R, NE>(G, ldg, J, ldj, N, p, q, tol, tol2, ll, flag);
                }
            }
            __syncthreads();  // the pairs of a round are disjoint; the next round re-pairs the columns
        }
        const int rotated = *flag;
        __syncthreads();
        if (rotated < 2) return true;
    }
    return false;
}

// ---- the exponent of an operand of the recompressions --------------------------------------------------------------------------------------
// The exponent of an operand before it is loaded (block_pow2_exponent over at(i, c), i < rows, c < q, read as bid_fill reads it; for complex
// elements over the larger of the two parts): the loads multiply every entry by 2^-e, so that the norms, both cores and the Jacobi run at
// unit scale as in k_batched_svd, and the singular values take 2^(eL + eM + eS + eR) back, one exponent per operand (left, mid, s, right).
// One more read of the operand (the second one hits L2); with e = 0 (a zero or non-finite operand) every entry is multiplied by 1 and the
// bits are the unscaled ones.  stage: four elements no thread reads before the next barrier.
template <typename R, typename At>
__device__ __forceinline__ int brc_exponent(int rows, int q, bool lanes_on_rows, At at, R *stage, int wv, int lane) {
    R mx = 0;
    if (lanes_on_rows) {
        for (int c = wv; c < q; c += BID_WAVES)
            for (int i = lane; i < rows; i += 64) mx = max(mx, pow2_key_max(at(i, c)));
    } else {
        // lanes along c: a wave takes 64 / qs rows per pass, qs the power of two >= min(q, 64), so that a narrow factor keeps every lane
        // loading (a maximum does not depend on the order it is taken in)
        int qs = 1;
        while (qs < q && qs < 64) qs <<= 1;
        const int rpw = 64 / qs, lr = lane / qs, lc = lane - lr * qs;
#pragma unroll 4
        for (int i = wv * rpw + lr; i < rows; i += BID_WAVES * rpw)
            for (int c = lc; c < q; c += qs) mx = max(mx, pow2_key_max(at(i, c)));
    }
    return __builtin_amdgcn_readfirstlane(block_pow2_exponent(mx, stage, wv, lane));  // uniform by construction: kept in a scalar register
}

// ---- the stack load of the tall recompressions --------------------------------------------------------------------------------------------
// one stage's stack into W (pitch ldw, hs rows): rows 0 .. top - 1 of position p's column are R[0 .. p, p] of the previous stage's copy Wp
// (the same pitch and physical columns) and zeros, rows top .. hs - 1 are at(i - top, c); then the real column norms by position (bid_norms'
// sums) with jp kept as it is.  top == 0 (stage 0): Wp is not read, and with jp the identity this is bid_load.
template <typename E, typename At>
__device__ __forceinline__ void brt_stack_load(E *W, int ldw, const E *Wp, int top, int hs, int q, bool lanes_on_rows, At at, real_t<E> *vn1, real_t<E> *vn2,
                                               const int *jp, int wv, int lane) {
    using R = real_t<E>;
    if (top) {
        for (int p = wv; p < q; p += BID_WAVES) {
            const size_t col = (size_t)jp[p] * ldw;
            for (int i = lane; i < top; i += 64) W[col + i] = i <= p ? Wp[col + i] : elem<E>::zero();
        }
    }
    const int rows = hs - top;
    if (lanes_on_rows) {
        for (int c = wv; c < q; c += BID_WAVES)
            for (int i = lane; i < rows; i += 64) W[(size_t)c * ldw + top + i] = at(i, c);
    } else {
        for (int i = wv; i < rows; i += BID_WAVES)
            for (int c = lane; c < q; c += 64) W[(size_t)c * ldw + top + i] = at(i, c);
    }
    __syncthreads();
    for (int p = wv; p < q; p += BID_WAVES) {
        const E *col = W + (size_t)jp[p] * ldw;
        R acc = 0;
        for (int i = lane; i < hs; i += 64) acc += abs2(col[i]);
        acc = wave_sum_dpp(acc);
        if (lane == 0) { const R nr = sqrt(acc); vn1[p] = nr; vn2[p] = nr; }
    }
    __syncthreads();
}

}  // namespace

}  // namespace rc
