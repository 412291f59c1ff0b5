// Batched column and two-sided IDs of many small same-shaped COMPLEX matrices in one launch (rc_column_id_rank_batched_c64 / _c32,
// rc_two_sided_id_rank_batched_c64 / _c32).
//
// The structure of kernels_batched_id.hip (one persistent workgroup of 256 threads per matrix, the same three device stages, the same
// grid and workspace rule, bid_grid) with the complex arithmetic of the lone complex path in rc_complex.hip:
//   * interleaved (re, im) data (rc_complex.hip's cplx<R>); the partial norms vn1 / vn2 are real, W and the tile complex;
//   * ?larfg for complex (k_c_qr_pivot_reflect): beta = -copysign(lapy3(alpha.re, alpha.im, xnorm), alpha.re) is real, tau complex,
//     the scale 1 / (alpha - beta) by Smith division; H = I only when xnorm == 0 and alpha.im == 0;
//   * H^H = I - conj(tau) v v^H with the conjugated dot v^H x, then the ?laqp2 down-date with |x_j| (k_c_qr_apply);
//   * pivots: first maximum of the real partial norms; the rank rule on the real R_jj = beta;
//   * Z = [I | R11^-1 R12] P^T by back substitution with complex division (k_c_trsm_upper).
// The two-sided row side mirrors rc_column_id_two_sided_c* (c_pivoted_lq -> c_lq_row_id): phase 2 factors C^H, C = A[:, col_ind[:r]]
// loaded with conjugation, and writes c[:, :r] = Z2^H; X = A[row_ind[:r], col_ind[:r]] is gathered from A.
//
// Register budget (every instance must run without scratch): one trailing column in flight per wave in the apply (the real kernels
// keep two) and 8 x 8 back-substitution tiles (the real kernels use 16 x 16).
//
// Every operation below commutes exactly with negating all imaginary parts (round to nearest is sign-symmetric, and each real part
// is even, each imaginary part odd in the imaginary inputs), so conj(A) gives the same permutations and ranks and the conjugate
// of every factor, bit for bit.
#include "rc_common.hpp"
#include "rc_device.hpp"

namespace rc {

namespace {

constexpr int BIC_THREADS = 256;
constexpr int BIC_WAVES = BIC_THREADS / 64;
constexpr int BIC_NB = 8;  // back-substitution tile

template <typename R>
struct cx {
    R re, im;
};
template <typename R> __device__ __forceinline__ cx<R> cmul(cx<R> a, cx<R> b) { return {a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re}; }
template <typename R> __device__ __forceinline__ cx<R> csub(cx<R> a, cx<R> b) { return {a.re - b.re, a.im - b.im}; }
template <typename R> __device__ __forceinline__ cx<R> conj_of(cx<R> a) { return {a.re, -a.im}; }
template <typename R> __device__ __forceinline__ R abs2(cx<R> a) { return a.re * a.re + a.im * a.im; }
template <typename R> __device__ __forceinline__ cx<R> cdiv(cx<R> a, cx<R> b) {  // Smith's algorithm (?ladiv), rc_complex.hip's
    if (fabs(b.re) >= fabs(b.im)) {
        const R r = b.im / b.re, d = b.re + b.im * r;
        return {(a.re + a.im * r) / d, (a.im - a.re * r) / d};
    }
    const R r = b.re / b.im, d = b.im + b.re * r;
    return {(a.re * r + a.im) / d, (a.im * r - a.re) / d};
}
template <typename R> __device__ __forceinline__ cx<R> czero() { return {(R)0, (R)0}; }
template <typename R> __device__ __forceinline__ cx<R> cone() { return {(R)1, (R)0}; }

// strided complex view (the rc_matrix of an interleaved-complex operand, strides in complex elements)
template <typename R>
struct CView {
    cx<R> *p;
    int64_t rows, cols, rs, cs;
};
template <typename R>
CView<R> cview(const rc_matrix &m) { return CView<R>{static_cast<cx<R> *>(m.data), m.rows, m.cols, m.row_stride, m.col_stride}; }

// dynamic LDS: [W: m x ldw complex, LDS variant only] tile[8 x 9] complex | vn1[n] vn2[n] red[8] real | jp[n]
template <typename R>
size_t bic_lds_bytes(int m, int n, bool in_lds) {
    size_t c = (size_t)BIC_NB * (BIC_NB + 1);
    if (in_lds) c += (size_t)n * (size_t)(m | 1);
    return c * sizeof(cx<R>) + ((size_t)2 * n + 8) * sizeof(R) + (size_t)n * sizeof(int);
}

// H_j^H = I - conj(tau) v v^H applied to the trailing columns p = j+1 .. n-1, one wave per column; rows j + lane + 64 e of the column
// in registers (NE * 64 >= m - j), then the ?laqp2 down-date of the column's partial norm with |x_j|
template <typename R, int NE>
__device__ __forceinline__ void bic_apply(cx<R> *W, int ldw, int m, int n, int j, const int *jp, R *vn1, R *vn2, cx<R> tj, int wv, int lane) {
    const int mrem = m - j;
    const cx<R> *vc = W + (size_t)jp[j] * ldw + j;
    cx<R> v[NE];
#pragma unroll
    for (int e = 0; e < NE; ++e) {
        // branch-free: lanes past the end read row j (always valid) and are masked by a select
        const int li = lane + 64 * e;
        const bool ok = li < mrem;
        const cx<R> vv = vc[ok ? li : 0];
        v[e] = ok ? (li == 0 ? cone<R>() : vv) : czero<R>();
    }
    const bool reflect = tj.re != (R)0 || tj.im != (R)0;  // tau == 0: H = I
    const cx<R> ctj = conj_of(tj);
    for (int p = j + 1 + wv; p < n; p += BIC_WAVES) {
        cx<R> *xc = W + (size_t)jp[p] * ldw + j;
        cx<R> x[NE];
#pragma unroll
        for (int e = 0; e < NE; ++e) {
            const int li = lane + 64 * e;
            const bool ok = li < mrem;
            const cx<R> xv = xc[ok ? li : 0];
            x[e] = ok ? xv : czero<R>();
        }
        if (reflect) {
            R dre = 0, dim = 0;  // v^H x
#pragma unroll
            for (int e = 0; e < NE; ++e) {
                dre = fma(v[e].re, x[e].re, dre);
                dre = fma(v[e].im, x[e].im, dre);
                dim = fma(v[e].re, x[e].im, dim);
                dim = fma(-v[e].im, x[e].re, dim);
            }
            const cx<R> f = cmul(ctj, cx<R>{wave_sum_dpp(dre), wave_sum_dpp(dim)});
#pragma unroll
            for (int e = 0; e < NE; ++e) {
                const int li = lane + 64 * e;
                x[e].re = fma(-f.re, v[e].re, x[e].re);  // v is zero out of range
                x[e].re = fma(f.im, v[e].im, x[e].re);
                x[e].im = fma(-f.re, v[e].im, x[e].im);
                x[e].im = fma(-f.im, v[e].re, x[e].im);
                if (li < mrem) xc[li] = x[e];
            }
        }
        const R vn = vn1[p];
        if (vn != (R)0) {
            R nn;
            const cx<R> x0{read_lane(x[0].re, 0), read_lane(x[0].im, 0)};
            if (laqp2_downdate(vn, vn2[p], (R)hypot(x0.re, x0.im), &nn)) {
                R ss = 0;
#pragma unroll
                for (int e = 0; e < NE; ++e) {
                    const int li = lane + 64 * e;
                    if (li > 0 && li < mrem) ss += abs2(x[e]);
                }
                ss = wave_sum_dpp(ss);
                if (lane == 0) { nn = (j < m - 1) ? sqrt(ss) : (R)0; vn1[p] = nn; vn2[p] = nn; }
            } else if (lane == 0) {
                vn1[p] = nn;
            }
        }
    }
}

// ---- the three stages of one factorization, shared by k_batched_id_c and both phases of k_batched_two_sided_c -----------------------
// (m x n below is the matrix being factored: A for a column ID, C^H for the row side of a two-sided ID)

// working copy W[c * ldw + i] = at(i, c), read with the lanes along i (lanes_on_rows) or along c (the input's fast direction),
// then the initial (real) column norms and the identity permutation
template <typename R, typename At>
__device__ __forceinline__ void bic_load(cx<R> *W, int ldw, int m, int n, bool lanes_on_rows, At at, R *vn1, R *vn2, int *jp, int wv, int lane) {
    if (lanes_on_rows) {
        for (int c = wv; c < n; c += BIC_WAVES)
            for (int i = lane; i < m; i += 64) W[(size_t)c * ldw + i] = at(i, c);
    } else {
        for (int i = wv; i < m; i += BIC_WAVES)
            for (int c = lane; c < n; c += 64) W[(size_t)c * ldw + i] = at(i, c);
    }
    __syncthreads();
    for (int c = wv; c < n; c += BIC_WAVES) {
        R acc = 0;
        for (int i = lane; i < m; i += 64) acc += abs2(W[(size_t)c * ldw + i]);
        acc = wave_sum_dpp(acc);
        if (lane == 0) { const R nr = sqrt(acc); vn1[c] = nr; vn2[c] = nr; jp[c] = c; }
    }
    __syncthreads();
}

// truncated pivoted QR of the working copy, at most k steps: pivots in jp (?geqp3's rule), R and the Householder vectors in W (LAPACK
// format, physical column order).  Returns the rank: the first j < k with R_jj == 0 or (tol > 0 and |R_jj / R_00| < tol), else k.
template <typename R>
__device__ __forceinline__ int bic_qrcp(cx<R> *W, int ldw, int m, int n, int k, double tol, int *jp, R *vn1, R *vn2, R *red, int tid, int wv, int lane) {
    int r = k;
    R r00 = 0;
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
            if (lane == 0 && pvt != j) {  // zlaqp2: swap the indices, carry the norms of position j to pvt
                const int t = jp[pvt]; jp[pvt] = jp[j]; jp[j] = t;
                vn1[pvt] = vn1[j];
                vn2[pvt] = vn2[j];
            }
        }
        __syncthreads();
        // ?larfg for complex on column jp[j], rows j..m-1 (k_c_qr_pivot_reflect's formula)
        cx<R> *col = W + (size_t)jp[j] * ldw;
        const cx<R> alpha = col[j];
        R acc = 0;
        for (int i = j + 1 + tid; i < m; i += BIC_THREADS) acc += abs2(col[i]);
        acc = wave_sum_dpp(acc);
        if (lane == 0) red[wv] = acc;
        __syncthreads();  // also orders every thread's read of alpha before the write of beta below
        const R ssq = (red[0] + red[1]) + (red[2] + red[3]);
        const R xnorm = sqrt(ssq);
        R beta = alpha.re;
        cx<R> tj = czero<R>();
        if (xnorm != (R)0 || alpha.im != (R)0) {
            beta = -copysign(sqrt(alpha.re * alpha.re + alpha.im * alpha.im + ssq), alpha.re);  // ?lapy3
            const cx<R> scal = cdiv(cone<R>(), cx<R>{alpha.re - beta, alpha.im});
            for (int i = j + 1 + tid; i < m; i += BIC_THREADS) col[i] = cmul(col[i], scal);
            tj = cx<R>{(beta - alpha.re) / beta, -alpha.im / beta};
            if (tid == 0) col[j] = cx<R>{beta, (R)0};
        }
        // R_jj = beta (real) decides the rank (qr.rs:187-200 as a ratio; uniform across the workgroup)
        if (j == 0) r00 = beta;
        if (beta == (R)0 || (tol > 0.0 && (double)fabs(beta / r00) < tol)) { r = j; break; }
        __syncthreads();
        if (j + 1 < n) {
            const int rem = m - j;
            if (rem <= 128) bic_apply<R, 2>(W, ldw, m, n, j, jp, vn1, vn2, tj, wv, lane);
            else if (rem <= 256) bic_apply<R, 4>(W, ldw, m, n, j, jp, vn1, vn2, tj, wv, lane);
            else bic_apply<R, 8>(W, ldw, m, n, j, jp, vn1, vn2, tj, wv, lane);
        }
        __syncthreads();
    }
    __syncthreads();
    return r;
}

// Z = [I | R11^-1 R12] P^T (k x n, rows r..k-1 zero) into Zb[i * zrs + c * zcs], or its conjugate when CONJ (the row side's Z2^H):
// blocked back substitution with k -> r (8 x 8 tiles of R11 staged in LDS, one thread per right-hand side, complex division on the
// diagonal), each column written straight to its final place
template <typename R, bool CONJ>
__device__ __forceinline__ void bic_z(const cx<R> *W, int ldw, int n, int r, int k, const int *jp, cx<R> (*tile)[BIC_NB + 1], cx<R> *Zb, int64_t zrs,
                                      int64_t zcs, int tid) {
    const int nblk = (r + BIC_NB - 1) / BIC_NB;
    const int ti = tid / BIC_NB, tk = tid % BIC_NB;
    auto out = [](cx<R> v) { return CONJ ? conj_of(v) : v; };  // its own inverse
    for (int q0 = 0; q0 < n; q0 += BIC_THREADS) {
        const int p = q0 + tid;  // position in the pivoted order
        const bool inside = p < n;
        const int dc = inside ? jp[p] : 0;  // where column p of [I | R11^-1 R12] goes
        const bool active = inside && p >= r;
        cx<R> *zc = Zb + (int64_t)dc * zcs;
        if (inside) {
            if (p < r)
                for (int i = 0; i < k; ++i) zc[i * zrs] = (i == p) ? cone<R>() : czero<R>();
            else
                for (int i = r; i < k; ++i) zc[i * zrs] = czero<R>();
        }
        const cx<R> *bcol = W + (size_t)dc * ldw;  // R12[:, p]: rows 0 .. r-1 of the physical column
        for (int bi = nblk - 1; bi >= 0; --bi) {
            const int r0 = bi * BIC_NB;
            cx<R> acc[BIC_NB];
#pragma unroll
            for (int ii = 0; ii < BIC_NB; ++ii) acc[ii] = (active && r0 + ii < r) ? bcol[r0 + ii] : czero<R>();
            for (int bj = nblk - 1; bj >= bi; --bj) {
                const int c0 = bj * BIC_NB;
                __syncthreads();
                if (ti < BIC_NB) {
                    const int i = r0 + ti, l = c0 + tk;
                    tile[ti][tk] = (i < r && l < r && i <= l) ? W[(size_t)jp[l] * ldw + i] : czero<R>();
                }
                __syncthreads();
                if (bj > bi) {
                    cx<R> x[BIC_NB];
#pragma unroll
                    for (int jj = 0; jj < BIC_NB; ++jj) x[jj] = (active && c0 + jj < r) ? out(zc[(c0 + jj) * zrs]) : czero<R>();  // own finished block
#pragma unroll
                    for (int jj = 0; jj < BIC_NB; ++jj)
#pragma unroll
                        for (int ii = 0; ii < BIC_NB; ++ii) acc[ii] = csub(acc[ii], cmul(tile[ii][jj], x[jj]));
                } else {
#pragma unroll
                    for (int ii = BIC_NB - 1; ii >= 0; --ii) {
                        if (r0 + ii < r) {
                            acc[ii] = cdiv(acc[ii], tile[ii][ii]);
#pragma unroll
                            for (int i2 = 0; i2 < ii; ++i2) acc[i2] = csub(acc[i2], cmul(tile[i2][ii], acc[ii]));
                        }
                    }
                }
            }
            if (active) {
#pragma unroll
                for (int ii = 0; ii < BIC_NB; ++ii)
                    if (r0 + ii < r) zc[(r0 + ii) * zrs] = out(acc[ii]);
            }
        }
    }
}

template <typename R, bool IN_LDS>
__global__ __launch_bounds__(BIC_THREADS) void k_batched_id_c(CView<R> a, int64_t abs, int count, int k, double tol, CView<R> cm, int64_t cbs,
                                                              CView<R> z, int64_t zbs, int64_t *__restrict__ col_ind, int64_t *__restrict__ ranks,
                                                              cx<R> *__restrict__ ws) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const int m = (int)a.rows, n = (int)a.cols;
    const int ldw = IN_LDS ? (m | 1) : m;
    cx<R> *lds = reinterpret_cast<cx<R> *>(smem_raw);
    cx<R> *W = IN_LDS ? lds : ws + (size_t)blockIdx.x * (size_t)m * (size_t)n;
    cx<R>(*tile)[BIC_NB + 1] = reinterpret_cast<cx<R>(*)[BIC_NB + 1]>(lds + (IN_LDS ? (size_t)n * ldw : 0));
    R *vn1 = reinterpret_cast<R *>(lds + (IN_LDS ? (size_t)n * ldw : 0) + BIC_NB * (BIC_NB + 1));
    R *vn2 = vn1 + n;
    R *red = vn2 + n;
    int *jp = reinterpret_cast<int *>(red + 8);
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;

    for (int b = blockIdx.x; b < count; b += gridDim.x) {
        const cx<R> *__restrict__ A = a.p + (int64_t)b * abs;
        bic_load(W, ldw, m, n, a.rs <= a.cs, [&](int i, int c) { return A[i * a.rs + c * a.cs]; }, vn1, vn2, jp, wv, lane);
        const int r = bic_qrcp(W, ldw, m, n, k, tol, jp, vn1, vn2, red, tid, wv, lane);

        // ---- outputs: permutation, rank, C, Z -------------------------------------------------------------------
        for (int p = tid; p < n; p += BIC_THREADS) col_ind[(int64_t)b * n + p] = jp[p];
        if (tid == 0) ranks[b] = r;
        cx<R> *Cb = cm.p + (int64_t)b * cbs;
        for (int j = wv; j < k; j += BIC_WAVES) {
            const cx<R> *src = A + (int64_t)jp[j] * a.cs;
            for (int i = lane; i < m; i += 64) Cb[i * cm.rs + j * cm.cs] = j < r ? src[i * a.rs] : czero<R>();
        }
        bic_z<R, false>(W, ldw, n, r, k, jp, tile, z.p + (int64_t)b * zbs, z.rs, z.cs, tid);
        __syncthreads();  // W, jp and the norms are rewritten by the next matrix
    }
}

// dynamic LDS of the two-sided kernel: [W: the larger of phase 1's n x (m|1) and phase 2's m x (k|1), LDS variant only] tile[8 x 9]
// complex | vn1[max(m, n)] vn2[max(m, n)] red[8] real | jp[n] jp2[m]
__host__ __device__ inline size_t btc_w_elems(int m, int n, int k) {
    const size_t w1 = (size_t)n * (size_t)(m | 1), w2 = (size_t)m * (size_t)(k | 1);
    return w1 > w2 ? w1 : w2;
}
template <typename R>
size_t btc_lds_bytes(int m, int n, int k, bool in_lds) {
    size_t c = (size_t)BIC_NB * (BIC_NB + 1);
    if (in_lds) c += btc_w_elems(m, n, k);
    return c * sizeof(cx<R>) + ((size_t)2 * std::max(m, n) + 8) * sizeof(R) + (size_t)(m + n) * sizeof(int);
}

// Two-sided ID A ~ C X R per matrix: phase 1 is k_batched_id_c's column ID (R = its Z, col_ind, the rank r); phase 2 is the column
// ID of C^H = conj(A[:, col_ind[:r]])^T (r x m) at rank r with tol = 0, by the same three stages: its permutation is row_ind and its
// Z, conjugated and written through c's transposed view, is c = Z2^H; X = A[row_ind[:r], col_ind[:r]] is gathered from the input.
template <typename R, bool IN_LDS>
__global__ __launch_bounds__(BIC_THREADS) void k_batched_two_sided_c(CView<R> a, int64_t abs, int count, int k, double tol, CView<R> cm, int64_t cbs,
                                                                     CView<R> xm, int64_t xbs, CView<R> z, int64_t zbs, int64_t *__restrict__ row_ind,
                                                                     int64_t *__restrict__ col_ind, int64_t *__restrict__ ranks, cx<R> *__restrict__ ws) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const int m = (int)a.rows, n = (int)a.cols, mn = m > n ? m : n;
    const int ldw = IN_LDS ? (m | 1) : m;
    cx<R> *lds = reinterpret_cast<cx<R> *>(smem_raw);
    cx<R> *W = IN_LDS ? lds : ws + (size_t)blockIdx.x * (size_t)m * (size_t)n;
    cx<R>(*tile)[BIC_NB + 1] = reinterpret_cast<cx<R>(*)[BIC_NB + 1]>(lds + (IN_LDS ? btc_w_elems(m, n, k) : 0));
    R *vn1 = reinterpret_cast<R *>(lds + (IN_LDS ? btc_w_elems(m, n, k) : 0) + BIC_NB * (BIC_NB + 1));
    R *vn2 = vn1 + mn;
    R *red = vn2 + mn;
    int *jp = reinterpret_cast<int *>(red + 8);  // phase 1's column permutation: read until X is gathered
    int *jp2 = jp + n;                           // phase 2's row permutation
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;

    for (int b = blockIdx.x; b < count; b += gridDim.x) {
        const cx<R> *__restrict__ A = a.p + (int64_t)b * abs;
        // ---- phase 1: column ID of A -> r (= Z), col_ind, the rank --------------------------------------------------
        bic_load(W, ldw, m, n, a.rs <= a.cs, [&](int i, int c) { return A[i * a.rs + c * a.cs]; }, vn1, vn2, jp, wv, lane);
        const int r = bic_qrcp(W, ldw, m, n, k, tol, jp, vn1, vn2, red, tid, wv, lane);
        for (int p = tid; p < n; p += BIC_THREADS) col_ind[(int64_t)b * n + p] = jp[p];
        if (tid == 0) ranks[b] = r;
        bic_z<R, false>(W, ldw, n, r, k, jp, tile, z.p + (int64_t)b * zbs, z.rs, z.cs, tid);
        __syncthreads();  // W and the norms are phase 2's from here

        // ---- phase 2: column ID of C^H (r x m), W2[p][i] = conj(A[p, col_ind[i]]) -> c = Z2^H, row_ind ------------------
        const int ldw2 = IN_LDS ? (r | 1) : r;
        bic_load(W, ldw2, r, m, a.cs < a.rs, [&](int i, int p) { return conj_of(A[p * a.rs + jp[i] * a.cs]); }, vn1, vn2, jp2, wv, lane);
        const int r2 = bic_qrcp(W, ldw2, r, m, r, 0.0, jp2, vn1, vn2, red, tid, wv, lane);  // r2 < r only on an exactly zero pivot
        for (int p = tid; p < m; p += BIC_THREADS) row_ind[(int64_t)b * m + p] = jp2[p];
        bic_z<R, true>(W, ldw2, m, r2, k, jp2, tile, cm.p + (int64_t)b * cbs, cm.cs, cm.rs, tid);  // Z2^H (m x k) through c's transposed view

        // ---- X = A[row_ind[:r], col_ind[:r]], rows and columns r..k-1 zero --------------------------------------------------
        cx<R> *Xb = xm.p + (int64_t)b * xbs;
        for (int j = wv; j < k; j += BIC_WAVES) {
            const cx<R> *src = A + (int64_t)jp[j] * a.cs;
            for (int i = lane; i < k; i += 64) Xb[i * xm.rs + j * xm.cs] = (i < r && j < r) ? src[jp2[i] * a.rs] : czero<R>();
        }
        __syncthreads();  // W, jp, jp2 and the norms are rewritten by the next matrix
    }
}

}  // namespace

// the real kernels' launch rule (bid_grid, BID_MAX_LDS): LDS variant when the complex working copy fits, else the workspace variant
template <typename R>
void batched_column_id_c(rc_context *c, const rc_matrix &a_, int64_t abs, int32_t count, int64_t k, double tol, const rc_matrix &cm_, int64_t cbs,
                         const rc_matrix &z_, int64_t zbs, int64_t *col_ind, int64_t *ranks) {
    const CView<R> a = cview<R>(a_), cm = cview<R>(cm_), z = cview<R>(z_);
    const int m = (int)a.rows, n = (int)a.cols;
    if (count <= 0) return;
    ProfScope ps(c, "op:batched_column_id<complex> %dx%d k=%lld count=%d", m, n, (long long)k, (int)count);
    const size_t lds_in = bic_lds_bytes<R>(m, n, true);
    const bool in_lds = lds_in <= BID_MAX_LDS;
    const size_t lds = in_lds ? lds_in : bic_lds_bytes<R>(m, n, false);
    auto kern = in_lds ? k_batched_id_c<R, true> : k_batched_id_c<R, false>;
    static bool attr_set[64] = {};
    if (!attr_set[c->device & 63]) {
        RC_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(k_batched_id_c<R, true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)BID_MAX_LDS));
        RC_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(k_batched_id_c<R, false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)BID_MAX_LDS));
        attr_set[c->device & 63] = true;
    }
    const size_t per = (size_t)m * (size_t)n * sizeof(cx<R>);
    const int64_t grid = bid_grid(c, reinterpret_cast<const void *>(kern), lds, in_lds ? 0 : per, count);
    cx<R> *ws = in_lds ? nullptr : c->alloc<cx<R>>((size_t)grid * (size_t)m * (size_t)n);
    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(BIC_THREADS), lds, c->stream, a, abs, (int)count, (int)k, tol, cm, cbs, z, zbs, col_ind, ranks, ws);
}

template <typename R>
void batched_two_sided_id_c(rc_context *c, const rc_matrix &a_, int64_t abs, int32_t count, int64_t k, double tol, const rc_matrix &cm_, int64_t cbs,
                            const rc_matrix &x_, int64_t xbs, const rc_matrix &z_, int64_t zbs, int64_t *row_ind, int64_t *col_ind, int64_t *ranks) {
    const CView<R> a = cview<R>(a_), cm = cview<R>(cm_), x = cview<R>(x_), z = cview<R>(z_);
    const int m = (int)a.rows, n = (int)a.cols;
    if (count <= 0) return;
    ProfScope ps(c, "op:batched_two_sided_id<complex> %dx%d k=%lld count=%d", m, n, (long long)k, (int)count);
    const size_t lds_in = btc_lds_bytes<R>(m, n, (int)k, true);
    const bool in_lds = lds_in <= BID_MAX_LDS;
    const size_t lds = in_lds ? lds_in : btc_lds_bytes<R>(m, n, (int)k, false);
    auto kern = in_lds ? k_batched_two_sided_c<R, true> : k_batched_two_sided_c<R, false>;
    static bool attr_set[64] = {};
    if (!attr_set[c->device & 63]) {
        RC_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(k_batched_two_sided_c<R, true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)BID_MAX_LDS));
        RC_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(k_batched_two_sided_c<R, false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)BID_MAX_LDS));
        attr_set[c->device & 63] = true;
    }
    const size_t per = (size_t)m * (size_t)n * sizeof(cx<R>);
    const int64_t grid = bid_grid(c, reinterpret_cast<const void *>(kern), lds, in_lds ? 0 : per, count);
    cx<R> *ws = in_lds ? nullptr : c->alloc<cx<R>>((size_t)grid * (size_t)m * (size_t)n);
    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(BIC_THREADS), lds, c->stream, a, abs, (int)count, (int)k, tol, cm, cbs, x, xbs, z, zbs, row_ind,
                       col_ind, ranks, ws);
}

template void batched_column_id_c<double>(rc_context *, const rc_matrix &, int64_t, int32_t, int64_t, double, const rc_matrix &, int64_t, const rc_matrix &,
                                          int64_t, int64_t *, int64_t *);
template void batched_column_id_c<float>(rc_context *, const rc_matrix &, int64_t, int32_t, int64_t, double, const rc_matrix &, int64_t, const rc_matrix &,
                                         int64_t, int64_t *, int64_t *);
template void batched_two_sided_id_c<double>(rc_context *, const rc_matrix &, int64_t, int32_t, int64_t, double, const rc_matrix &, int64_t,
                                             const rc_matrix &, int64_t, const rc_matrix &, int64_t, int64_t *, int64_t *, int64_t *);
template void batched_two_sided_id_c<float>(rc_context *, const rc_matrix &, int64_t, int32_t, int64_t, double, const rc_matrix &, int64_t,
                                            const rc_matrix &, int64_t, const rc_matrix &, int64_t, int64_t *, int64_t *, int64_t *);

}  // namespace rc
