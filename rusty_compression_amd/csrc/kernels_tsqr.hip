// Communication-avoiding QR / pivoted QR of TALL-SKINNY matrices (m >> n, n <= ~138 f64)
// for gfx950.  Same results as the Householder chain of kernels_qr.hip (LAPACK ?geqp3 +
// ?orgqr semantics, including the SIGNS of R's diagonal), organised for MI355X:
//
//   Y (m x n)  --CholeskyQR2-->  Y = Q1 R1        three MFMA GEMMs per pass (Gram, apply R^-1),
//                                                  the n x n Cholesky + inverse in ONE workgroup's LDS
//   R1 (n x n) --Householder QRCP in LDS-->  R1 P = Q2 R     (?laqp2 semantics: first-max pivot,
//                                                  LAPACK norm down-dating / tol3z recompute)
//   Q = Q1 Q2  (one GEMM),  then the Householder sign convention of LAPACK is re-imposed:
//   the reflector representation of an orthonormal Q is unique, its signs d_j follow from an
//   LU-type elimination on Q's top k x k block (d_j = -sgn of the j-th pivot candidate), so
//   Q <- Q D, R <- D R reproduce ?geqp3/?orgqr exactly (tests: R to 1e-14 of LAPACK).
//
// Why: the m x n Householder chain needs ~2n dependent kernel launches that each stream the
// whole trailing matrix through single CUs (measured 3.2 ms for 8192 x 133); here the only
// serial parts act on n x n data inside one CU's LDS and everything O(m n^2) is a GEMM.
// CholeskyQR2 is only valid while cond(Y)^2 * eps < 1: k_chol_inv certifies its own result
// (positive pivots, ||Q1^T Q1 - I||_max small before the second pass) and raises a flag, on
// which the caller falls back to the Householder chain (rc_api.hip).
//
// Replaces: ?geqp3 + ?orgqr on sketches (/root/reference/src/pivoted_qr.rs:81-183 as called
// from src/random_sampling.rs:114) and the QR/LQ reduction inside ?gesdd (src/compute_svd.rs:19).
#include "rc_common.hpp"
#include "rc_device.hpp"
#include "rc_launch.hpp"

namespace rc {

// what stands in for a Cholesky pivot that is not positive (the failure is flagged; the arithmetic behind it stays finite)
template <typename T> __device__ inline T tiny_pivot();
template <> __device__ inline double tiny_pivot<double>() { return 1e-300; }
template <> __device__ inline float tiny_pivot<float>() { return 1e-30f; }

template <typename T>
__device__ inline T wave_sum64(T v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
template <typename T>
__device__ inline T row_sum16(T v) {  // sum over an aligned group of 16 lanes
#pragma unroll
    for (int off = 8; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// ---------------------------------------------------------------------------
// Cholesky G = R^T R (R upper) + R^{-1}, n x n in the LDS of one workgroup.
//   flag bit 0: non-positive pivot (G not numerically SPD)
//   flag bit 1: check_identity && max|G - I| > ident_tol  (first pass left Q1 too far from orthonormal)
// r1 (empty on the first pass of CholeskyQR2): the first pass's factor.  The second pass then leaves the factor of the whole
// matrix, r_out = R r1, instead of its own R: no caller wants R2 by itself, and the product was a GEMM and a reduction launch
// behind this kernel.  Each entry is one sum over the inner index, ascending from the diagonal of R to that of r1.
// FOLD says whether r1 is given: the first pass keeps the instance it had (its n dependent steps are a tenth of the chain).
// ---------------------------------------------------------------------------
template <typename T, int NT, bool FOLD>
__global__ __launch_bounds__(1024) void k_chol_inv(Mat<T> g, Mat<T> r_out, Mat<T> rinv_out, Mat<T> r1, int check_identity, T ident_tol, T skip_tol, int *flag) {
    // Register-tiled right-looking Cholesky: thread (ti, tc) of the 32 x 32 thread grid owns
    // the entries (ti + 32 a, tc + 32 b), a, b < NT, in registers; per step only pivot row j
    // goes through LDS (double buffered: ONE barrier per step).
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const int n = (int)g.rows;
    const int ld = n | 1;
    T *A = reinterpret_cast<T *>(smem_raw);  // A[i * ld + c], used by the inversion phase
    T *svec = A + (size_t)n * ld;            // n
    T *rowbuf = svec + n;                    // 2 * n
    T *red = rowbuf + 2 * n;                 // 16
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int ti = tid >> 5, tc = tid & 31;

    T reg[NT][NT];
    T dev = 0;
#pragma unroll
    for (int a = 0; a < NT; ++a)
#pragma unroll
        for (int b = 0; b < NT; ++b) {
            const int i = ti + 32 * a, c = tc + 32 * b;
            T v = 0;
            if (i < n && c < n) {
                v = g.at(i, c);
                dev = max(dev, fabs(v - ((i == c) ? (T)1 : (T)0)));
            }
            reg[a][b] = v;
        }
    // r1's upper triangle is fetched behind g, before anything waits for g, and parked in A (free until the loop below): if the
    // pass turns out to be the identity, r_out = I r1 is this copy, and neither its load nor its layout stands behind the decision
    // (only where the decision is taken: its barrier is what separates these writes from the loop's use of A)
    if constexpr (FOLD) {
        if (check_identity) {
#pragma unroll
            for (int a = 0; a < NT; ++a)
#pragma unroll
                for (int b = 0; b < NT; ++b) {
                    const int i = ti + 32 * a, c = tc + 32 * b;
                    if (i < n && c < n) A[i * ld + c] = c >= i ? r1.at(i, c) : (T)0;
                }
        }
    }
    if (check_identity) {
        dev = wave_max_dpp(dev);
        if (lane == 0) red[wv] = dev;
        __syncthreads();
        T mx = 0;
        for (int k = 0; k < 16; ++k) mx = max(mx, red[k]);
        if (tid == 0 && !(mx <= ident_tol)) atomicOr(flag, 2);
        // The first pass already delivered orthonormal columns to working accuracy (well-conditioned input:
        // max |Q1^T Q1 - I| <= skip_tol): the second pass would change nothing above that level, so R2 = R2^-1 = I
        // and the 2 n dependent column steps below are skipped (r_out = I r1 is r1's upper triangle, exactly).
        if (mx <= skip_tol) {
#pragma unroll
            for (int a = 0; a < NT; ++a)
#pragma unroll
                for (int b = 0; b < NT; ++b) {
                    const int i = ti + 32 * a, c = tc + 32 * b;
                    if (i < n && c < n) {
                        const T e = (i == c) ? (T)1 : (T)0;
                        if constexpr (!FOLD) r_out.at(i, c) = e;
                        rinv_out.at(i, c) = e;
                        if constexpr (FOLD) {  // (from A, behind the barrier above: written along r_out's contiguous index whichever that is)
                            const bool rows_fast = r_out.rs < r_out.cs;
                            const int io = rows_fast ? tc + 32 * b : i, co = rows_fast ? ti + 32 * a : c;
                            if (io < n && co < n) r_out.at(io, co) = A[io * ld + co];
                        }
                    }
                }
            return;
        }
    }

    // One loop for the factor and its inverse.  X = R^-1 by the right-looking column recurrence of X R = I:
    //   X(:, j) /= r_jj ;  X(:, c) -= X(:, j) R(j, c)  for c > j
    // needs exactly the row of R that step j of the factorization completes, so both rank-1 updates share the step's one
    // barrier (the separate bottom-up Gauss-Jordan pass was another n dependent steps).  X is register-tiled like the
    // factor; only tiles on or above the block diagonal exist (a <= b).
    T xr[NT][NT];
#pragma unroll
    for (int a = 0; a < NT; ++a)
#pragma unroll
        for (int b = 0; b < NT; ++b) xr[a][b] = (ti + 32 * a == tc + 32 * b) ? (T)1 : (T)0;
    T *colbuf = A;  // 2 * n
    for (int j = 0; j < n; ++j) {
        T *rb = rowbuf + (j & 1) * n;
        T *cb = colbuf + (j & 1) * n;
        const int ja = j >> 5, jt = j & 31;
        if (ti == jt) {  // owners of row j publish it (unscaled; rb[j] is the pivot)
#pragma unroll
            for (int a = 0; a < NT; ++a)
                if (a == ja) {
#pragma unroll
                    for (int b = a; b < NT; ++b) {
                        const int c = tc + 32 * b;
                        if (c >= j && c < n) rb[c] = reg[a][b];
                    }
                }
        }
        if (tc == jt) {  // owners of column j of X publish it (before its scaling; rows <= j)
#pragma unroll
            for (int b = 0; b < NT; ++b)
                if (b == ja) {
#pragma unroll
                    for (int a = 0; a <= b; ++a) {
                        const int i = ti + 32 * a;
                        if (i <= j) cb[i] = xr[a][b];
                    }
                }
        }
        __syncthreads();
        T d = rb[j];
        if (!(d > (T)0)) {
            if (tid == 0) atomicOr(flag, 1);
            d = tiny_pivot<T>();
        }
        const T invr = fast_rsqrt(d), invd = invr * invr;
        T cv[NT];
#pragma unroll
        for (int b = 0; b < NT; ++b) { const int c = tc + 32 * b; cv[b] = (c > j && c < n) ? rb[c] : (T)0; }
#pragma unroll
        for (int a = 0; a < NT; ++a) {
            const int i = ti + 32 * a;
            if (i == j) {  // row j becomes the final row of R
#pragma unroll
                for (int b = a; b < NT; ++b) {
                    const int c = tc + 32 * b;
                    if (c >= j && c < n) reg[a][b] *= invr;
                }
            } else if (i > j && i < n) {
                const T w = rb[i] * invd;
#pragma unroll
                for (int b = a; b < NT; ++b) reg[a][b] -= w * cv[b];  // entries below the diagonal are never used
            }
            if (i <= j) {  // X(i, c) -= X(i, j) R(j, c) = (cb[i] / r_jj) (rb[c] / r_jj)
                const T xj = cb[i];
                const T w = xj * invd;
#pragma unroll
                for (int b = a; b < NT; ++b) {
                    xr[a][b] -= w * cv[b];
                    if (b == ja && tc == jt) xr[a][b] = xj * invr;  // column j itself: final
                }
            }
        }
    }
#pragma unroll
    for (int a = 0; a < NT; ++a)
#pragma unroll
        for (int b = 0; b < NT; ++b) {
            const int i = ti + 32 * a, c = tc + 32 * b;
            if (i < n && c < n) {
                if constexpr (!FOLD) r_out.at(i, c) = (b >= a && c >= i) ? reg[a][b] : (T)0;
                rinv_out.at(i, c) = (b >= a && c >= i) ? xr[a][b] : (T)0;
            }
        }
    if constexpr (!FOLD) return;
    // r_out = R r1: R goes into A (the last step's readers of colbuf are past the barrier below).  r1 is read where it lies, in
    // memory, up to n loads per entry: deliberate -- LDS does not hold a second n x n matrix at the n of the flagship workload,
    // and this path (a second pass that does factor) costs its n dependent steps first: 220 us against about 35 for the product.
    __syncthreads();
#pragma unroll
    for (int a = 0; a < NT; ++a)
#pragma unroll
        for (int b = a; b < NT; ++b) {
            const int i = ti + 32 * a, c = tc + 32 * b;
            if (i < n && c < n && c >= i) A[i * ld + c] = reg[a][b];
        }
    __syncthreads();
#pragma unroll
    for (int a = 0; a < NT; ++a)
#pragma unroll
        for (int b = 0; b < NT; ++b) {
            const int i = ti + 32 * a, c = tc + 32 * b;
            if (i < n && c < n) {
                T acc = 0;
                for (int l = i; l <= c; ++l) acc = fma(A[i * ld + l], r1.at(l, c), acc);
                r_out.at(i, c) = acc;
            }
        }
}

template <typename T>
static size_t chol_lds(int64_t n) { return ((size_t)n * (n | 1) + 3 * (size_t)n + 16) * sizeof(T); }

template <typename T, int NT, bool FOLD>
static void chol_inv_launch(rc_context *c, Mat<T> g, Mat<T> r, Mat<T> rinv, Mat<T> r1, bool check_identity, T ident_tol, T skip_tol, int *flag) {
    raise_lds_limit<k_chol_inv<T, NT, FOLD>>(c->device, kLdsCap);
    hipLaunchKernelGGL((k_chol_inv<T, NT, FOLD>), dim3(1), dim3(1024), chol_lds<T>(g.rows), c->stream, g, r, rinv, r1, check_identity ? 1 : 0, ident_tol, skip_tol, flag);
}
// r1 empty: r = R, g = R^T R.  r1 given (n x n upper triangular): r = R r1
template <typename T>
static void chol_inv(rc_context *c, Mat<T> g, Mat<T> r, Mat<T> rinv, Mat<T> r1, bool check_identity, T ident_tol, T skip_tol, int *flag) {
    const int64_t n = g.rows;
    RC_REQUIRE(n <= 224 && chol_lds<T>(n) <= kLdsCap, RC_INVALID_ARGUMENT, "chol_inv: n = %lld does not fit LDS", (long long)n);
    ProfScope ps(c, "op:chol_inv n=%lld", (long long)n);
#define RC_CI(NT_)                                                                                          \
    do {                                                                                                    \
        if (r1.empty()) chol_inv_launch<T, NT_, false>(c, g, r, rinv, r1, check_identity, ident_tol, skip_tol, flag); \
        else chol_inv_launch<T, NT_, true>(c, g, r, rinv, r1, check_identity, ident_tol, skip_tol, flag);    \
    } while (0)
    if (n <= 64) RC_CI(2);
    else if (n <= 160) RC_CI(5);
    else if constexpr (sizeof(T) == 4) RC_CI(7);  // (f64: n > 160 does not fit LDS and has failed the check above)
#undef RC_CI
}

template <typename T>
bool tsqr_supported(int64_t m, int64_t n) {
    const size_t small_lds = ((size_t)n * (n | 1) + 4 * (size_t)n) * sizeof(T) + (size_t)n * sizeof(int) + 256;
    return n >= 2 && m >= 4 * n && m >= 1024 && small_lds <= kLdsCapWide;
}

// Y = Q R by CholeskyQR2 with Q left in factored form: Q = q1 r2i.  y: m x n (any strides, not modified), q1: m x n (row-major
// for coalesced GEMM epilogues), r2i: n x n, r: n x n (upper, any strides).  *flag (device int) gets bits OR-ed in on failure.
// Callers fold r2i into whatever small matrix multiplies Q next (Q2 of the small QRCP, U_c / V_c of the small SVD), so the
// tall matrix is read by two Gram products and written / read by two applications instead of three (four with the sign pass).
// Five launches: two Gram products, one application and the two k_chol_inv; r = R2 R1 is formed inside the second of those.
template <typename T>
void tsqr_cholqr2_factored(rc_context *c, Mat<T> y, Mat<T> q1, Mat<T> r2i, Mat<T> r, int *flag) {
    const int64_t m = y.rows, n = y.cols;
    ProfScope ps(c, "op:cholqr2 %lldx%lld", (long long)m, (long long)n);
    ArenaMark mark(c);
    Mat<T> g = rowmajor(c->alloc<T>((size_t)n * even_ld(n)), n, n, even_ld(n));
    Mat<T> r1 = rowmajor(c->alloc<T>((size_t)n * even_ld(n)), n, n, even_ld(n)), r1i = rowmajor(c->alloc<T>((size_t)n * even_ld(n)), n, n, even_ld(n));
    gemm_chain<T>(c, 1, y.t(), y, 0, g);
    chol_inv<T>(c, g, r1, r1i, Mat<T>(), false, 0, 0, flag);
    gemm_chain<T>(c, 1, y, r1i, 0, q1);
    gemm_chain<T>(c, 1, q1.t(), q1, 0, g);
    // after one pass ||Q1^T Q1 - I|| ~ cond(Y)^2 eps; the second pass is only accurate while that is << 1
    static const int skip_ok = env_int("RC_CHOLQR_SKIP", 1);
    const T skip_tol = skip_ok ? (sizeof(T) == 8 ? (T)2.5e-14 : (T)1e-6) : (T)-1;
    chol_inv<T>(c, g, r, r2i, r1, true, (T)1e-2, skip_tol, flag);  // r = R2 r1
}

// Y = Q R with Q formed: q m x n (any strides)
template <typename T>
void tsqr_cholqr2(rc_context *c, Mat<T> y, Mat<T> q, Mat<T> r, int *flag) {
    const int64_t m = y.rows, n = y.cols;
    ArenaMark mark(c);
    Mat<T> q1 = rowmajor(c->alloc<T>((size_t)m * even_ld(n)), m, n, even_ld(n));
    Mat<T> r2i = rowmajor(c->alloc<T>((size_t)n * even_ld(n)), n, n, even_ld(n));
    tsqr_cholqr2_factored<T>(c, y, q1, r2i, r, flag);
    gemm<T>(c, 1, q1, r2i, 0, q);
}

// ---------------------------------------------------------------------------
// Householder QRCP (?laqp2 semantics) of an n x n matrix in the LDS of ONE workgroup,
// plus the explicit orthogonal factor.  Columns are never moved (jp maps position -> column).
//   rin  : n x n input (any strides)
//   rout : kmax x n, rout(i, p) = (i <= p) ? R(i, jp[p]) : 0      (may be empty)
//   q2   : n x q2.cols = H_0 ... H_{kmax-1} [I ; 0]                 (may be empty)
// ---------------------------------------------------------------------------
template <typename T>
__device__ inline T safe_hypot(T a, T b) {  // ?lapy2
    a = fabs(a); b = fabs(b);
    const T w = max(a, b), z = min(a, b);
    if (z == (T)0) return w;
    const T q = z * fast_rcp(w);
    const T e = (T)1 + q * q;
    return w * (e * fast_rsqrt(e));
}
template <typename T>
__device__ inline T fast_sqrt_pos(T x) { return x > (T)0 ? x * fast_rsqrt(x) : (T)0; }

// One Householder step of k_qrcp_small applied to the trailing columns (one LPP-lane group per column, NEJ rows per lane
// from row j on) + the ?laqp2 norm down-date.  safe != 0: a read past the end of a column stays inside the LDS image (it
// lands in the pad row, in the next column or in the norm / tau / permutation arrays behind the matrix, all of which the kernel
// has written: finite values), so the loads carry no bounds: the reflector entries there are zero, the products are exact zeros
// and the sums are the same bits as with bounds.
template <typename T, int NEJ, int LPP>
__device__ __forceinline__ void qrcp_small_apply(T *A, int ld, int n, int j, int grp, int ll, int ngrp, const int *jp, T *vn1, T *vn2, T tj, int pivot, bool safe) {
    const T *vcol = A + jp[j] * ld;
    T v[NEJ];
#pragma unroll
    for (int e = 0; e < NEJ; ++e) {
        int i = j + ll + LPP * e;
        v[e] = (i < n) ? ((i == j) ? (T)1 : vcol[i]) : (T)0;
    }
    for (int p = j + 1 + grp; p < n; p += ngrp) {
        T *xcol = A + jp[p] * ld;
        T x[NEJ];
        T dot = 0;
        if (safe) {
#pragma unroll
            for (int e = 0; e < NEJ; ++e) {
                x[e] = xcol[j + ll + LPP * e];
                dot = fma(v[e], x[e], dot);
            }
        } else {
#pragma unroll
            for (int e = 0; e < NEJ; ++e) {
                int i = j + ll + LPP * e;
                x[e] = (i < n) ? xcol[i] : (T)0;
                dot = fma(v[e], x[e], dot);
            }
        }
        if (tj != (T)0) {
            dot = group_sum_dpp<LPP>(dot);
            const T f = tj * dot;
#pragma unroll
            for (int e = 0; e < NEJ; ++e) {
                int i = j + ll + LPP * e;
                if (i < n) { x[e] -= f * v[e]; xcol[i] = x[e]; }
            }
        }
        if (pivot) {
            const T xj = xcol[j];  // written by lane ll == 0 of this group: same wave, LDS ops are in order
            const T vn = vn1[p];
            if (vn != (T)0) {
                T t = fabs(xj) * fast_rcp(vn);
                T temp = (T)1 - t * t;
                temp = temp > (T)0 ? temp : (T)0;
                T rr = vn * fast_rcp(vn2[p]);
                T temp2 = temp * rr * rr;
                if (temp2 <= num<T>::tol3z()) {
                    T ss = 0;
#pragma unroll
                    for (int e = 0; e < NEJ; ++e) {
                        int i = j + ll + LPP * e;
                        if (i > j && i < n) ss += x[e] * x[e];
                    }
                    ss = group_sum_dpp<LPP>(ss);
                    if (ll == 0) { T nn = (j < n - 1) ? fast_sqrt_pos(ss) : (T)0; vn1[p] = nn; vn2[p] = nn; }
                } else if (ll == 0) {
                    vn1[p] = vn * fast_sqrt_pos(temp);
                }
            }
        }
    }
}

// x <- H_j x for the Q2 formation of k_qrcp_small: rows ll + LPP e, register blocks E0 .. NE - 1 (the blocks below E0 lie
// above row j, where the reflector is zero).
template <typename T, int NE, int LPP, int E0>
__device__ __forceinline__ void qrcp_small_reflect(T (&x)[NE], const T *vcol, T tj, int j, int n, int ll) {
    T v[NE];
    T dot = 0;
#pragma unroll
    for (int e = E0; e < NE; ++e) {
        int i = ll + LPP * e;
        v[e] = 0;
        if (i < n && i >= j) { v[e] = (i == j) ? (T)1 : vcol[i]; dot = fma(v[e], x[e], dot); }
    }
    dot = group_sum_dpp<LPP>(dot);
    const T f = tj * dot;
#pragma unroll
    for (int e = E0; e < NE; ++e) x[e] -= f * v[e];
}

// The same sums without a branch around each load: every lane's loads are issued together (a masked row reads row j and is zeroed
// by a select), then the products of the live rows are accumulated in qrcp_small_reflect's order, so dot, f and x are its bits.
// For a group that has a CU to itself: there the step is the NE - E0 LDS round trips the branches put one behind the other,
// which sixteen waves on one CU hide behind each other and two cannot.
template <typename T, int NE, int LPP, int E0>
__device__ __forceinline__ void qrcp_small_reflect_flat(T (&x)[NE], const T *vcol, T tj, int j, int n, int ll) {
    T v[NE];
    bool on[NE];
#pragma unroll
    for (int e = E0; e < NE; ++e) {
        const int i = ll + LPP * e;
        on[e] = i < n && i >= j;
        v[e] = vcol[on[e] ? i : j];
    }
    // (the empty statement uses every loaded value, so no load can be sunk under a branch on its mask again)
#pragma unroll
    for (int e = E0; e < NE; ++e) asm volatile("" : "+v"(v[e]));
#pragma unroll
    for (int e = E0; e < NE; ++e) v[e] = on[e] ? ((ll + LPP * e == j) ? (T)1 : v[e]) : (T)0;
    T dot = 0;
#pragma unroll
    for (int e = E0; e < NE; ++e) dot = on[e] ? fma(v[e], x[e], dot) : dot;
    dot = group_sum_dpp<LPP>(dot);
    const T f = tj * dot;
#pragma unroll
    for (int e = E0; e < NE; ++e) x[e] -= f * v[e];
}

// Column cq of Q2 by one LPP-lane group: apply H_min(cq,kmax-1) ... H_0 to e_cq (A, tau, jp: the factored LDS image, read-only)
// (xkeep, FLAT only: the caller's registers get the column as well, rows ll + LPP e)
template <typename T, int NE, int LPP, bool FLAT = false>
__device__ __forceinline__ void qrcp_small_q2_column(const T *A, int ld, int n, int kmax, const T *tau, const int *jp, int cq, int ll, Mat<T> q2, T *xkeep = nullptr) {
    T x[NE];
#pragma unroll
    for (int e = 0; e < NE; ++e) x[e] = (ll + LPP * e == cq) ? (T)1 : (T)0;
    const int j0 = cq < kmax - 1 ? cq : kmax - 1;
    T tnext = tau[j0 > 0 ? j0 : 0];
    int pnext = jp[j0 > 0 ? j0 : 0];
    for (int j = j0; j >= 0; --j) {
        const T tj = FLAT ? tnext : tau[j];
        if (tj == (T)0) {
            if constexpr (FLAT) { const int jn = j > 0 ? j - 1 : 0; tnext = tau[jn]; pnext = jp[jn]; }
            continue;
        }
        const T *vcol = A + (FLAT ? pnext : jp[j]) * ld;
        // register blocks that lie entirely above row j hold only zeros of the reflector: the instance that starts at
        // the largest multiple of four blocks below row j skips them (same sums, the skipped products are exact zeros)
        const int e0 = j / LPP;
        if constexpr (FLAT) {
            // tau and jp of the next step are fetched with this step's reflector, not in front of the next one
            const int jn = j > 0 ? j - 1 : 0;
            tnext = tau[jn];
            pnext = jp[jn];
            if (NE > 12 && e0 >= 12) qrcp_small_reflect_flat<T, NE, LPP, (NE > 12 ? 12 : 0)>(x, vcol, tj, j, n, ll);
            else if (NE > 8 && e0 >= 8) qrcp_small_reflect_flat<T, NE, LPP, (NE > 8 ? 8 : 0)>(x, vcol, tj, j, n, ll);
            else if (NE > 4 && e0 >= 4) qrcp_small_reflect_flat<T, NE, LPP, (NE > 4 ? 4 : 0)>(x, vcol, tj, j, n, ll);
            else qrcp_small_reflect_flat<T, NE, LPP, 0>(x, vcol, tj, j, n, ll);
            continue;
        }
        if (NE > 12 && e0 >= 12) qrcp_small_reflect<T, NE, LPP, (NE > 12 ? 12 : 0)>(x, vcol, tj, j, n, ll);
        else if (NE > 8 && e0 >= 8) qrcp_small_reflect<T, NE, LPP, (NE > 8 ? 8 : 0)>(x, vcol, tj, j, n, ll);
        else if (NE > 4 && e0 >= 4) qrcp_small_reflect<T, NE, LPP, (NE > 4 ? 4 : 0)>(x, vcol, tj, j, n, ll);
        else qrcp_small_reflect<T, NE, LPP, 0>(x, vcol, tj, j, n, ll);
    }
#pragma unroll
    for (int e = 0; e < NE; ++e) {
        int i = ll + LPP * e;
        if (i < n) q2.at(i, cq) = x[e];
        if constexpr (FLAT) xkeep[e] = x[e];
    }
}

// IMG: the kernel stops after the factorization and writes its LDS image (the factored matrix, the norms, tau, then jp) to img
// instead of forming Q2; k_qrcp_small_q2 forms Q2 from it on several workgroups.
template <typename T, int NE, int NTHR, bool IMG = false>
__global__ __launch_bounds__(NTHR) void k_qrcp_small(Mat<T> rin, int kmax, int pivot, int64_t *jpvt_out, Mat<T> rout, Mat<T> q2, T *img = nullptr) {
    constexpr int LPP = 8;     // lanes per column in the update
    // NTHR threads = NTHR / 8 column groups: 1024 (n <= 144) covers the trailing columns of a step in one or two passes
    constexpr int NGRP = NTHR / LPP;
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const int n = (int)rin.rows;
    const int ld = n | 1;
    T *A = reinterpret_cast<T *>(smem_raw);  // column-major: A[c * ld + i]
    T *vn1 = A + (size_t)n * ld;
    T *vn2 = vn1 + n;
    T *tau = vn2 + n;
    int *jp = reinterpret_cast<int *>(tau + n);
    const int tid = threadIdx.x, lane = tid & 63;
    const int ll = tid % LPP, grp = tid / LPP;
    const bool safe = LPP * NE <= 3 * n;  // rows read past a column's end stay inside the LDS image (see qrcp_small_apply)

    for (int e = tid; e < n * n; e += NTHR) {
        int i = e % n, cc = e / n;
        A[cc * ld + i] = rin.at(i, cc);
    }
    // the pad row of an even n (ld = n + 1) is read by the unbounded loads of qrcp_small_apply too: whatever the last kernel on this CU
    // left there -- a NaN or an infinity among it -- times the reflector's zero is a NaN, and the column never becomes a pivot
    if (ld > n)
        for (int cc = tid; cc < n; cc += NTHR) A[cc * ld + n] = (T)0;
    __syncthreads();
    for (int p = grp; p < n; p += NGRP) {
        T acc = 0;
        for (int i = ll; i < n; i += LPP) { T v = A[p * ld + i]; acc += v * v; }
        acc = group_sum_dpp<LPP>(acc);
        if (ll == 0) { T nr = sqrt(acc); vn1[p] = nr; vn2[p] = nr; jp[p] = p; tau[p] = (T)0; }  // tau: unbounded reads may land on it
    }
    __syncthreads();

    for (int j = 0; j < kmax; ++j) {
        if (tid < 64) {  // wave 0: pivot search (first maximum, like idamax), "swap", reflector (?larfg)
            if (pivot) {
                T best = (T)-1;
                int bi = 0x7fffffff;
                for (int p = j + lane; p < n; p += 64) {
                    T v = fabs(vn1[p]);
                    if (v > best) { best = v; bi = p; }
                }
                const T mx = wave_max_dpp(best);
                const int pv = wave_min_dpp(best == mx ? bi : 0x7fffffff);
                const int pvt = (pv >= j && pv < n) ? pv : j;
                if (lane == 0 && pvt != j) {
                    int t = jp[pvt]; jp[pvt] = jp[j]; jp[j] = t;
                    vn1[pvt] = vn1[j];
                    vn2[pvt] = vn2[j];
                }
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            }
            T *col = A + jp[j] * ld;
            const T alpha = col[j];
            T acc = 0;
            for (int i = j + 1 + lane; i < n; i += 64) { T v = col[i]; acc += v * v; }
            acc = wave_sum_dpp(acc);
            const T xnorm = fast_sqrt_pos(acc);
            if (xnorm == (T)0) {
                if (lane == 0) tau[j] = 0;
            } else {
                const T beta = -copysign(safe_hypot(alpha, xnorm), alpha);
                const T scal = fast_rcp(alpha - beta);
                for (int i = j + 1 + lane; i < n; i += 64) col[i] *= scal;
                if (lane == 0) { tau[j] = (beta - alpha) * fast_rcp(beta); col[j] = beta; }
            }
        }
        __syncthreads();
        {   // apply H_j to the remaining columns; one LPP-lane group per column.  The register tile covers the rows that are
            // left (the step is bound by the instructions issued, so short tiles for the late steps count)
            const int rem = n - j;
            const T tj = tau[j];
            if (NE > 12 && rem > 8 * 12) qrcp_small_apply<T, NE, LPP>(A, ld, n, j, grp, ll, NGRP, jp, vn1, vn2, tj, pivot, safe);
            else if (NE > 8 && rem > 8 * 8) qrcp_small_apply<T, (NE > 12 ? 12 : NE), LPP>(A, ld, n, j, grp, ll, NGRP, jp, vn1, vn2, tj, pivot, safe);
            else if (NE > 4 && rem > 8 * 4) qrcp_small_apply<T, (NE > 8 ? 8 : NE), LPP>(A, ld, n, j, grp, ll, NGRP, jp, vn1, vn2, tj, pivot, safe);
            else qrcp_small_apply<T, (NE > 4 ? 4 : NE), LPP>(A, ld, n, j, grp, ll, NGRP, jp, vn1, vn2, tj, pivot, safe);
        }
        __syncthreads();
    }

    for (int p = tid; p < n; p += NTHR) jpvt_out[p] = jp[p];
    if (!rout.empty()) {
        const int64_t total = rout.rows * rout.cols;
        for (int64_t e = tid; e < total; e += NTHR) {
            int i = (int)(e / rout.cols), p = (int)(e % rout.cols);
            rout.at(i, p) = (i <= p) ? A[jp[p] * ld + i] : (T)0;
        }
    }
    if constexpr (IMG) {
        const int nt = n * ld + 3 * n;  // A, vn1, vn2, tau are contiguous; jp follows as ints
        for (int e = tid; e < nt; e += NTHR) img[e] = A[e];
        int *ijp = reinterpret_cast<int *>(img + nt);
        for (int p = tid; p < n; p += NTHR) ijp[p] = jp[p];
        return;
    }
    if (!q2.empty()) {  // column cq of Q2: apply H_min(cq,kmax-1) ... H_0 to e_cq; A is read-only now
        for (int cq = grp; cq < (int)q2.cols; cq += NGRP) qrcp_small_q2_column<T, NE, LPP>(A, ld, n, kmax, tau, jp, cq, ll, q2);
    }
}

// Q2 of k_qrcp_small<T, NE, ., true> on several workgroups: each loads the image into its LDS and forms cpw columns, one 8-lane
// group per column with the steps of the in-kernel formation in its order (qrcp_small_q2_column, loads issued together).
// Columns are independent, so a CU holds cpw / 8 waves of them instead of sixteen and the phase is bound by the longest
// column's dependent chain.
// w not empty: the workgroup goes on to its own columns of  w = r2i q2  and  top = q1top w  (small_product_w_top, rc_device.hpp):
// the columns of Q2 are in registers and the LDS image is dead by then, so they take its place (cpw <= kQ2FoldCols then).
constexpr int kQ2FoldCols = 32;  // 2 * 32 columns of n | 1 words fit where the n columns of the image (n > 64) stood
template <typename T, int NE>
__global__ __launch_bounds__(1024) void k_qrcp_small_q2(const T *img, int n, int kmax, Mat<T> q2, int cpw, Mat<T> r2i, Mat<T> q1top, Mat<T> w, Mat<T> top) {
    constexpr int LPP = 8;
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const int ld = n | 1;
    T *A = reinterpret_cast<T *>(smem_raw);
    T *tau = A + (size_t)n * ld + 2 * n;
    int *jp = reinterpret_cast<int *>(tau + n);
    const int tid = threadIdx.x;
    const int nt = n * ld + 3 * n;
    constexpr int U = 8;  // loads in flight per thread and round (the image is 141 KB at n = 133: three rounds)
    for (int e0 = tid; e0 < nt; e0 += 1024 * U) {
        T val[U];
#pragma unroll
        for (int u = 0; u < U; ++u) val[u] = img[min(e0 + 1024 * u, nt - 1)];
#pragma unroll
        for (int u = 0; u < U; ++u)
            if (e0 + 1024 * u < nt) A[e0 + 1024 * u] = val[u];
    }
    const int *ijp = reinterpret_cast<const int *>(img + nt);
    for (int p = tid; p < n; p += 1024) jp[p] = ijp[p];
    __syncthreads();
    const int ll = tid % LPP, grp = tid / LPP;
    const int cq = (int)blockIdx.x * cpw + grp;
    const bool mine = grp < cpw && cq < (int)q2.cols;
    T x[NE];
    if (mine) qrcp_small_q2_column<T, NE, LPP, true>(A, ld, n, kmax, tau, jp, cq, ll, q2, x);
    if (w.empty()) return;
    const int c0 = (int)blockIdx.x * cpw, nc = min(cpw, (int)q2.cols - c0);
    T *Qs = A, *Ws = A + kQ2FoldCols * ld;
    __syncthreads();  // every group has read the image for the last time
    if (mine) {
#pragma unroll
        for (int e = 0; e < NE; ++e) {
            const int i = ll + LPP * e;
            if (i < n) Qs[grp * ld + i] = x[e];
        }
    }
    __syncthreads();
    small_product_w_top<T, NE>(r2i, q1top, w, top, c0, nc, Qs, Ws, ld, tid, 1024);
}

// The same columns where Q2 was formed inside k_qrcp_small (q2 is read from memory), and out = r2i x alone (top empty) for
// svd_finish: kSmallProductCols columns per workgroup.
template <typename T, int NT8>
__global__ __launch_bounds__(256) void k_small_products(Mat<T> r2i, Mat<T> x, Mat<T> q1top, Mat<T> w, Mat<T> top) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const int n = (int)r2i.rows, ldx = n | 1;
    T *Xs = reinterpret_cast<T *>(smem_raw), *Ws = Xs + kSmallProductCols * ldx;
    const int tid = threadIdx.x;
    const int c0 = (int)blockIdx.x * kSmallProductCols, nc = min(kSmallProductCols, (int)x.cols - c0);
    if (top.empty()) { small_product_tri<T, NT8>(r2i, x, w, c0, nc, Xs, tid, 256); return; }
    small_product_load_cols<T>(x, c0, nc, Xs, ldx, tid, 256);
    __syncthreads();
    small_product_w_top<T, NT8>(r2i, q1top, w, top, c0, nc, Xs, Ws, ldx, tid, 256);
}
template <typename T>
static void small_products_launch(rc_context *c, Mat<T> r2i, Mat<T> x, Mat<T> q1top, Mat<T> w, Mat<T> top) {
    const int64_t n = r2i.rows;
    RC_REQUIRE(r2i.cols == n && x.rows == n && w.rows == n && w.cols == x.cols && (top.empty() || (q1top.cols == n && top.rows == q1top.rows && top.cols == x.cols)),
               RC_INVALID_ARGUMENT, "small products: shape mismatch");
    if (x.cols == 0) return;
    const size_t lds = 2 * (size_t)kSmallProductCols * (n | 1) * sizeof(T);
    RC_REQUIRE(n <= 8 * 26 && lds <= 64 * 1024, RC_INVALID_ARGUMENT, "small products: n = %lld is too large", (long long)n);
    const dim3 grid((unsigned)cdiv(x.cols, kSmallProductCols));
    if (n <= 8 * 8) hipLaunchKernelGGL((k_small_products<T, 8>), grid, dim3(256), lds, c->stream, r2i, x, q1top, w, top);
    else if (n <= 8 * 18) hipLaunchKernelGGL((k_small_products<T, 18>), grid, dim3(256), lds, c->stream, r2i, x, q1top, w, top);
    else hipLaunchKernelGGL((k_small_products<T, 26>), grid, dim3(256), lds, c->stream, r2i, x, q1top, w, top);
}
// out = r2i x: r2i n x n upper triangular, x and out n x nc (any strides)
template <typename T>
void small_tri_product(rc_context *c, Mat<T> r2i, Mat<T> x, Mat<T> out) {
    ProfScope ps(c, "op:small_tri_product n=%lld cols=%lld", (long long)r2i.rows, (long long)x.cols);
    small_products_launch<T>(c, r2i, x, Mat<T>(), out, Mat<T>());
}

// w not empty (then q2 is not either): w = r2i q2 (n x q2.cols) and top = q1top w (q1top: rows x n) are formed as well, by the
// workgroups that form Q2 where it is spread, by one more launch of the same body where it is not.
template <typename T>
void qrcp_small(rc_context *c, Mat<T> rin, int64_t kmax, bool pivot, int64_t *jpvt, Mat<T> rout, Mat<T> q2, Mat<T> r2i, Mat<T> q1top, Mat<T> w, Mat<T> top) {
    const int64_t n = rin.rows;
    RC_REQUIRE(rin.rows == rin.cols, RC_INVALID_ARGUMENT, "qrcp_small: square input required");
    RC_REQUIRE(w.empty() || (!q2.empty() && !top.empty() && r2i.rows == n && r2i.cols == n && w.rows == n && w.cols == q2.cols && q1top.cols == n &&
                             top.rows == q1top.rows && top.cols == q2.cols),
               RC_INVALID_ARGUMENT, "qrcp_small: shape mismatch of the folded products");
    const size_t lds = ((size_t)n * (n | 1) + 3 * (size_t)n) * sizeof(T) + (size_t)n * sizeof(int) + 64;
    RC_REQUIRE(lds <= kLdsCap && n <= 208, RC_INVALID_ARGUMENT, "qrcp_small: n = %lld does not fit LDS", (long long)n);
    ProfScope ps(c, "op:qrcp_small n=%lld k=%lld", (long long)n, (long long)kmax);
#define RC_QS(NE, NT_)                                                                                                 \
    do {                                                                                                               \
        raise_lds_limit<k_qrcp_small<T, NE, NT_>>(c->device, kLdsCap);                                                 \
        hipLaunchKernelGGL((k_qrcp_small<T, NE, NT_>), dim3(1), dim3(NT_), lds, c->stream, rin, (int)kmax, pivot ? 1 : 0, jpvt, rout, q2, (T *)nullptr); \
    } while (0)
    static const int wide = env_int("RC_QRCP_SMALL_1024", 1);
    // workgroups of the separate Q2 launch (0: Q2 stays inside k_qrcp_small).  With fewer than 8 compressions side by side the
    // kernel slots are the bound: Q2's columns are independent and leave the one CU of k_qrcp_small
    static const int q2_wgs = std::min(std::max(env_int("RC_QRCP_Q2_WGS", 8), 0), 64);
    if (n > 64 && n <= 144 && wide && q2_wgs > 0 && !q2.empty() && c->lanes_in_flight() < 8) {
        ArenaMark mark(c);
        const size_t nt = (size_t)n * (n | 1) + 3 * (size_t)n;
        T *img = c->alloc<T>(nt + (size_t)n);  // (n ints behind nt words of T)
        raise_lds_limit<k_qrcp_small<T, 18, 1024, true>>(c->device, kLdsCap);
        raise_lds_limit<k_qrcp_small_q2<T, 18>>(c->device, kLdsCap);
        hipLaunchKernelGGL((k_qrcp_small<T, 18, 1024, true>), dim3(1), dim3(1024), lds, c->stream, rin, (int)kmax, pivot ? 1 : 0, jpvt, rout, q2, img);
        // whole waves of columns per workgroup (8 columns a wave), at most the 128 column groups of a workgroup
        // (with the products behind the columns at most kQ2FoldCols: both sets of columns stand in LDS where the image was)
        const int cpw = (int)std::min<int64_t>(cdiv(cdiv(q2.cols, q2_wgs), 8) * 8, w.empty() ? 128 : kQ2FoldCols);
        ProfScope pq(c, "op:qrcp_small_q2 n=%lld cols=%lld wgs=%d", (long long)n, (long long)q2.cols, (int)cdiv(q2.cols, cpw));
        hipLaunchKernelGGL((k_qrcp_small_q2<T, 18>), dim3((unsigned)cdiv(q2.cols, cpw)), dim3(1024), lds, c->stream, (const T *)img, (int)n, (int)kmax, q2, cpw, r2i, q1top, w, top);
        return;
    }
    if (n <= 64) RC_QS(8, 512);
    else if (n <= 144 && wide) RC_QS(18, 1024);
    else if (n <= 144) RC_QS(18, 512);
    else RC_QS(26, 512);
#undef RC_QS
    if (!w.empty()) small_products_launch<T>(c, r2i, q2, q1top, w, top);
}

// ---------------------------------------------------------------------------
// Householder sign convention: d_j such that Q D = H_0 ... H_{k-1} [I ; 0] with LAPACK's
// reflectors (beta = -sign(alpha) |x|).  LU-type elimination on the top k x k block of Q.
// ---------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(1024) void k_householder_signs(Mat<T> q, T *d) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const int k = (int)q.cols;
    const int ld = k | 1;
    T *W = reinterpret_cast<T *>(smem_raw);  // W[i * ld + c]
    const int tid = threadIdx.x;
    for (int e = tid; e < k * k; e += 1024) {
        int i = e % k, cc = e / k;
        W[i * ld + cc] = q.at(i, cc);
    }
    __syncthreads();
    const int ti = tid >> 5, tc = tid & 31;
    for (int j = 0; j < k; ++j) {
        const T s = W[j * ld + j];
        const T dj = (s > (T)0) ? (T)-1 : (T)1;
        const T u = (T)1 + fabs(s);
        if (tid == 0) d[j] = dj;
        const T inv = -dj / u;  // one division per step and thread (it was one per row: the kernel was bound by them)
        for (int i = j + 1 + ti; i < k; i += 32) {
            const T li = W[i * ld + j] * inv;
            for (int cc = j + 1 + tc; cc < k; cc += 32) W[i * ld + cc] -= li * W[j * ld + cc];
        }
        __syncthreads();
    }
}
template <typename T>
__global__ __launch_bounds__(256) void k_scale_cols_rows(Mat<T> q, Mat<T> r, const T *d) {
    // q(:, j) *= d_j ; r(j, :) *= d_j
    const int64_t tq = q.rows * q.cols, tr = r.rows * r.cols;
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < tq + tr; e += (int64_t)gridDim.x * blockDim.x) {
        if (e < tq) {
            int64_t j = e / q.rows, i = e - j * q.rows;
            if (d[j] < (T)0) q.at(i, j) = -q.at(i, j);
        } else {
            int64_t f = e - tq;
            int64_t i = f / r.cols, p = f - i * r.cols;
            if (d[i] < (T)0) r.at(i, p) = -r.at(i, p);
        }
    }
}

// d_j of the sign convention from the top k x k block of Q (k x k, any strides)
template <typename T>
static void householder_signs(rc_context *c, Mat<T> top, T *d) {
    const int64_t k = top.cols;
    const size_t lds = (size_t)k * (k | 1) * sizeof(T);
    RC_REQUIRE(top.rows >= k && lds <= kLdsCap, RC_INVALID_ARGUMENT, "sign fix: k = %lld does not fit LDS", (long long)k);
    raise_lds_limit<k_householder_signs<T>>(c->device, kLdsCap);
    hipLaunchKernelGGL(k_householder_signs<T>, dim3(1), dim3(1024), lds, c->stream, top, d);
}
template <typename T>
static void scale_cols_rows(rc_context *c, Mat<T> q, Mat<T> r, const T *d) {
    const int64_t total = q.rows * q.cols + r.rows * r.cols;
    hipLaunchKernelGGL(k_scale_cols_rows<T>, dim3((unsigned)std::min<int64_t>(cdiv(total, 256), 4096)), dim3(256), 0, c->stream, q, r, d);
}

template <typename T>
void householder_sign_fix(rc_context *c, Mat<T> q, Mat<T> r) {
    const int64_t k = q.cols;
    if (k == 0) return;
    RC_REQUIRE(q.rows >= k, RC_INVALID_ARGUMENT, "sign fix: q must be tall");
    ProfScope ps(c, "op:householder_sign_fix k=%lld", (long long)k);
    ArenaMark mark(c);
    T *d = c->alloc<T>((size_t)k);
    householder_signs<T>(c, q, d);
    scale_cols_rows<T>(c, q, r, d);
}

int tsqr_fold() {
    static const int fold = env_int("RC_TSQR_FOLD", 1);
    return fold;
}

// Pivoted (or plain) QR of the tall-skinny y through CholeskyQR2 + small QRCP + sign fix.
//   q: m x k column-major (may be empty), r: k x n (may be empty), ind: n
// Q = Q1 (R2^-1 Q2 D): the n x k factor W = R2^-1 Q2 is formed first, the signs D (+-1: exact) come from the top k x k block
// Q1[:k, :] W and go into W's columns and R's rows, and ONE tall product writes Q.  (Until round 3: Q1 R2^-1, then (.) Q2, then a
// sign pass over Q: two more passes over the tall matrix; RC_TSQR_FOLD=0 restores that order.)
template <typename T>
void qrcp_tall_fast(rc_context *c, Mat<T> y, int64_t k, bool pivot, Mat<T> q, Mat<T> r, int64_t *ind, int *flag) {
    const int64_t m = y.rows, n = y.cols;
    ProfScope ps(c, "op:qrcp_tall_fast %lldx%lld k=%lld pivot=%d", (long long)m, (long long)n, (long long)k, pivot ? 1 : 0);
    ArenaMark mark(c);
    const int fold = tsqr_fold();
    Mat<T> q1 = rowmajor(c->alloc<T>((size_t)m * even_ld(n)), m, n, even_ld(n));
    Mat<T> r1 = colmajor(c->alloc<T>((size_t)n * even_ld(n)), n, n, even_ld(n));
    Mat<T> r2i = rowmajor(c->alloc<T>((size_t)n * even_ld(n)), n, n, even_ld(n));
    if (fold) tsqr_cholqr2_factored<T>(c, y, q1, r2i, r1, flag);
    else tsqr_cholqr2<T>(c, y, q1, r1, flag);
    Mat<T> q2 = colmajor(c->alloc<T>((size_t)even_ld(n) * k), n, k, even_ld(n));
    Mat<T> rr = r.empty() ? rowmajor(c->alloc<T>((size_t)k * even_ld(n)), k, n, even_ld(n)) : r;
    Mat<T> qq = q.empty() ? rowmajor(c->alloc<T>((size_t)m * even_ld(k)), m, k, even_ld(k)) : q;
    if (!fold) {
        qrcp_small<T>(c, r1, k, pivot, ind, rr, q2, Mat<T>(), Mat<T>(), Mat<T>(), Mat<T>());
        gemm<T>(c, 1, q1, q2, 0, qq);
        householder_sign_fix<T>(c, qq, rr);
        return;
    }
    Mat<T> w = colmajor(c->alloc<T>((size_t)even_ld(n) * k), n, k, even_ld(n));
    Mat<T> top = colmajor(c->alloc<T>((size_t)even_ld(k) * k), k, k, even_ld(k));
    T *d = c->alloc<T>((size_t)k);
    qrcp_small<T>(c, r1, k, pivot, ind, rr, q2, r2i, q1.sub(0, k, 0, n), w, top);  // ... and w = r2i q2, top = q1[:k, :] w
    householder_signs<T>(c, top, d);
    scale_cols_rows<T>(c, w, rr, d);
    gemm_chain<T>(c, 1, q1, w, 0, qq);
}

#define RC_INST(T)                                                                                               \
    template bool tsqr_supported<T>(int64_t, int64_t);                                                           \
    template void tsqr_cholqr2<T>(rc_context *, Mat<T>, Mat<T>, Mat<T>, int *);                                  \
    template void tsqr_cholqr2_factored<T>(rc_context *, Mat<T>, Mat<T>, Mat<T>, Mat<T>, int *);                 \
    template void qrcp_small<T>(rc_context *, Mat<T>, int64_t, bool, int64_t *, Mat<T>, Mat<T>, Mat<T>, Mat<T>, Mat<T>, Mat<T>); \
    template void small_tri_product<T>(rc_context *, Mat<T>, Mat<T>, Mat<T>);                                   \
    template void householder_sign_fix<T>(rc_context *, Mat<T>, Mat<T>);                                         \
    template void qrcp_tall_fast<T>(rc_context *, Mat<T>, int64_t, bool, Mat<T>, Mat<T>, int64_t *, int *);
RC_INST(double)
RC_INST(float)
#undef RC_INST

}  // namespace rc
