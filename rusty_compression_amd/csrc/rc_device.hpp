// Device-side helpers shared by the single-workgroup kernels: DPP / readlane reductions
// (no LDS traffic, no ds_bpermute latency) and Newton-refined f64 reciprocal / rsqrt.
// gfx950 (wave64, GFX9 DPP controls) only.
#pragma once

#include <hip/hip_runtime.h>

namespace rc {

// ---- DPP moves -----------------------------------------------------------------
// quad_perm [1,0,3,2] = 0xB1, quad_perm [2,3,0,1] = 0x4E, row_half_mirror = 0x141, row_mirror = 0x140
template <int CTRL>
__device__ inline float dpp_mov(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, true));
}
template <int CTRL>
__device__ inline int dpp_mov(int v) {
    return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xF, 0xF, true);
}
template <int CTRL>
__device__ inline double dpp_mov(double v) {
    long long b = __double_as_longlong(v);
    int lo = (int)(b & 0xffffffffLL), hi = (int)(b >> 32);
    int rlo = __builtin_amdgcn_update_dpp(0, lo, CTRL, 0xF, 0xF, true);
    int rhi = __builtin_amdgcn_update_dpp(0, hi, CTRL, 0xF, 0xF, true);
    return __longlong_as_double(((long long)rhi << 32) | (unsigned int)rlo);
}

// sum over an aligned group of W lanes (W = 4, 8 or 16); every lane of the group gets the
// total, bitwise identical across the group (the butterfly is symmetric)
template <int W, typename T>
__device__ inline T group_sum_dpp(T v) {
    v += dpp_mov<0xB1>(v);
    v += dpp_mov<0x4E>(v);
    if (W >= 8) v += dpp_mov<0x141>(v);
    if (W >= 16) v += dpp_mov<0x140>(v);
    return v;
}
template <int W, typename T>
__device__ inline T group_max_dpp(T v) {
    v = max(v, dpp_mov<0xB1>(v));
    v = max(v, dpp_mov<0x4E>(v));
    if (W >= 8) v = max(v, dpp_mov<0x141>(v));
    if (W >= 16) v = max(v, dpp_mov<0x140>(v));
    return v;
}
template <int W>
__device__ inline int group_min_dpp(int v) {
    v = min(v, dpp_mov<0xB1>(v));
    v = min(v, dpp_mov<0x4E>(v));
    if (W >= 8) v = min(v, dpp_mov<0x141>(v));
    if (W >= 16) v = min(v, dpp_mov<0x140>(v));
    return v;
}

// ---- readlane (wave-uniform result) ------------------------------------------------
__device__ inline int read_lane(int v, int lane) { return __builtin_amdgcn_readlane(v, lane); }
__device__ inline float read_lane(float v, int lane) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane)); }
__device__ inline double read_lane(double v, int lane) {
    long long b = __double_as_longlong(v);
    int lo = __builtin_amdgcn_readlane((int)(b & 0xffffffffLL), lane);
    int hi = __builtin_amdgcn_readlane((int)(b >> 32), lane);
    return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}

// full-wave (64 lanes) reductions: DPP inside the four rows, then four readlanes
template <typename T>
__device__ inline T wave_sum_dpp(T v) {
    v = group_sum_dpp<16>(v);
    return (read_lane(v, 0) + read_lane(v, 16)) + (read_lane(v, 32) + read_lane(v, 48));
}
template <typename T>
__device__ inline T wave_max_dpp(T v) {
    v = group_max_dpp<16>(v);
    return max(max(read_lane(v, 0), read_lane(v, 16)), max(read_lane(v, 32), read_lane(v, 48)));
}
__device__ inline int wave_min_dpp(int v) {
    v = group_min_dpp<16>(v);
    return min(min(read_lane(v, 0), read_lane(v, 16)), min(read_lane(v, 32), read_lane(v, 48)));
}

// ---- power-of-two normalisation of a batched working copy ---------------------------------
// The batched IDs and SVDs bring their working copy to a largest component magnitude in [1, 2) by an exact power of two, so that the
// sums of squares of the column norms and of ?larfg neither overflow nor go subnormal for any block inside the stated domain, and the
// result for 2^e A is bit for bit the result for A (a power of two commutes with every rounding inside the normal range).
// The key of one component: its magnitude, +inf for NaN and +-inf (max() then never sees a NaN and a non-finite block is recognised)
template <typename T>
__device__ inline T pow2_key(T v) {
    const T a = fabs(v);
    return a < (T)INFINITY ? a : (T)INFINITY;
}
// The block's exponent e = floor(log2(max key)) from every thread's own maximum, for workgroups of four waves: one DPP wave maximum, four
// values through stage[0..3], one barrier.  A zero block and a block with a non-finite entry take e = 0 (the working copy is then the
// input, bit for bit).  e is clamped so that 2^-e is a normal number.  Uniform over the workgroup.
template <typename T>
__device__ inline int block_pow2_exponent(T mx, T *stage, int wv, int lane) {
    mx = wave_max_dpp(mx);
    if (lane == 0) stage[wv] = mx;
    __syncthreads();
    mx = max(max(stage[0], stage[1]), max(stage[2], stage[3]));
    if (mx == (T)0 || !(mx < (T)INFINITY)) return 0;
    constexpr int lim = sizeof(T) == 8 ? 1022 : 126;
    const int e = ilogb(mx);
    return e < -lim ? -lim : (e > lim ? lim : e);
}

// ---- sums of squares over the whole f64 range: the three accumulators of LAPACK 3.10's ?lassq ----
// A component with magnitude in [2^-511, 2^486) is squared as it stands (med: the plain sum), a larger one after a multiplication by
// 2^-538 (big), a smaller one after a multiplication by 2^537 (sml): no square overflows or goes subnormal, and 2^32 of them still sum
// inside the range.  The constants are ?lassq's tsml, tbig, sbig and ssml for f64.  NaN goes into med and stays NaN, +-inf into big.
// The bins are summed apart, each in the caller's fixed order, and combined once (ssq_norm).
constexpr double SSQ_TSML = 0x1p-511, SSQ_TBIG = 0x1p486, SSQ_SSML = 0x1p537, SSQ_SBIG = 0x1p-538;
struct SumSq3 {
    double med, big, sml;
};
__device__ __forceinline__ void ssq_add(SumSq3 &s, double v) {
    const double a = fabs(v);
    if (a >= SSQ_TBIG) {
        const double t = v * SSQ_SBIG;
        s.big = fma(t, t, s.big);
    } else if (a < SSQ_TSML) {
        const double t = v * SSQ_SSML;
        s.sml = fma(t, t, s.sml);
    } else {
        s.med = fma(v, v, s.med);
    }
}
// The watch that lets a caller keep the single accumulator on plain data: the largest exponent field of the components seen and the
// smallest one minus 1, a zero field (zero, or a subnormal, whose square vanishes against any block of the domain) left out by the
// wrap-around.  ssq_all_plain: every component seen lies in [2^-511, 2^486) (fields 512 .. 1508) or has a zero field; then the plain
// sum is the med bin, bit for bit, and big and sml take nothing.  NaN and +-inf (field 2047) are not plain.
__device__ __forceinline__ void ssq_watch(unsigned &emx, unsigned &emn, double v) {
    const unsigned e = ((unsigned)__double2hiint(v) >> 20) & 0x7ffu;
    emx = max(emx, e);
    emn = min(emn, e - 1u);
}
__device__ __forceinline__ bool ssq_all_plain(unsigned emx, unsigned emn) { return emx < 1509u && emn >= 511u; }
// sqrt of the sum the three bins stand for, ?lassq's combination followed by ?nrm2's: with nothing in big and sml it is sqrt(med), the
// single accumulator's result bit for bit.  Roundings on top of the bins' own sums: at most 5 (two sqrt, a division, 1 + q^2, a product).
__device__ inline double ssq_norm(double med, double big, double sml) {
    if (med != med) return med;
    if (big > 0.0) {
        if (med > 0.0) big += (med * SSQ_SBIG) * SSQ_SBIG;
        return sqrt(big) * 0x1p538;
    }
    if (sml > 0.0) {
        if (med > 0.0) {
            const double x = sqrt(med), y = sqrt(sml) * 0x1p-537;
            const double lo = x < y ? x : y, hi = x < y ? y : x, q = lo / hi;
            return hi * sqrt(fma(q, q, 1.0));
        }
        return sqrt(sml) * 0x1p-537;
    }
    return sqrt(med);
}

// ---- fast, fully accurate reciprocal / reciprocal square root --------------------------
// v_rcp_f64 / v_rsq_f64 deliver ~2^-23 relative accuracy; two Newton steps reach the f64
// rounding level (error <= ~2 ulp) at a fraction of the IEEE division / sqrt expansions.
__device__ inline double fast_rcp(double x) {
    double r = __builtin_amdgcn_rcp(x);
    r = fma(fma(-x, r, 1.0), r, r);
    r = fma(fma(-x, r, 1.0), r, r);
    return r;
}
__device__ inline float fast_rcp(float x) { return 1.0f / x; }
__device__ inline double fast_rsqrt(double x) {
    double r = __builtin_amdgcn_rsq(x);
    // r <- r * (1.5 - 0.5 x r^2)
    r = r * fma(-0.5 * x, r * r, 1.5);
    r = r * fma(-0.5 * x, r * r, 1.5);
    return r;
}
__device__ inline float fast_rsqrt(float x) { return 1.0f / sqrtf(x); }

// ---- the constants of the number formats: eps = the unit roundoff (LAPACK's ?lamch('E')), tol3z = sqrt(eps) ----
template <typename T> struct num;
template <> struct num<double> {
    static __host__ __device__ constexpr double eps() { return 1.1102230246251565e-16; }    // 2^-53
    static __host__ __device__ constexpr double tol3z() { return 1.0536712127723509e-08; }  // sqrt(2^-53)
};
template <> struct num<float> {
    static __host__ __device__ constexpr float eps() { return 5.9604644775390625e-08f; }  // 2^-24
    static __host__ __device__ constexpr float tol3z() { return 2.44140625e-04f; }        // sqrt(2^-24)
};

// ---- ?laqp2 partial-norm down-date ---------------------------------------------------
// tol3z: below it the down-dated norm has lost its digits and is recomputed from the column.  The same formula as the down-date of
// the per-step chain (kernels_qr.hip, k_qr_apply), which keeps its own copy so that its instantiations stay as they were.
// vn: partial norm of the column before the step (vn1), vn_ref: its norm at the last recompute (vn2), xj: its new row-j entry.
// Returns true when the norm must be recomputed from rows j+1.. of the updated column; otherwise *vn_new is the down-dated norm.
template <typename T>
__device__ inline bool laqp2_downdate(T vn, T vn_ref, T xj, T *vn_new) {
    T t = fabs(xj) / vn;
    T temp = (T)1 - t * t;
    temp = temp > (T)0 ? temp : (T)0;
    T r = vn / vn_ref;
    T temp2 = temp * r * r;
    if (temp2 <= num<T>::tol3z()) return true;
    *vn_new = vn * sqrt(temp);
    return false;
}

// ---- one-sided (Hestenes) Jacobi: shared by the lone core (kernels_svd.hip) and the batched SVD (kernels_batched_id.hip) ----

// circle-method pairing: round r of N-1 (N even), pair slot pi of N/2
__device__ inline void rr_pair(int N, int r, int pi, int &p, int &q) {
    if (pi == 0) { p = N - 1; q = r; }
    else { p = (r + pi) % (N - 1); q = (r - pi + (N - 1)) % (N - 1); }
    if (p > q) { int t = p; p = q; q = t; }
}

// Rotation that annihilates the (p, q) entry of the Gram matrix: with d = aqq - app, h = 2 apq (zeta = d / h)
//   t = sign(zeta) / (|zeta| + sqrt(1 + zeta^2)) = sign(d h) |h| / (|d| + sqrt(d^2 + h^2)),   c = 1 / sqrt(1 + t^2),  s = c t
// -- the second form has one reciprocal less on the round's dependent chain.  t only decides how completely the entry is
// annihilated, so its reciprocal and root take ONE Newton step (1e-15); c decides the orthogonality of the rotation and keeps two.
// Always evaluated in f64: with f32 parameters c^2 + s^2 - 1 has a systematic sign, and the thousands of rotations a
// column goes through inflate the singular values (3e-5 at n = 300).  A tiny angle (|d| >> |h|) is safe: t -> 0.
template <typename T>
__device__ inline void jacobi_rotation(T app, T aqq, T apq, T &c, T &s) {
    const double d = (double)aqq - (double)app, h = 2.0 * (double)apq;
    const double w = fma(d, d, h * h);
    double ri = __builtin_amdgcn_rsq(w);
    ri = ri * fma(-0.5 * w, ri * ri, 1.5);
    const double den = fabs(d) + w * ri;
    double rd = __builtin_amdgcn_rcp(den);
    rd = fma(fma(-den, rd, 1.0), rd, rd);
    const double t = copysign(fabs(h) * rd, d * h);
    const double cd = fast_rsqrt(fma(t, t, 1.0));
    c = (T)cd;
    s = (T)(cd * t);
}

// The two threshold tests of a column pair, on apq2 = |apq|^2 formed in f64.  Both compare products of squared norms, so both are
// evaluated in f64 whatever T is (for T = double the casts are no-ops): in f32 two columns of norm 1e-9 or less put
// tol^2 app aqq below the smallest f32 number and apq^2 next to it, the tests then read "rotate iff apq^2 did not vanish", the sweeps
// stop with cosines far above tol between the columns of tiny singular values, and G Sigma^-1 is not orthonormal (measured with
// the tests in f32 on 4^-5 X Y^T and 4^-8 X Y^T of rank n / 4, n = 32 .. 192: max |U^T U - I| = 2e-4 .. 0.59, against 3e-6 in f64).
//   coupled: rotate iff |apq| > tol sqrt(app aqq)   (tol2 = tol^2)
template <typename T>
__device__ __forceinline__ bool jacobi_pair_is_coupled(T app, T aqq, double apq2, T tol2) {
    return apq2 > (double)tol2 * (double)app * (double)aqq;
}
//   "another sweep is needed" after a rotation by the angle (c, s) of a pair whose cosine was g.  Such a rotation leaves at most
// |s| * (largest cosine of this sweep) behind in pairs that were already annihilated, so a sweep may be the last one only if every
// rotation in it had BOTH a small cosine (g <= sqrt(tol) / 4, 9e-9 in f64) AND a small angle (|s| <= 4 sqrt(tol)): for well
// separated singular values the second follows from the first (quadratic convergence), for clustered / repeated ones
// (sigma_p ~ sigma_q: the angle is O(1) however small g is) it does not, and such sweeps are followed by another one until an
// all-quiet or all-small sweep has been seen
template <typename T>
__device__ __forceinline__ bool jacobi_rotation_was_large(T app, T aqq, double apq2, T s, T tol) {
    return apq2 > (double)tol * 0.0625 * (double)app * (double)aqq || s * s > (T)16 * tol;
}

// Sweep budget of the LDS-resident Jacobi; the fused launch of k_jacobi_lds hands the sweep count over in the 8-bit payload of a tagged word.
constexpr int kMaxSweeps = 30;

// ---- the chain's small products, inside the kernels next to them ("The small products folded") ----
// out(i, c0 + cc) = sum_l a(i, l) X[cc * ldx + l], i < rows, cc < nc, l < n: the nc columns of the right factor stand in LDS, one
// 8-lane group forms one row of eight of them.  Lane ll takes l = ll + 8 t with t ascending (UPPER: a is upper triangular and no
// term left of the diagonal is taken), then the eight partial sums go through group_sum_dpp<8>.
// That is ONE order per entry: it depends on neither the workgroup size, nor the columns a workgroup holds, nor the launch the
// body runs in, so two paths that call it on the same operands give the same bits.  xout (LDS, may be null) gets the result as
// well, xout[cc * ldx + i].  M: Mat<T>.  Whole 8-lane groups must enter.  NT8 >= cdiv(n, 8): a lane's entries of the row are
// loaded together, one round trip to memory per item.  Every fma reads its operand of the right factor from LDS, so the CU's
// one LDS pipe is the bound of the body (profiles/r08_small_products_ab.txt).
template <typename T, bool UPPER, int NT8, typename M>
__device__ __forceinline__ void small_product_cols(M a, int rows, int n, const T *X, int ldx, int nc, M out, int c0, T *xout, int tid, int nthr) {
    constexpr int LPP = 8, CW = 8;
    const int ll = tid % LPP, ngrp = nthr / LPP;
    const int ncg = (nc + CW - 1) / CW;
    for (int item = tid / LPP; item < rows * ncg; item += ngrp) {
        const int i = item % rows, cb = (item / rows) * CW;
        const T *xc[CW];
#pragma unroll
        for (int u = 0; u < CW; ++u) xc[u] = X + (cb + u < nc ? cb + u : nc - 1) * ldx;
        T acc[CW], av[NT8];
#pragma unroll
        for (int u = 0; u < CW; ++u) acc[u] = 0;
        const T *arow = &a.at(i, 0);
#pragma unroll
        for (int t = 0; t < NT8; ++t) {
            const int l = ll + LPP * t;
            av[t] = (l < n && (!UPPER || l >= i)) ? arow[l * a.cs] : (T)0;
        }
#pragma unroll
        for (int t = 0; t < NT8; ++t) {
            const int l = ll + LPP * t;
            if (l < n && (!UPPER || l >= i)) {  // (no term where there is none: LDS past a column's end is not read)
#pragma unroll
                for (int u = 0; u < CW; ++u) acc[u] = fma(av[t], xc[u][l], acc[u]);
            }
        }
#pragma unroll
        for (int u = 0; u < CW; ++u) acc[u] = group_sum_dpp<LPP>(acc[u]);
        if (ll == 0) {
#pragma unroll
            for (int u = 0; u < CW; ++u)
                if (cb + u < nc) {
                    out.at(i, c0 + cb + u) = acc[u];
                    if (xout) xout[(cb + u) * ldx + i] = acc[u];
                }
        }
    }
}
// columns [c0, c0 + nc) of x to LDS, X[cc * ldx + i]
template <typename T, typename M>
__device__ __forceinline__ void small_product_load_cols(M x, int c0, int nc, T *X, int ldx, int tid, int nthr) {
    const int rows = (int)x.rows;
    for (int e = tid; e < nc * rows; e += nthr) {
        const int cc = e / rows, i = e - cc * rows;
        X[cc * ldx + i] = x.at(i, c0 + cc);
    }
}
// Columns [c0, c0 + nc) of  w = r2i q2  (r2i: n x n upper triangular, the columns of q2 in LDS at Qs) and of  top = q1top w
// (q1top: k x n), for qrcp_tall_fast.  Ws: LDS for the same columns of w.  Called by every thread of the workgroup.
template <typename T, int NT8, typename M>
__device__ __forceinline__ void small_product_w_top(M r2i, M q1top, M w, M top, int c0, int nc, const T *Qs, T *Ws, int ldx, int tid, int nthr) {
    const int n = (int)r2i.rows;
    small_product_cols<T, true, NT8>(r2i, n, n, Qs, ldx, nc, w, c0, Ws, tid, nthr);
    __syncthreads();
    small_product_cols<T, false, NT8>(q1top, (int)q1top.rows, n, Ws, ldx, nc, top, c0, (T *)nullptr, tid, nthr);
}
// Columns [c0, c0 + nc) of  out = r2i x  (x read from memory), for svd_finish.  X: LDS, nc * (n | 1) words.  Called by every
// thread of the workgroup.
template <typename T, int NT8, typename M>
__device__ __forceinline__ void small_product_tri(M r2i, M x, M out, int c0, int nc, T *X, int tid, int nthr) {
    const int n = (int)r2i.rows, ldx = n | 1;
    small_product_load_cols<T>(x, c0, nc, X, ldx, tid, nthr);
    __syncthreads();
    small_product_cols<T, true, NT8>(r2i, n, n, X, ldx, nc, out, c0, (T *)nullptr, tid, nthr);
}
constexpr int kSmallProductCols = 8;  // columns per workgroup where the body has a launch, or a role of one, to itself

}  // namespace rc
