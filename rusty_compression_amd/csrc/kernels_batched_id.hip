// Batched column ID of many small same-shaped matrices in one launch (rc_column_id_rank_batched_*).
//
// Per matrix the sequence of rc_column_id_rank_*: QR::compute_from(a) -> compress(.) -> column_id()
// (reference src/qr.rs:187-200, :270-309; examples/interpolative_decomposition.rs:25-32) with ?geqp3's pivoting rule.
//
// MI355X mapping.  A persistent grid of G workgroups (256 threads = 4 waves) walks the batch, b = blockIdx.x, blockIdx.x + G, ...;
// one workgroup factors one matrix from start to finish, so nothing crosses workgroups and matrix b's bits depend on matrix b
// alone (not on G, count or the neighbours).  The m x n working copy lives in LDS when it fits next to the small arrays, otherwise
// in workgroup blockIdx.x's slot of a G x (m x n) global workspace: bounded by G, not by count.  Per step j:
//   wave 0      pivot search over the partial norms in LDS (first maximum, NaN skipped, like k_qr_pivot_reflect), index "swap" in jp[]
//   workgroup   ?larfg on column jp[j] (the formula of k_qr_pivot_reflect); R_jj decides the rank (tolerance or exact zero)
//   one wave per column: H_j applied to the trailing columns from registers + the ?laqp2 norm down-date (k_qr_apply's scheme)
// After r steps: Z = [I | R11^-1 R12] P^T by k_id_z's blocked back substitution (16 x 16 tiles of R11 staged in LDS, one thread
// per right-hand side), written straight to its final column; C[:, j] = A[:, jp[j]] copied from the input (bit for bit).
//
// Batched two-sided ID (rc_two_sided_id_rank_batched_*): the same workgroup then takes the row ID of C = A[:, col_ind[:r]] as the
// column ID of C^T (reference ColumnID::two_sided_id, src/col_interp_decomp.rs:116-125: an LQ of C, then row_id()), through the
// same three device stages (load + norms, pivoted QR with the stopping rule, Z back substitution).
#include "rc_common.hpp"
#include "rc_device.hpp"

namespace rc {

namespace {

constexpr int BID_THREADS = 256;
constexpr int BID_WAVES = BID_THREADS / 64;
constexpr int BID_NB = 16;  // back-substitution tile (k_id_z's)

// dynamic LDS: [W: m x ldw, LDS variant only] vn1[n] vn2[n] tile[16 x 17] red[8] | jp[n] (ints last: the T arrays stay aligned)
template <typename T>
size_t bid_lds_bytes(int m, int n, bool in_lds) {
    size_t t = (size_t)2 * n + BID_NB * (BID_NB + 1) + 8;
    if (in_lds) t += (size_t)n * (size_t)(m | 1);
    return t * sizeof(T) + (size_t)n * sizeof(int);
}

// H_j applied to the trailing columns p = j+1 .. n-1, one wave per column, two columns per wave in flight; rows j + lane + 64 e
// of the column in registers (NE * 64 >= m - j), then the ?laqp2 down-date of the column's partial norm
template <typename T, int NE>
__device__ __forceinline__ void bid_apply(T *W, int ldw, int m, int n, int j, const int *jp, T *vn1, T *vn2, T tj, int wv, int lane) {
    const int mrem = m - j;
    const T *vc = W + (size_t)jp[j] * ldw + j;
    T v[NE];
#pragma unroll
    for (int e = 0; e < NE; ++e) {
        // branch-free: lanes past the end read row j (always valid) and are masked by a select, as in k_qr_apply
        const int li = lane + 64 * e;
        const bool ok = li < mrem;
        const T vv = vc[ok ? li : 0];
        v[e] = ok ? (li == 0 ? (T)1 : vv) : (T)0;
    }
    for (int p0 = j + 1 + wv; p0 < n; p0 += 2 * BID_WAVES) {
        const int p1 = p0 + BID_WAVES;
        const bool has1 = p1 < n;  // wave-uniform
        T *xc[2] = {W + (size_t)jp[p0] * ldw + j, W + (size_t)jp[has1 ? p1 : p0] * ldw + j};
        T x[2][NE];
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int e = 0; e < NE; ++e) {
                const int li = lane + 64 * e;
                const bool ok = li < mrem;
                const T xv = xc[u][ok ? li : 0];
                x[u][e] = ok ? xv : (T)0;
            }
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            if (u == 1 && !has1) break;
            const int p = u ? p1 : p0;
            if (tj != (T)0) {  // tau == 0: H = I
                T dot = 0;
#pragma unroll
                for (int e = 0; e < NE; ++e) dot = fma(v[e], x[u][e], dot);
                const T f = tj * wave_sum_dpp(dot);
#pragma unroll
                for (int e = 0; e < NE; ++e) {
                    const int li = lane + 64 * e;
                    x[u][e] = fma(-f, v[e], x[u][e]);  // v is zero out of range
                    if (li < mrem) xc[u][li] = x[u][e];
                }
            }
            const T vn = vn1[p];
            if (vn != (T)0) {
                T nn;
                if (laqp2_downdate(vn, vn2[p], read_lane(x[u][0], 0), &nn)) {
                    T ss = 0;
#pragma unroll
                    for (int e = 0; e < NE; ++e) {
                        const int li = lane + 64 * e;
                        if (li > 0 && li < mrem) ss += x[u][e] * x[u][e];
                    }
                    ss = wave_sum_dpp(ss);
                    if (lane == 0) { nn = (j < m - 1) ? sqrt(ss) : (T)0; vn1[p] = nn; vn2[p] = nn; }
                } else if (lane == 0) {
                    vn1[p] = nn;
                }
            }
        }
    }
}

// ---- the three stages of one factorization, shared by k_batched_id and both phases of k_batched_two_sided ------------------------
// (m x n below is the matrix being factored: A for a column ID, C^T for the row side of a two-sided ID)

// working copy W[c * ldw + i] = at(i, c), read with the lanes along i (lanes_on_rows) or along c (the input's fast direction),
// then the initial column norms and the identity permutation
template <typename T, typename At>
__device__ __forceinline__ void bid_load(T *W, int ldw, int m, int n, bool lanes_on_rows, At at, T *vn1, T *vn2, int *jp, int wv, int lane) {
    if (lanes_on_rows) {
        for (int c = wv; c < n; c += BID_WAVES)
            for (int i = lane; i < m; i += 64) W[(size_t)c * ldw + i] = at(i, c);
    } else {
        for (int i = wv; i < m; i += BID_WAVES)
            for (int c = lane; c < n; c += 64) W[(size_t)c * ldw + i] = at(i, c);
    }
    __syncthreads();
    for (int c = wv; c < n; c += BID_WAVES) {
        T acc = 0;
        for (int i = lane; i < m; i += 64) { const T v = W[(size_t)c * ldw + i]; acc += v * v; }
        acc = wave_sum_dpp(acc);
        if (lane == 0) { const T nr = sqrt(acc); vn1[c] = nr; vn2[c] = nr; jp[c] = c; }
    }
    __syncthreads();
}

// truncated pivoted QR of the working copy, at most k steps: pivots in jp (?geqp3's rule), R and the Householder vectors in W (LAPACK
// format, physical column order).  Returns the rank: the first j < k with R_jj == 0 or (tol > 0 and |R_jj / R_00| < tol), else k.
template <typename T>
__device__ __forceinline__ int bid_qrcp(T *W, int ldw, int m, int n, int k, double tol, int *jp, T *vn1, T *vn2, T *red, int tid, int wv, int lane) {
    int r = k;
    T r00 = 0;
    for (int j = 0; j < k; ++j) {
        if (wv == 0) {  // pivot: first maximum of the partial norms; NaN never wins (v > best), no valid index -> j
            T best = (T)-1;
            int bi = 0x7fffffff;
            for (int p = j + lane; p < n; p += 64) {
                const T v = fabs(vn1[p]);
                if (v > best) { best = v; bi = p; }
            }
            const T mx = wave_max_dpp(best);
            const int pv = wave_min_dpp(best == mx ? bi : 0x7fffffff);
            const int pvt = (pv >= j && pv < n) ? pv : j;
            if (lane == 0 && pvt != j) {  // dlaqp2: swap the indices, carry the norms of position j to pvt
                const int t = jp[pvt]; jp[pvt] = jp[j]; jp[j] = t;
                vn1[pvt] = vn1[j];
                vn2[pvt] = vn2[j];
            }
        }
        __syncthreads();
        // ?larfg on column jp[j], rows j..m-1 (k_qr_pivot_reflect's formula)
        T *col = W + (size_t)jp[j] * ldw;
        const T alpha = col[j];
        T acc = 0;
        for (int i = j + 1 + tid; i < m; i += BID_THREADS) { const T v = col[i]; acc += v * v; }
        acc = wave_sum_dpp(acc);
        if (lane == 0) red[wv] = acc;
        __syncthreads();  // also orders every thread's read of alpha before the write of beta below
        const T xnorm = sqrt((red[0] + red[1]) + (red[2] + red[3]));
        T beta = alpha, tj = 0;
        if (xnorm != (T)0) {
            beta = -copysign(hypot(alpha, xnorm), alpha);
            const T scal = (T)1 / (alpha - beta);
            for (int i = j + 1 + tid; i < m; i += BID_THREADS) col[i] *= scal;
            tj = (beta - alpha) / beta;
            if (tid == 0) col[j] = beta;
        }
        // R_jj = beta decides the rank (qr.rs:187-200 as a ratio; uniform across the workgroup)
        if (j == 0) r00 = beta;
        if (beta == (T)0 || (tol > 0.0 && (double)fabs(beta / r00) < tol)) { r = j; break; }
        __syncthreads();
        if (j + 1 < n) {
            const int rem = m - j;
            if (rem <= 128) bid_apply<T, 2>(W, ldw, m, n, j, jp, vn1, vn2, tj, wv, lane);
            else if (rem <= 256) bid_apply<T, 4>(W, ldw, m, n, j, jp, vn1, vn2, tj, wv, lane);
            else bid_apply<T, 8>(W, ldw, m, n, j, jp, vn1, vn2, tj, wv, lane);
        }
        __syncthreads();
    }
    __syncthreads();
    return r;
}

// Z = [I | R11^-1 R12] P^T (k x n, rows r..k-1 zero) into Zb[i * zrs + c * zcs]: k_id_z's blocked back substitution with k -> r
// (16 x 16 tiles of R11 staged in LDS, one thread per right-hand side), each column written straight to its final place
template <typename T>
__device__ __forceinline__ void bid_z(const T *W, int ldw, int n, int r, int k, const int *jp, T (*tile)[BID_NB + 1], T *Zb, int64_t zrs, int64_t zcs, int tid) {
    const int nblk = (r + BID_NB - 1) / BID_NB;
    const int ti = tid / BID_NB, tk = tid % BID_NB;
    for (int q0 = 0; q0 < n; q0 += BID_THREADS) {
        const int p = q0 + tid;  // position in the pivoted order
        const bool inside = p < n;
        const int dc = inside ? jp[p] : 0;  // where column p of [I | R11^-1 R12] goes
        const bool active = inside && p >= r;
        T *zc = Zb + (int64_t)dc * zcs;
        if (inside) {
            if (p < r)
                for (int i = 0; i < k; ++i) zc[i * zrs] = (i == p) ? (T)1 : (T)0;
            else
                for (int i = r; i < k; ++i) zc[i * zrs] = (T)0;
        }
        const T *bcol = W + (size_t)dc * ldw;  // R12[:, p]: rows 0 .. r-1 of the physical column
        for (int bi = nblk - 1; bi >= 0; --bi) {
            const int r0 = bi * BID_NB;
            T acc[BID_NB];
#pragma unroll
            for (int ii = 0; ii < BID_NB; ++ii) acc[ii] = (active && r0 + ii < r) ? bcol[r0 + ii] : (T)0;
            for (int bj = nblk - 1; bj >= bi; --bj) {
                const int c0 = bj * BID_NB;
                __syncthreads();
                {
                    const int i = r0 + ti, l = c0 + tk;
                    tile[ti][tk] = (i < r && l < r && i <= l) ? W[(size_t)jp[l] * ldw + i] : (T)0;
                }
                __syncthreads();
                if (bj > bi) {
                    T x[BID_NB];
#pragma unroll
                    for (int jj = 0; jj < BID_NB; ++jj) x[jj] = (active && c0 + jj < r) ? zc[(c0 + jj) * zrs] : (T)0;  // this thread's own finished block
#pragma unroll
                    for (int jj = 0; jj < BID_NB; ++jj)
#pragma unroll
                        for (int ii = 0; ii < BID_NB; ++ii) acc[ii] -= tile[ii][jj] * x[jj];
                } else {
#pragma unroll
                    for (int ii = BID_NB - 1; ii >= 0; --ii) {
                        if (r0 + ii < r) {
                            acc[ii] /= tile[ii][ii];
#pragma unroll
                            for (int i2 = 0; i2 < ii; ++i2) acc[i2] -= tile[i2][ii] * acc[ii];
                        }
                    }
                }
            }
            if (active) {
#pragma unroll
                for (int ii = 0; ii < BID_NB; ++ii)
                    if (r0 + ii < r) zc[(r0 + ii) * zrs] = acc[ii];
            }
        }
    }
}

template <typename T, bool IN_LDS>
__global__ __launch_bounds__(BID_THREADS) void k_batched_id(Mat<T> a, int64_t abs, int count, int k, double tol, Mat<T> cm, int64_t cbs, Mat<T> z,
                                                            int64_t zbs, int64_t *__restrict__ col_ind, int64_t *__restrict__ ranks, T *__restrict__ ws) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const int m = (int)a.rows, n = (int)a.cols;
    const int ldw = IN_LDS ? (m | 1) : m;
    T *lds = reinterpret_cast<T *>(smem_raw);
    T *W = IN_LDS ? lds : ws + (size_t)blockIdx.x * (size_t)m * (size_t)n;
    T *vn1 = lds + (IN_LDS ? (size_t)n * ldw : 0);
    T *vn2 = vn1 + n;
    T(*tile)[BID_NB + 1] = reinterpret_cast<T(*)[BID_NB + 1]>(vn2 + n);
    T *red = vn2 + n + BID_NB * (BID_NB + 1);
    int *jp = reinterpret_cast<int *>(red + 8);
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;

    for (int b = blockIdx.x; b < count; b += gridDim.x) {
        const T *__restrict__ A = a.p + (int64_t)b * abs;
        bid_load(W, ldw, m, n, a.rs <= a.cs, [&](int i, int c) { return A[i * a.rs + c * a.cs]; }, vn1, vn2, jp, wv, lane);
        const int r = bid_qrcp(W, ldw, m, n, k, tol, jp, vn1, vn2, red, tid, wv, lane);

        // ---- outputs: permutation, rank, C, Z -------------------------------------------------------------------
        for (int p = tid; p < n; p += BID_THREADS) col_ind[(int64_t)b * n + p] = jp[p];
        if (tid == 0) ranks[b] = r;
        T *Cb = cm.p + (int64_t)b * cbs;
        for (int j = wv; j < k; j += BID_WAVES) {
            const T *src = A + (int64_t)jp[j] * a.cs;
            for (int i = lane; i < m; i += 64) Cb[i * cm.rs + j * cm.cs] = j < r ? src[i * a.rs] : (T)0;
        }
        bid_z(W, ldw, n, r, k, jp, tile, z.p + (int64_t)b * zbs, z.rs, z.cs, tid);
        __syncthreads();  // W, jp and the norms are rewritten by the next matrix
    }
}

// dynamic LDS of the two-sided kernel: [W: the larger of phase 1's n x (m|1) and phase 2's m x (k|1), LDS variant only]
// vn1[max(m, n)] vn2[max(m, n)] tile[16 x 17] red[8] | jp[n] jp2[m]
__host__ __device__ inline size_t bts_w_elems(int m, int n, int k) {
    const size_t w1 = (size_t)n * (size_t)(m | 1), w2 = (size_t)m * (size_t)(k | 1);
    return w1 > w2 ? w1 : w2;
}
template <typename T>
size_t bts_lds_bytes(int m, int n, int k, bool in_lds) {
    size_t t = (size_t)2 * std::max(m, n) + BID_NB * (BID_NB + 1) + 8;
    if (in_lds) t += bts_w_elems(m, n, k);
    return t * sizeof(T) + (size_t)(m + n) * sizeof(int);
}

// Two-sided ID A ~ C X R per matrix: phase 1 is k_batched_id's column ID (R = its Z, col_ind, the rank r); phase 2 is the column
// ID of C^T = A[:, col_ind[:r]]^T (r x m) at rank r with tol = 0, by the same three stages: its permutation is row_ind and its Z,
// written through c's transposed view, is c = Z2^T; X = A[row_ind[:r], col_ind[:r]] is gathered from the input.  In the workspace
// variant phase 2's m x r copy (ldw = r) fits the m x n slot; the LDS variant reserves the larger of the two phases' needs.
template <typename T, bool IN_LDS>
__global__ __launch_bounds__(BID_THREADS) void k_batched_two_sided(Mat<T> a, int64_t abs, int count, int k, double tol, Mat<T> cm, int64_t cbs,
                                                                   Mat<T> xm, int64_t xbs, Mat<T> z, int64_t zbs, int64_t *__restrict__ row_ind,
                                                                   int64_t *__restrict__ col_ind, int64_t *__restrict__ ranks, T *__restrict__ ws) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const int m = (int)a.rows, n = (int)a.cols, mn = m > n ? m : n;
    const int ldw = IN_LDS ? (m | 1) : m;
    T *lds = reinterpret_cast<T *>(smem_raw);
    T *W = IN_LDS ? lds : ws + (size_t)blockIdx.x * (size_t)m * (size_t)n;
    T *vn1 = lds + (IN_LDS ? bts_w_elems(m, n, k) : 0);
    T *vn2 = vn1 + mn;
    T(*tile)[BID_NB + 1] = reinterpret_cast<T(*)[BID_NB + 1]>(vn2 + mn);
    T *red = vn2 + mn + BID_NB * (BID_NB + 1);
    int *jp = reinterpret_cast<int *>(red + 8);  // phase 1's column permutation: read until X is gathered
    int *jp2 = jp + n;                           // phase 2's row permutation
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;

    for (int b = blockIdx.x; b < count; b += gridDim.x) {
        const T *__restrict__ A = a.p + (int64_t)b * abs;
        // ---- phase 1: column ID of A -> r (= Z), col_ind, the rank --------------------------------------------------
        bid_load(W, ldw, m, n, a.rs <= a.cs, [&](int i, int c) { return A[i * a.rs + c * a.cs]; }, vn1, vn2, jp, wv, lane);
        const int r = bid_qrcp(W, ldw, m, n, k, tol, jp, vn1, vn2, red, tid, wv, lane);
        for (int p = tid; p < n; p += BID_THREADS) col_ind[(int64_t)b * n + p] = jp[p];
        if (tid == 0) ranks[b] = r;
        bid_z(W, ldw, n, r, k, jp, tile, z.p + (int64_t)b * zbs, z.rs, z.cs, tid);
        __syncthreads();  // W and the norms are phase 2's from here

        // ---- phase 2: column ID of C^T (r x m), W2[p][i] = A[p, col_ind[i]] -> c = Z2^T, row_ind ------------------------
        const int ldw2 = IN_LDS ? (r | 1) : r;
        bid_load(W, ldw2, r, m, a.cs < a.rs, [&](int i, int p) { return A[p * a.rs + jp[i] * a.cs]; }, vn1, vn2, jp2, wv, lane);
        const int r2 = bid_qrcp(W, ldw2, r, m, r, 0.0, jp2, vn1, vn2, red, tid, wv, lane);  // r2 < r only on an exactly zero pivot
        for (int p = tid; p < m; p += BID_THREADS) row_ind[(int64_t)b * m + p] = jp2[p];
        bid_z(W, ldw2, m, r2, k, jp2, tile, cm.p + (int64_t)b * cbs, cm.cs, cm.rs, tid);  // Z2 (k x m) through c's transposed view

        // ---- X = A[row_ind[:r], col_ind[:r]], rows and columns r..k-1 zero --------------------------------------------------
        T *Xb = xm.p + (int64_t)b * xbs;
        for (int j = wv; j < k; j += BID_WAVES) {
            const T *src = A + (int64_t)jp[j] * a.cs;
            for (int i = lane; i < k; i += 64) Xb[i * xm.rs + j * xm.cs] = (i < r && j < r) ? src[jp2[i] * a.rs] : (T)0;
        }
        __syncthreads();  // W, jp, jp2 and the norms are rewritten by the next matrix
    }
}

}  // namespace

// persistent grid: the resident workgroups of every CU, fewer when the workspace (ws_per bytes per workgroup, 0 in the LDS variants)
// would pass 256 MiB unless that leaves less than one workgroup per CU; never more than count (shared with kernels_batched_id_c.hip)
int64_t bid_grid(rc_context *c, const void *kern, size_t lds, size_t ws_per, int32_t count) {
    static int cus_of[64] = {};
    int &cus = cus_of[c->device & 63];
    if (!cus && (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->device) != hipSuccess || cus <= 0)) cus = 256;
    int per_cu = 0;
    RC_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, BID_THREADS, lds));
    int64_t grid = (int64_t)cus * std::max(per_cu, 1);
    if (ws_per) grid = std::min<int64_t>(grid, std::max<int64_t>(cus, (int64_t)((size_t)256 << 20) / (int64_t)ws_per));
    return std::min<int64_t>(grid, count);
}

template <typename T>
void batched_column_id(rc_context *c, Mat<T> a, int64_t abs, int32_t count, int64_t k, double tol, Mat<T> cm, int64_t cbs, Mat<T> z, int64_t zbs,
                       int64_t *col_ind, int64_t *ranks) {
    const int m = (int)a.rows, n = (int)a.cols;
    if (count <= 0) return;
    ProfScope ps(c, "op:batched_column_id %dx%d k=%lld count=%d", m, n, (long long)k, (int)count);
    const size_t lds_in = bid_lds_bytes<T>(m, n, true);
    const bool in_lds = lds_in <= BID_MAX_LDS;
    const size_t lds = in_lds ? lds_in : bid_lds_bytes<T>(m, n, false);
    auto kern = in_lds ? k_batched_id<T, true> : k_batched_id<T, false>;
    static bool attr_set[64] = {};
    if (!attr_set[c->device & 63]) {
        RC_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(k_batched_id<T, true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)BID_MAX_LDS));
        RC_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(k_batched_id<T, false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)BID_MAX_LDS));
        attr_set[c->device & 63] = true;
    }
    const size_t per = (size_t)m * (size_t)n * sizeof(T);
    const int64_t grid = bid_grid(c, reinterpret_cast<const void *>(kern), lds, in_lds ? 0 : per, count);
    T *ws = in_lds ? nullptr : c->alloc<T>((size_t)grid * (size_t)m * (size_t)n);
    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(BID_THREADS), lds, c->stream, a, abs, (int)count, (int)k, tol, cm, cbs, z, zbs, col_ind, ranks, ws);
}

// the same grid and workspace rule; LDS or workspace chosen from the larger need of the two phases
template <typename T>
void batched_two_sided_id(rc_context *c, Mat<T> a, int64_t abs, int32_t count, int64_t k, double tol, Mat<T> cm, int64_t cbs, Mat<T> x, int64_t xbs,
                          Mat<T> z, int64_t zbs, int64_t *row_ind, int64_t *col_ind, int64_t *ranks) {
    const int m = (int)a.rows, n = (int)a.cols;
    if (count <= 0) return;
    ProfScope ps(c, "op:batched_two_sided_id %dx%d k=%lld count=%d", m, n, (long long)k, (int)count);
    const size_t lds_in = bts_lds_bytes<T>(m, n, (int)k, true);
    const bool in_lds = lds_in <= BID_MAX_LDS;
    const size_t lds = in_lds ? lds_in : bts_lds_bytes<T>(m, n, (int)k, false);
    auto kern = in_lds ? k_batched_two_sided<T, true> : k_batched_two_sided<T, false>;
    static bool attr_set[64] = {};
    if (!attr_set[c->device & 63]) {
        RC_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(k_batched_two_sided<T, true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)BID_MAX_LDS));
        RC_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(k_batched_two_sided<T, false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)BID_MAX_LDS));
        attr_set[c->device & 63] = true;
    }
    const size_t per = (size_t)m * (size_t)n * sizeof(T);
    const int64_t grid = bid_grid(c, reinterpret_cast<const void *>(kern), lds, in_lds ? 0 : per, count);
    T *ws = in_lds ? nullptr : c->alloc<T>((size_t)grid * (size_t)m * (size_t)n);
    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(BID_THREADS), lds, c->stream, a, abs, (int)count, (int)k, tol, cm, cbs, x, xbs, z, zbs, row_ind,
                       col_ind, ranks, ws);
}

template void batched_column_id<double>(rc_context *, Mat<double>, int64_t, int32_t, int64_t, double, Mat<double>, int64_t, Mat<double>, int64_t, int64_t *, int64_t *);
template void batched_column_id<float>(rc_context *, Mat<float>, int64_t, int32_t, int64_t, double, Mat<float>, int64_t, Mat<float>, int64_t, int64_t *, int64_t *);
template void batched_two_sided_id<double>(rc_context *, Mat<double>, int64_t, int32_t, int64_t, double, Mat<double>, int64_t, Mat<double>, int64_t,
                                           Mat<double>, int64_t, int64_t *, int64_t *, int64_t *);
template void batched_two_sided_id<float>(rc_context *, Mat<float>, int64_t, int32_t, int64_t, double, Mat<float>, int64_t, Mat<float>, int64_t,
                                          Mat<float>, int64_t, int64_t *, int64_t *, int64_t *);

}  // namespace rc
