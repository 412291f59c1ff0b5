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
        // ---- working copy (read in the input's fast direction) + initial column norms -----------------------------
        if (a.rs <= a.cs) {
            for (int c = wv; c < n; c += BID_WAVES)
                for (int i = lane; i < m; i += 64) W[(size_t)c * ldw + i] = A[i * a.rs + c * a.cs];
        } else {
            for (int i = wv; i < m; i += BID_WAVES)
                for (int c = lane; c < n; c += 64) W[(size_t)c * ldw + i] = A[i * a.rs + c * a.cs];
        }
        __syncthreads();
        for (int c = wv; c < n; c += BID_WAVES) {
            T acc = 0;
            for (int i = lane; i < m; i += 64) { const T v = W[(size_t)c * ldw + i]; acc += v * v; }
            acc = wave_sum_dpp(acc);
            if (lane == 0) { const T nr = sqrt(acc); vn1[c] = nr; vn2[c] = nr; jp[c] = c; }
        }
        __syncthreads();

        // ---- truncated pivoted QR, stopping at the rank -----------------------------------------------------------
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

        // ---- outputs: permutation, rank, C, Z -------------------------------------------------------------------
        for (int p = tid; p < n; p += BID_THREADS) col_ind[(int64_t)b * n + p] = jp[p];
        if (tid == 0) ranks[b] = r;
        T *Cb = cm.p + (int64_t)b * cbs;
        for (int j = wv; j < k; j += BID_WAVES) {
            const T *src = A + (int64_t)jp[j] * a.cs;
            for (int i = lane; i < m; i += 64) Cb[i * cm.rs + j * cm.cs] = j < r ? src[i * a.rs] : (T)0;
        }
        // Z = [I | R11^-1 R12] P^T: k_id_z with k -> r, rows r..k-1 zero
        T *Zb = z.p + (int64_t)b * zbs;
        const int nblk = (r + BID_NB - 1) / BID_NB;
        const int ti = tid / BID_NB, tk = tid % BID_NB;
        for (int q0 = 0; q0 < n; q0 += BID_THREADS) {
            const int p = q0 + tid;  // position in the pivoted order
            const bool inside = p < n;
            const int dc = inside ? jp[p] : 0;  // where column p of [I | R11^-1 R12] goes
            const bool active = inside && p >= r;
            T *zc = Zb + (int64_t)dc * z.cs;
            if (inside) {
                if (p < r)
                    for (int i = 0; i < k; ++i) zc[i * z.rs] = (i == p) ? (T)1 : (T)0;
                else
                    for (int i = r; i < k; ++i) zc[i * z.rs] = (T)0;
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
                        for (int jj = 0; jj < BID_NB; ++jj) x[jj] = (active && c0 + jj < r) ? zc[(c0 + jj) * z.rs] : (T)0;  // this thread's own finished block
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
                        if (r0 + ii < r) zc[(r0 + ii) * z.rs] = acc[ii];
                }
            }
        }
        __syncthreads();  // W, jp and the norms are rewritten by the next matrix
    }
}

}  // namespace

template <typename T>
void batched_column_id(rc_context *c, Mat<T> a, int64_t abs, int32_t count, int64_t k, double tol, Mat<T> cm, int64_t cbs, Mat<T> z, int64_t zbs,
                       int64_t *col_ind, int64_t *ranks) {
    const int m = (int)a.rows, n = (int)a.cols;
    if (count <= 0) return;
    ProfScope ps(c, "op:batched_column_id %dx%d k=%lld count=%d", m, n, (long long)k, (int)count);
    static int cus_of[64] = {};
    int &cus = cus_of[c->device & 63];
    if (!cus && (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->device) != hipSuccess || cus <= 0)) cus = 256;
    constexpr size_t kMaxLds = 160 * 1024 - 1024;
    const size_t lds_in = bid_lds_bytes<T>(m, n, true);
    const bool in_lds = lds_in <= kMaxLds;
    const size_t lds = in_lds ? lds_in : bid_lds_bytes<T>(m, n, false);
    auto kern = in_lds ? k_batched_id<T, true> : k_batched_id<T, false>;
    static bool attr_set[64] = {};
    if (!attr_set[c->device & 63]) {
        RC_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(k_batched_id<T, true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kMaxLds));
        RC_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(k_batched_id<T, false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kMaxLds));
        attr_set[c->device & 63] = true;
    }
    int per_cu = 0;
    RC_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, reinterpret_cast<const void *>(kern), BID_THREADS, lds));
    int64_t grid = (int64_t)cus * std::max(per_cu, 1);
    T *ws = nullptr;
    if (!in_lds) {  // one working copy per workgroup; at most 256 MiB of them unless that leaves less than one workgroup per CU
        const size_t per = (size_t)m * (size_t)n * sizeof(T);
        grid = std::min<int64_t>(grid, std::max<int64_t>(cus, (int64_t)((size_t)256 << 20) / (int64_t)per));
    }
    grid = std::min<int64_t>(grid, count);
    if (!in_lds) ws = c->alloc<T>((size_t)grid * (size_t)m * (size_t)n);
    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(BID_THREADS), lds, c->stream, a, abs, (int)count, (int)k, tol, cm, cbs, z, zbs, col_ind, ranks, ws);
}

template void batched_column_id<double>(rc_context *, Mat<double>, int64_t, int32_t, int64_t, double, Mat<double>, int64_t, Mat<double>, int64_t, int64_t *, int64_t *);
template void batched_column_id<float>(rc_context *, Mat<float>, int64_t, int32_t, int64_t, double, Mat<float>, int64_t, Mat<float>, int64_t, int64_t *, int64_t *);

}  // namespace rc
