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
//
// Batched truncated SVD (rc_svd_rank_batched_*): k_batched_svd, the same grid and the same first two stages run to all N steps,
// then one-sided Jacobi on the transposed triangular factor and U formed from the kept reflectors (see its comment below).
//
// Batched recompression (rc_lowrank_recompress_batched_*): k_batched_recompress, the same grid and stages on the two thin factors of
// a low-rank block, the same Jacobi on their small core, both Q's applied by the same reflector routine (see its comment below).
//
// Tall left factors (rc_lowrank_recompress_tall_batched_*, m <= 65536): k_batched_recompress<T, true>, the same kernel text with the left
// factor taken through a flat Householder TSQR in stages of 512 rows kept in the workgroup's slot (see "tall left factors" below).
//
// Both factors tall (rc_lowrank_recompress_large_batched_*, m, n <= 65536): k_batched_recompress<T, true, true>, the right factor through
// the same stages behind the left factor's in the slot, vt formed down them with u's signs (see "both factors tall" below).
//
// Batched sketched column ID (rc_sketch_column_id_rank_batched_*): k_batched_sketch_id, the same grid; the working copy is the sketch
// Omega A (l x n, l <= 128) formed by MFMA while A streams through LDS once, then the same stages on l rows (see its comment below).
//
// Batched range step (rc_sketch_range_step_batched_*): k_batched_range_step, the same grid; that sketch stored as Y^T, its pivoted QR run to
// all l steps, Q formed explicitly and the projection A Q^T by the sketch routine on A's transposed view (see its comment below).
//
// The stages that read the same for real and complex elements stand once in batched_stages.hpp, as templates over the element type that
// this file instantiates for double and float: the fill, the norms and their power-of-two normalisation, the pivoted-QR step loop bid_qrcp,
// the back substitution bid_z, k_batched_id and k_batched_two_sided with their LDS carve-up and plans, the Jacobi schedule
// bsv_jacobi and brt_stack_load.  Here stay the real family's own routines (bid_apply, bsv_round, bsv_sign, the form_u routines, the core
// products) and the SVD, recompression, sketch and range-step kernels.
//
// The launchers follow rc_batched_launch.hpp: a plan function per entry point, then prepare, label, workspace, launch.  All but the sketch
// product's are written once for all four element types in batched_launchers.hpp; the file ends with what they take from this family
// (RealFamily: the Args structs, the LDS and workspace sizes and the instance to launch) and their instantiation for double and float.
// bid_grid and the first-use LDS cap of the whole batched family are defined in rc_launch.hip.
#include "batched_launchers.hpp"
#include "batched_stages.hpp"
#include "rc_batched_launch.hpp"
#include "rc_common.hpp"
#include "rc_device.hpp"
#include "rc_gemm.hpp"

namespace rc {

namespace {

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

// ---- batched truncated SVD (rc_svd_rank_batched_*) -----------------------------------------------------------------------------
// Per matrix, in the tall orientation M x N (N = min(m, n); a wide matrix is read through its transposed view): the pivoted QR of
// bid_qrcp run to N steps (W P = Q R, reflectors kept), one-sided Jacobi on the N x N core G = R^T with the rotations accumulated
// in J (R^T J = V_R Sigma, so J = U_R), singular values = the column norms of G, then U = Q [J_k; 0] with the k kept columns in
// registers and V_R = G Sigma^-1, whose rows the pivoted QR permutes: V_W[jp[i], :] = V_R[i, :].  Jacobi on R^T, the rows of the
// pivoted R, rather than on its columns: R's rows are graded by the pivoting, R^T's columns are then nearly orthogonal and the
// sweeps converge in a few rounds (Drmac & Veselic's preconditioning); on R's columns the 128 x 128 bench matrices used up the
// 30-sweep budget.  Everything stays inside one workgroup.

// Jacobi rows per lane of a 16-lane pair group (N <= 16 NE) and rows per lane of a 64-lane U column (M <= 64 NE)
// (both threshold tests are evaluated in f64, so that in f32 two columns of norm 1e-9 or less, whose app aqq and apq^2 pass the
// smallest f32 number, are still rotated until they are orthogonal: jacobi_pair_is_coupled, rc_device.hpp)
template <typename T, int NE>
__device__ __forceinline__ void bsv_round(T *G, int ldg, T *J, int ldj, int N, int p, int q, T tol, T tol2, int ll, int *flag) {
    T *gp = G + (size_t)p * ldg, *gq = G + (size_t)q * ldg;
    T a[NE], b[NE];
    T app = 0, aqq = 0, apq = 0;
#pragma unroll
    for (int e = 0; e < NE; ++e) {
        const int i = ll + 16 * e;
        a[e] = i < N ? gp[i] : (T)0;
        b[e] = i < N ? gq[i] : (T)0;
        app = fma(a[e], a[e], app);
        aqq = fma(b[e], b[e], aqq);
        apq = fma(a[e], b[e], apq);
    }
    app = group_sum_dpp<16>(app);
    aqq = group_sum_dpp<16>(aqq);
    apq = group_sum_dpp<16>(apq);
    // k_jacobi_lds's test and thresholds: rotate iff |apq| > tol sqrt(app aqq) (uniform over the 16 lanes)
    const double apq2 = (double)apq * (double)apq;
    if (!jacobi_pair_is_coupled(app, aqq, apq2, tol2)) return;
    T c, s;
    jacobi_rotation(app, aqq, apq, c, s);
    T *vp = J + (size_t)p * ldj, *vq = J + (size_t)q * ldj;
#pragma unroll
    for (int e = 0; e < NE; ++e) {
        const int i = ll + 16 * e;
        if (i < N) {
            gp[i] = c * a[e] - s * b[e];
            gq[i] = s * a[e] + c * b[e];
            const T x = vp[i], y = vq[i];
            vp[i] = c * x - s * y;
            vq[i] = s * x + c * y;
        }
    }
    if (ll == 0 && jacobi_rotation_was_large(app, aqq, apq2, s, tol)) *flag = 2;  // plain store: every writer writes 2
}

// sign of a column held by one wave (value x[e] at output row orow(e)): -1 when its largest-|.| entry (the first such in output row
// order) is negative, else +1 (also when every entry is NaN)
template <typename T, int NE, typename Row>
__device__ __forceinline__ int bsv_sign(const T (&x)[NE], Row orow) {
    T mx = 0;
#pragma unroll
    for (int e = 0; e < NE; ++e) mx = max(mx, fabs(x[e]));
    mx = wave_max_dpp(mx);
    int key = 0x7fffffff;
#pragma unroll
    for (int e = 0; e < NE; ++e) {
        const int o = orow(e);
        if (o >= 0 && fabs(x[e]) == mx) key = min(key, 2 * o + (x[e] < (T)0 ? 1 : 0));
    }
    key = wave_min_dpp(key);
    return (key != 0x7fffffff && (key & 1)) ? -1 : 1;
}

// U[:, c] = sgn[c] Q [J[:, srt[c]]; 0] for the kept columns c < r (zero for r <= c < k): one wave per column, the M rows in
// registers (row lane + 64 e), the N reflectors applied backward, H_j = I - tau_j v_j v_j^T with v_j in W's column jp[j] below row j
template <typename T, int NE>
__device__ __forceinline__ void bsv_form_u(const T *W, int ldw, const T *J, int ldj, int M, int N, int k, int r, const int *jp, const T *taus,
                                           const int *srt, int *sgn, bool sign_here, T *U, int64_t urs, int64_t ucs, int wv, int lane) {
    for (int c = wv; c < k; c += BID_WAVES) {
        T *uc = U + (int64_t)c * ucs;
        if (c >= r) {
            for (int i = lane; i < M; i += 64) uc[i * urs] = (T)0;
            continue;
        }
        const T *jc = J + (size_t)srt[c] * ldj;
        T x[NE];
#pragma unroll
        for (int e = 0; e < NE; ++e) {
            const int i = lane + 64 * e;
            x[e] = i < N ? jc[i] : (T)0;
        }
        for (int j = N - 1; j >= 0; --j) {
            const T tau = taus[j];
            if (tau == (T)0) continue;  // H_j = I (uniform)
            const T *vc = W + (size_t)jp[j] * ldw;
            T v[NE];
            T dot = 0;
#pragma unroll
            for (int e = 0; e < NE; ++e) {
                const int i = lane + 64 * e;
                const T vv = vc[i < M ? i : j];  // branch-free: lanes out of range read row j and are masked below
                v[e] = i > j && i < M ? vv : (i == j ? (T)1 : (T)0);
                dot = fma(v[e], x[e], dot);
            }
            const T f = tau * wave_sum_dpp(dot);
#pragma unroll
            for (int e = 0; e < NE; ++e) x[e] = fma(-f, v[e], x[e]);
        }
        if (sign_here) {
            const int s = bsv_sign<T, NE>(x, [&](int e) { const int i = lane + 64 * e; return i < M ? i : -1; });
            if (lane == 0) sgn[c] = s;
#pragma unroll
            for (int e = 0; e < NE; ++e) x[e] = s < 0 ? -x[e] : x[e];
        } else if (sgn[c] < 0) {
#pragma unroll
            for (int e = 0; e < NE; ++e) x[e] = -x[e];
        }
#pragma unroll
        for (int e = 0; e < NE; ++e) {
            const int i = lane + 64 * e;
            if (i < M) uc[i * urs] = x[e];
        }
    }
}

// LDS of k_batched_svd: [W: N x (M|1), W_LDS only] G: N x ldg [J: N x ldg, V_LDS only] vn1[N] vn2[N] taus[N] sig[N] red[8]
// | jp[N] srt[N] sgn[128] flag[4] (ints last: the T arrays stay aligned)
template <typename T>
size_t bsv_lds_bytes(int M, int N, int ldg, bool w_lds, bool v_lds) {
    size_t t = (size_t)N * ldg + 4 * (size_t)N + 8;
    if (w_lds) t += (size_t)N * (size_t)(M | 1);
    if (v_lds) t += (size_t)N * ldg;
    return t * sizeof(T) + (size_t)(2 * N + 128 + 4) * sizeof(int);
}

// a: m x n input view; uo (M x k) and vo (k x N) are the views the work orientation's U and V^T go to (u and vt for a tall matrix,
// vt^T and u^T for a wide one), each moved by its own batch stride; s (count x N) and ranks contiguous.  W_LDS / V_LDS: the working
// copy W / the rotations J (the singular vectors of R) live in LDS, else in the workgroup's workspace slot; the core G is in LDS.
template <typename T, bool W_LDS, bool V_LDS>
__global__ __launch_bounds__(BID_THREADS) void k_batched_svd(Mat<T> a, int64_t abs, int count, int k, double tol, Mat<T> uo, int64_t ubs, Mat<T> vo, int64_t vbs,
                                                             T *__restrict__ s_out, int64_t *__restrict__ ranks, T *__restrict__ ws, int *health, int ldg) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const bool wide = a.rows < a.cols;
    const int M = (int)(wide ? a.cols : a.rows), N = (int)(wide ? a.rows : a.cols);
    const int ldw = W_LDS ? (M | 1) : M, ldj = V_LDS ? ldg : N;
    T *lds = reinterpret_cast<T *>(smem_raw);
    T *wsb = ws + (size_t)blockIdx.x * ((W_LDS ? 0 : (size_t)M * N) + (V_LDS ? 0 : (size_t)N * N));
    T *W = W_LDS ? lds : wsb;
    T *G = lds + (W_LDS ? (size_t)N * ldw : 0);
    T *J = V_LDS ? G + (size_t)N * ldg : wsb + (W_LDS ? 0 : (size_t)M * N);
    T *vn1 = G + (size_t)N * ldg + (V_LDS ? (size_t)N * ldg : 0);
    T *vn2 = vn1 + N, *taus = vn2 + N, *sig = taus + N, *red = sig + N;
    int *jp = reinterpret_cast<int *>(red + 8);
    int *srt = jp + N, *sgn = srt + N, *flag = sgn + 128;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    // the input in the work orientation and its fast direction
    const int64_t ars = wide ? a.cs : a.rs, acs = wide ? a.rs : a.cs;

    for (int b = blockIdx.x; b < count; b += gridDim.x) {
        const T *__restrict__ A = a.p + (int64_t)b * abs;
        // ---- QR: W P = Q R, all N steps (exact zero pivots are steps with H = I), taus kept -------------------------------------
        const int e2 = bid_load_pow2(W, ldw, M, N, ars <= acs, [&](int i, int c) { return A[i * ars + c * acs]; }, vn1, vn2, jp, red + 4, wv, lane);
        bid_qrcp<T, true>(W, ldw, M, N, N, 0.0, jp, vn1, vn2, red, tid, wv, lane, taus);
        // ---- core G = R^T (R in pivoted column order: G[:, j] = row j of R) and J = I ------------------------------------------
        for (int j = wv; j < N; j += BID_WAVES) {
            for (int i = lane; i < N; i += 64) {
                G[(size_t)j * ldg + i] = i >= j ? W[(size_t)jp[i] * ldw + j] : (T)0;
                J[(size_t)j * ldj + i] = i == j ? (T)1 : (T)0;
            }
        }
        __syncthreads();
        bool conv;
        if (N <= 16) conv = bsv_jacobi<T, 1>(G, ldg, J, ldj, N, tid, flag);
        else if (N <= 32) conv = bsv_jacobi<T, 2>(G, ldg, J, ldj, N, tid, flag);
        else if (N <= 64) conv = bsv_jacobi<T, 4>(G, ldg, J, ldj, N, tid, flag);
        else conv = bsv_jacobi<T, 8>(G, ldg, J, ldj, N, tid, flag);
        if (!conv && tid == 0) atomicOr(health, 16);  // the sweep budget ran out: bit 16, as the lone Jacobi reports it
        // ---- singular values: column norms, sorted descending (a strict total order: NaN last, ties by column) ----------------------
        for (int j = tid >> 4; j < N; j += BID_THREADS / 16) {
            const T *gj = G + (size_t)j * ldg;
            T acc = 0;
            for (int i = tid & 15; i < N; i += 16) acc = fma(gj[i], gj[i], acc);
            acc = group_sum_dpp<16>(acc);
            if ((tid & 15) == 0) sig[j] = sqrt(acc);
        }
        __syncthreads();
        T *sb = s_out + (int64_t)b * N;
        for (int i = tid; i < N; i += BID_THREADS) {
            const T ki = sig[i] >= (T)0 ? sig[i] : (T)-1;
            int pos = 0;
            for (int j = 0; j < N; ++j) {
                const T kj = sig[j] >= (T)0 ? sig[j] : (T)-1;
                pos += (kj > ki || (kj == ki && j < i)) ? 1 : 0;
            }
            srt[pos] = i;
            sb[pos] = ldexp(sig[i], e2);  // W was 2^-e2 times the block: the one output that carries its scale
        }
        __syncthreads();
        // ---- rank: the first j < k with s_j == 0 or (tol > 0 and s_j / s_0 < tol), else k ---------------------------------------
        if (tid == 0) {
            const T s0 = sig[srt[0]];
            int r = k;
            for (int j = 0; j < k; ++j) {
                const T sj = sig[srt[j]];
                if (sj == (T)0 || (tol > 0.0 && (double)(sj / s0) < tol)) { r = j; break; }
            }
            flag[1] = r;
            ranks[b] = r;
        }
        __syncthreads();
        const int r = flag[1];
        // ---- signs: the largest-|.| entry of each kept column of the caller's u is positive --------------------------------------
        // (a wide matrix's u is V = G Sigma^-1: its signs are fixed here, before U is formed; a tall one's in bsv_form_u)
        if (wide) {
            for (int c = wv; c < r; c += BID_WAVES) {
                const T *gc = G + (size_t)srt[c] * ldg;
                const T sj = sig[srt[c]], inv = sj > (T)0 ? (T)1 / sj : (T)0;
                T x[2];
                for (int e = 0; e < 2; ++e) {
                    const int i = lane + 64 * e;
                    x[e] = i < N ? gc[i] * inv : (T)0;
                }
                const int sg = bsv_sign<T, 2>(x, [&](int e) { const int i = lane + 64 * e; return i < N ? jp[i] : -1; });
                if (lane == 0) sgn[c] = sg;
            }
            __syncthreads();
        }
        // ---- U = Q [J_k; 0] straight into the output view -------------------------------------------------------------------------
        T *Ub = uo.p + (int64_t)b * ubs;
        if (M <= 64) bsv_form_u<T, 1>(W, ldw, J, ldj, M, N, k, r, jp, taus, srt, sgn, !wide, Ub, uo.rs, uo.cs, wv, lane);
        else if (M <= 128) bsv_form_u<T, 2>(W, ldw, J, ldj, M, N, k, r, jp, taus, srt, sgn, !wide, Ub, uo.rs, uo.cs, wv, lane);
        else if (M <= 256) bsv_form_u<T, 4>(W, ldw, J, ldj, M, N, k, r, jp, taus, srt, sgn, !wide, Ub, uo.rs, uo.cs, wv, lane);
        else bsv_form_u<T, 8>(W, ldw, J, ldj, M, N, k, r, jp, taus, srt, sgn, !wide, Ub, uo.rs, uo.cs, wv, lane);
        __syncthreads();  // sgn of a tall matrix is written above
        // ---- V^T: row c of vo is sgn[c] V_W[:, c], V_W[jp[i], c] = V_R[i, c] = G[i, srt[c]] / s_c; rows r..k-1 zero ---------------
        T *Vb = vo.p + (int64_t)b * vbs;
        for (int c = wv; c < k; c += BID_WAVES) {
            const int j0 = c < r ? srt[c] : 0;
            const T *gc = G + (size_t)j0 * ldg;
            const T sj = sig[j0], inv = c < r && sj > (T)0 ? (sgn[c] < 0 ? (T)-1 : (T)1) / sj : (T)0;
            for (int i = lane; i < N; i += 64) Vb[c * vo.rs + (int64_t)jp[i] * vo.cs] = gc[i] * inv;
        }
        __syncthreads();  // W, G, J and the small arrays are rewritten by the next matrix
    }
}

// ---- batched recompression of low-rank factors (rc_lowrank_recompress_batched_*) -----------------------------------------------
// Per block, with q = in_ranks[b] clamped to [0, K]: A = left[:, :q] mid[:q, :q] diag(s[:q]) right[:q, :] is never formed.  The two
// thin factors are factored where they stand, left[:, :q] P_L = Q_L R_L and right[:q, :]^T P_R = Q_R R_R (bid_qrcp to q steps each,
// reflectors kept), so A = Q_L C Q_R^T with the q x q core C = R_L P_L^T mid diag(s) P_R^T R_R^T; the rest is k_batched_svd on the
// core: one-sided Jacobi on G = C^T with the rotations in J (C^T J = V_c Sigma, J = U_c), singular values = the column norms of G,
// U = Q_L [U_c; 0] and V = Q_R [V_c; 0] by backward reflector application straight into the output views.  O((m + n) q^2) work.
// G = C^T, not C: an exactly zero column of left is pivoted last and is a step with H = I, which leaves a zero row in R_L, hence a
// zero row of C = a zero column of G, and the rotation test (apq^2 > tol^2 app aqq, false for apq = 0) never touches a zero column:
// its singular value comes out as exactly 0.
//
// The core is formed by two q x q x q products in LDS, one thread per element, summed over the inner index in ascending order:
//   T1[a, j] = sum_b mid[a, b] s[b] Rr[j, b]   (T1 in J's place: J = I only afterwards)
//   C[i, j]  = sum_a Rl[i, a] T1[a, j]         (stored as G[i * ldg + j]: column i of G = row i of C)
// where Rl[:, c] is the upper-triangular column R_L P_L^T keeps for the factor's own column c (rows 0 .. ip[c] of the working copy's
// column c, ip the inverse of the pivot order), Rr likewise.  The lanes run along j: T1, Wr and G are read and written at consecutive
// addresses and mid[a, b], Rl[i, a] are one broadcast address per wave.

template <typename T>
struct BrcArgs {
    Mat<T> left, mid, right, u, vt;
    int64_t lbs, mbs, rbs, ubs, vbs, s_stride;
    const T *s;
    const int64_t *in_ranks;
    T *s_out;
    int64_t *ranks;
    T *ws;
    int *health;
    double tol;
    int count, k, ldg;
    bool l_lds, r_lds, v_lds;  // the copy of left / of right^T / the rotations J in LDS (else in the workgroup's workspace slot)
};

// LDS: [Wl: K x (m|1)] [Wr: K x (n|1)] G: K x ldg [J: K x ldg] vn1[K] vn2[K] taul[K] taur[K] sig[K] red[8]
// | jpl[K] jpr[K] ipl[K] ipr[K] srt[K] sgn[128] flag[4] (ints last: the T arrays stay aligned)
template <typename T>
size_t brc_lds_bytes(int m, int n, int K, int ldg, bool l_lds, bool r_lds, bool v_lds) {
    size_t t = (size_t)K * ldg + 5 * (size_t)K + 8;
    if (l_lds) t += (size_t)K * (size_t)(m | 1);
    if (r_lds) t += (size_t)K * (size_t)(n | 1);
    if (v_lds) t += (size_t)K * ldg;
    return t * sizeof(T) + (size_t)(5 * K + 128 + 4) * sizeof(int);
}
__host__ __device__ inline size_t brc_ws_elems(int m, int n, int K, bool l_lds, bool r_lds, bool v_lds) {
    return (l_lds ? 0 : (size_t)m * K) + (r_lds ? 0 : (size_t)n * K) + (v_lds ? 0 : (size_t)K * K);
}

// ---- tall left factors (rc_lowrank_recompress_tall_batched_*, m <= 65536) ----------------------------------------------------------
// left[:, :q] is factored by a flat Householder TSQR with stored reflectors, still inside one workgroup.  Stage 0 is the factorization
// above on rows 0 .. min(m, H) - 1, H = BRT_H = 512 rows (what bid_qrcp and bsv_reflect_back<T, 8> hold).  Stage s >= 1 factors a stack:
// the upper triangle of the previous stage's R (q rows, zeros below the diagonal) on top of the next min(H - q, rows left) rows of left,
// the columns in the cumulative pivot order, by the same q pivoted steps; an exactly zero column of left is an exactly zero column of every
// stack, so it stays a step with H = I and a zero row of the last R.  A stack's column for the factor's column c is stored at physical
// column c, and jp (position -> physical column) is carried from stage to stage instead of being reset: after the last stage it is the
// cumulative permutation, and (the last stage's copy, jp) stand where (Wl, jpl) stand in the core products.  The stage height depends on
// q, not on K: a block's bits are those of a call of inner width q.  Every stage's factored copy, taus and pivots stay in the
// workgroup's workspace slot (brt_stage_elems each) for the backward pass, brt_form_u.  m <= H is one stage and the kernel above.
// (BRT_H, brt_stages, brt_stage_elems and the grid bound brt_grid_cap are in rc_batched_launch.hpp, shared with the complex kernel.)
// the slot: the stage copies of the widest inner rank first (m > H; brc_ws_elems' copy of left otherwise), then brc_ws_elems' other parts
__host__ __device__ inline size_t brt_ws_elems(int m, int n, int K, bool l_lds, bool r_lds, bool v_lds) {
    if (m <= BRT_H) return brc_ws_elems(m, n, K, l_lds, r_lds, v_lds);
    return (size_t)brt_stages(m, K) * brt_stage_elems(K) + brc_ws_elems(0, n, K, true, r_lds, v_lds);
}

// x <- H_0 .. H_{N-1} x for a column held by one wave (row lane + 64 e in x[e], M rows): bsv_form_u's reflector loop as a routine of its
// own, for a column that goes through several factorizations (bsv_form_u keeps its loop: sharing this one changed k_batched_svd's stream)
template <typename T, int NE>
__device__ __forceinline__ void bsv_reflect_back(const T *W, int ldw, int M, int N, const int *jp, const T *taus, T (&x)[NE], int lane) {
    for (int j = N - 1; j >= 0; --j) {
        const T tau = taus[j];
        if (tau == (T)0) continue;  // H_j = I (uniform)
        const T *vc = W + (size_t)jp[j] * ldw;
        T v[NE];
        T dot = 0;
#pragma unroll
        for (int e = 0; e < NE; ++e) {
            const int i = lane + 64 * e;
            const T vv = vc[i < M ? i : j];  // branch-free: lanes out of range read row j and are masked below
            v[e] = i > j && i < M ? vv : (i == j ? (T)1 : (T)0);
            dot = fma(v[e], x[e], dot);
        }
        const T f = tau * wave_sum_dpp(dot);
#pragma unroll
        for (int e = 0; e < NE; ++e) x[e] = fma(-f, v[e], x[e]);
    }
}

// U[:, c] = sgn[c] Q_0 [Q_1 [.. Q_{S-1} [J[:, srt[c]]; 0] ..; 0]; 0] for S >= 2 stages at stage0 + s * se: one wave per column carries x (q
// values) down the stages.  Stage s >= 1 applies its reflectors to [x; 0] (H rows in registers); rows q .. of the result are that chunk's
// rows of u, rows 0 .. q - 1 replace x; stage 0's result fills rows 0 .. H - 1.  The sign rule runs over all m rows: per chunk the
// largest |.| and its first row (bsv_sign's key), the larger magnitude wins and on a tie the smaller row, which is the later chunk seen.
// Stage 0's rows are written with the final sign; the wave then negates the rows it wrote before, each lane its own addresses.
template <typename T>
__device__ __forceinline__ void brt_form_u(const T *stage0, size_t se, int S, int K, int q, int m, const T *J, int ldj, int k, int r, const int *srt, int *sgn,
                                           T *U, int64_t urs, int64_t ucs, int wv, int lane) {
    constexpr int NE = BRT_H / 64;
    for (int c = wv; c < k; c += BID_WAVES) {
        T *uc = U + (int64_t)c * ucs;
        if (c >= r) {
            for (int i = lane; i < m; i += 64) uc[i * urs] = (T)0;
            continue;
        }
        const T *jc = J + (size_t)srt[c] * ldj;
        T x[NE];
#pragma unroll
        for (int e = 0; e < NE; ++e) {
            const int i = lane + 64 * e;
            x[e] = i < q ? jc[i] : (T)0;
        }
        T best = (T)-1;
        int bkey = 0x7fffffff;
        for (int s = S - 1; s >= 0; --s) {
            const T *Ws = stage0 + (size_t)s * se, *ts = Ws + (size_t)BRT_H * K;
            const int top = s ? q : 0, base = s ? BRT_H + (s - 1) * (BRT_H - q) : 0;
            const int hs = top + min(BRT_H - top, m - base);
            bsv_reflect_back<T, NE>(Ws, BRT_H, hs, q, reinterpret_cast<const int *>(ts + K), ts, x, lane);
            T mx = 0;
#pragma unroll
            for (int e = 0; e < NE; ++e) {
                const int i = lane + 64 * e;
                if (i >= top && i < hs) mx = max(mx, fabs(x[e]));
            }
            mx = wave_max_dpp(mx);
            int key = 0x7fffffff;
#pragma unroll
            for (int e = 0; e < NE; ++e) {
                const int i = lane + 64 * e;
                if (i >= top && i < hs && fabs(x[e]) == mx) key = min(key, 2 * (base + i - top) + (x[e] < (T)0 ? 1 : 0));
            }
            key = wave_min_dpp(key);
            if (key != 0x7fffffff && mx >= best) { best = mx; bkey = key; }  // this chunk's rows precede every chunk seen so far
            if (s) {
#pragma unroll
                for (int e = 0; e < NE; ++e) {
                    const int i = lane + 64 * e;
                    if (i >= top && i < hs) uc[(int64_t)(base + i - top) * urs] = x[e];
                    x[e] = i < top ? x[e] : (T)0;
                }
            }
        }
        const bool neg = bkey != 0x7fffffff && (bkey & 1);
        if (lane == 0) sgn[c] = neg ? -1 : 1;
#pragma unroll
        for (int e = 0; e < NE; ++e) {
            const int i = lane + 64 * e;
            uc[(int64_t)i * urs] = neg ? -x[e] : x[e];  // stage 0 of S >= 2 stages holds H rows
        }
        if (neg) {
            for (int s = 1; s < S; ++s) {
                const int base = BRT_H + (s - 1) * (BRT_H - q), rows = min(BRT_H - q, m - base);
                for (int i = lane; i < rows; i += 64) {
                    T *p = uc + (int64_t)(base + i) * urs;
                    *p = -*p;
                }
            }
        }
    }
}

// ---- both factors tall (rc_lowrank_recompress_large_batched_*, m, n <= 65536) -------------------------------------------------------
// right[:q, :]^T (n x q) goes through the scheme above when n > H: the same stages, jpr carried from stage to stage, every stage's copy,
// taus and pivots in the workgroup's slot behind the left factor's part; (the last stage's copy, jpr) stand where (Wr, jpr) stand in T1.
// n <= H is the tall call itself: the launcher runs k_batched_recompress<T, true> under the tall call's plan, so the bits are that call's.
// the slot: the left factor's part (stage copies for m > H, brc_ws_elems' copy otherwise), the right factor's stage copies, then J
__host__ __device__ inline size_t brl_ws_elems(int m, int n, int K, bool l_lds, bool r_lds, bool v_lds) {
    if (n <= BRT_H) return brt_ws_elems(m, n, K, l_lds, r_lds, v_lds);
    return brt_ws_elems(m, 0, K, l_lds, true, true) + (size_t)brt_stages(n, K) * brt_stage_elems(K) + (v_lds ? 0 : (size_t)K * K);
}

// V[:, c] = sgn[c] Q_0 [Q_1 [.. Q_{S-1} [Vc[:, srt[c]]; 0] ..; 0]; 0] for S >= 2 stages of the right factor: brt_form_u with the signs
// already fixed on u, so every chunk is written once with its sign and no row is visited twice.  V is vt's transposed view (n x k).
template <typename T>
__device__ __forceinline__ void brl_form_vt(const T *stage0, size_t se, int S, int K, int q, int n, const T *Vc, int ldv, int k, int r, const int *srt,
                                            const int *sgn, T *V, int64_t vrs, int64_t vcs, int wv, int lane) {
    constexpr int NE = BRT_H / 64;
    for (int c = wv; c < k; c += BID_WAVES) {
        T *vc = V + (int64_t)c * vcs;
        if (c >= r) {
            for (int i = lane; i < n; i += 64) vc[i * vrs] = (T)0;
            continue;
        }
        const T *gc = Vc + (size_t)srt[c] * ldv;
        const bool neg = sgn[c] < 0;
        T x[NE];
#pragma unroll
        for (int e = 0; e < NE; ++e) {
            const int i = lane + 64 * e;
            x[e] = i < q ? gc[i] : (T)0;
        }
        for (int s = S - 1; s >= 0; --s) {
            const T *Ws = stage0 + (size_t)s * se, *ts = Ws + (size_t)BRT_H * K;
            const int top = s ? q : 0, base = s ? BRT_H + (s - 1) * (BRT_H - q) : 0;
            const int hs = top + min(BRT_H - top, n - base);
            bsv_reflect_back<T, NE>(Ws, BRT_H, hs, q, reinterpret_cast<const int *>(ts + K), ts, x, lane);
            if (s) {
#pragma unroll
                for (int e = 0; e < NE; ++e) {
                    const int i = lane + 64 * e;
                    if (i >= top && i < hs) vc[(int64_t)(base + i - top) * vrs] = neg ? -x[e] : x[e];
                    x[e] = i < top ? x[e] : (T)0;
                }
            }
        }
#pragma unroll
        for (int e = 0; e < NE; ++e) vc[(int64_t)(lane + 64 * e) * vrs] = neg ? -x[e] : x[e];  // stage 0 of S >= 2 stages holds H rows
    }
}

// (brc_exponent, the exponent of an operand before it is loaded, is in batched_stages.hpp, shared with the complex kernel.)
// TALL = false: rc_lowrank_recompress_batched_*.  TALL = true: rc_lowrank_recompress_tall_batched_*, the left factor by stages (see above).
// LARGE (with TALL): rc_lowrank_recompress_large_batched_* for n > BRT_H, the right factor by stages too (see "both factors tall"); the
// launcher sends n <= BRT_H to the TALL instance, so this one carries neither the one-stage path of the right factor nor bsv_form_u for vt
template <typename T, bool TALL, bool LARGE = false>
__global__ __launch_bounds__(BID_THREADS) void k_batched_recompress(BrcArgs<T> a) {
    static_assert(TALL || !LARGE, "the large instance is the tall one with a staged right factor");
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const int m = (int)a.left.rows, n = (int)a.right.cols, K = (int)a.left.cols;
    const int kk = a.k < K ? a.k : K, ldg = a.ldg;
    const bool multi = TALL && m > BRT_H;  // the plan keeps the stage copies out of LDS
    constexpr bool rmulti = LARGE;  // likewise for the right factor's: n > BRT_H in that instance
    const int ldl = multi ? BRT_H : a.l_lds ? (m | 1) : m, ldr = rmulti ? BRT_H : a.r_lds ? (n | 1) : n, ldj = a.v_lds ? ldg : K;
    T *lds = reinterpret_cast<T *>(smem_raw);
    T *wsb = a.ws + (size_t)blockIdx.x * (LARGE  ? brl_ws_elems(m, n, K, a.l_lds, a.r_lds, a.v_lds)
                                          : TALL ? brt_ws_elems(m, n, K, a.l_lds, a.r_lds, a.v_lds)
                                                 : brc_ws_elems(m, n, K, a.l_lds, a.r_lds, a.v_lds));
    T *Wl0 = lds, *Wr0 = lds + (a.l_lds ? (size_t)K * ldl : 0);
    T *G = Wr0 + (a.r_lds ? (size_t)K * ldr : 0);
    T *J = G + (size_t)K * ldg;
    T *vn1 = J + (a.v_lds ? (size_t)K * ldg : 0);
    if (!a.l_lds) { Wl0 = wsb; wsb += multi ? (size_t)brt_stages(m, K) * brt_stage_elems(K) : (size_t)m * K; }
    if (!a.r_lds) { Wr0 = wsb; wsb += rmulti ? (size_t)brt_stages(n, K) * brt_stage_elems(K) : (size_t)n * K; }
    if (!a.v_lds) J = wsb;
    T *vn2 = vn1 + K, *taul = vn2 + K, *taur = taul + K, *sig = taur + K, *red = sig + K;
    int *jpl = reinterpret_cast<int *>(red + 8);
    int *jpr = jpl + K, *ipl = jpr + K, *ipr = ipl + K, *srt = ipr + K, *sgn = srt + K, *flag = sgn + 128;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;

    for (int b = blockIdx.x; b < a.count; b += gridDim.x) {
        int q = K;
        if (a.in_ranks) {
            const int64_t rv = a.in_ranks[b];
            q = rv < 0 ? 0 : rv > K ? K : (int)rv;
        }
        q = __builtin_amdgcn_readfirstlane(q);  // one value per block, uniform by construction
        T *sb = a.s_out + (int64_t)b * K;
        T *Ub = a.u.p + (int64_t)b * a.ubs, *Vb = a.vt.p + (int64_t)b * a.vbs;
        for (int i = q + tid; i < K; i += BID_THREADS) sb[i] = (T)0;
        if (q == 0) {  // uniform over the workgroup; no input is read
            if (tid == 0) a.ranks[b] = 0;
            for (int c = wv; c < kk; c += BID_WAVES) {
                for (int i = lane; i < m; i += 64) Ub[i * a.u.rs + c * a.u.cs] = (T)0;
                for (int i = lane; i < n; i += 64) Vb[c * a.vt.rs + i * a.vt.cs] = (T)0;
            }
            continue;
        }
        // ---- the two pivoted QRs, q steps each (exact zero pivots are steps with H = I), taus and pivots kept -----------------------
        const T *__restrict__ L = a.left.p + (int64_t)b * a.lbs;
        const T *__restrict__ R = a.right.p + (int64_t)b * a.rbs;
        T *Wl = Wl0;  // the copy the core and U read: the last stage's
        T *Wr = Wr0;  // likewise for T1
        // the factors' exponents (red[4..7], then red[0..3]: bid_qrcp writes red only behind the loads' barriers)
        const int el = brc_exponent(m, q, a.left.rs <= a.left.cs, [&](int i, int c) { return L[(int64_t)i * a.left.rs + c * a.left.cs]; }, red + 4, wv, lane);
        const int er = brc_exponent(n, q, a.right.cs <= a.right.rs, [&](int i, int c) { return R[c * a.right.rs + i * a.right.cs]; }, red, wv, lane);
        // mid's and s's (q x q and q elements): they enter T1 times 2^-em and 2^-es, so an X or an s that carries a block's scale meets the
        // normalised factors at unit scale as well, and a factor set with every operand extreme and a unit-scale product stays in range
        const T *__restrict__ Mb = a.mid.p ? a.mid.p + (int64_t)b * a.mbs : nullptr;
        const T *__restrict__ Sb = a.s ? a.s + (int64_t)b * a.s_stride : nullptr;
        const int em = Mb ? brc_exponent(q, q, a.mid.rs <= a.mid.cs, [&](int i, int c) { return Mb[(int64_t)i * a.mid.rs + c * a.mid.cs]; }, red + 4, wv, lane) : 0;
        const int es = Sb ? brc_exponent(q, 1, true, [&](int i, int) { return Sb[i]; }, red, wv, lane) : 0;
        const T scl = ldexp((T)1, -el), scr = ldexp((T)1, -er), scm = ldexp((T)1, -em), scs = ldexp((T)1, -es);
        [[maybe_unused]] int S = 1;
        if constexpr (TALL) {
            S = brt_stages(m, q);
            const size_t se = brt_stage_elems(K);
            for (int j = tid; j < q; j += BID_THREADS) jpl[j] = j;  // ordered before its first read by brt_stack_load's barrier
            for (int s = 0; s < S; ++s) {
                const int top = s ? q : 0, base = s ? BRT_H + (s - 1) * (BRT_H - q) : 0;
                const int hs = top + min(BRT_H - top, m - base);
                T *Ws = Wl0 + (multi ? (size_t)s * se : 0);
                T *ts = multi ? Ws + (size_t)BRT_H * K : taul;
                brt_stack_load(Ws, ldl, Ws - (s ? se : 0), top, hs, q, a.left.rs <= a.left.cs,
                               [&](int i, int c) { return L[(int64_t)(base + i) * a.left.rs + c * a.left.cs] * scl; }, vn1, vn2, jpl, wv, lane);
                bid_qrcp<T, true>(Ws, ldl, hs, q, q, 0.0, jpl, vn1, vn2, red, tid, wv, lane, ts);
                if (multi) {  // the stage's pivots beside its taus; jpl goes on as the next stage's starting order
                    int *js = reinterpret_cast<int *>(ts + K);
                    for (int j = tid; j < q; j += BID_THREADS) js[j] = jpl[j];
                }
                Wl = Ws;
            }
        } else {
            bid_load(Wl, ldl, m, q, a.left.rs <= a.left.cs, [&](int i, int c) { return L[i * a.left.rs + c * a.left.cs] * scl; }, vn1, vn2, jpl, wv, lane);
            bid_qrcp<T, true>(Wl, ldl, m, q, q, 0.0, jpl, vn1, vn2, red, tid, wv, lane, taul);
        }
        [[maybe_unused]] int Sr = 1;
        if constexpr (LARGE) {  // the left factor's stage loop on right[:q, :]^T, every stage in the slot
            Sr = brt_stages(n, q);
            const size_t se = brt_stage_elems(K);
            for (int j = tid; j < q; j += BID_THREADS) jpr[j] = j;  // ordered before its first read by brt_stack_load's barrier
            for (int s = 0; s < Sr; ++s) {
                const int top = s ? q : 0, base = s ? BRT_H + (s - 1) * (BRT_H - q) : 0;
                const int hs = top + min(BRT_H - top, n - base);
                T *Ws = Wr0 + (size_t)s * se;
                T *ts = Ws + (size_t)BRT_H * K;
                brt_stack_load(Ws, ldr, Ws - (s ? se : 0), top, hs, q, a.right.cs <= a.right.rs,
                               [&](int i, int c) { return R[c * a.right.rs + (int64_t)(base + i) * a.right.cs] * scr; }, vn1, vn2, jpr, wv, lane);
                bid_qrcp<T, true>(Ws, ldr, hs, q, q, 0.0, jpr, vn1, vn2, red, tid, wv, lane, ts);
                int *js = reinterpret_cast<int *>(ts + K);
                for (int j = tid; j < q; j += BID_THREADS) js[j] = jpr[j];
                Wr = Ws;
            }
        } else {
            bid_load(Wr, ldr, n, q, a.right.cs <= a.right.rs, [&](int i, int c) { return R[c * a.right.rs + i * a.right.cs] * scr; }, vn1, vn2, jpr, wv, lane);
            bid_qrcp<T, true>(Wr, ldr, n, q, q, 0.0, jpr, vn1, vn2, red, tid, wv, lane, taur);
        }
        for (int j = tid; j < q; j += BID_THREADS) { ipl[jpl[j]] = j; ipr[jpr[j]] = j; }
        __syncthreads();
        // ---- T1 = mid diag(s) Rr^T in J's place ----------------------------------------------------------------------------------------
        for (int idx = tid; idx < q * q; idx += BID_THREADS) {
            const int ai = idx / q, j = idx - ai * q;
            T acc;
            if (Mb) {
                acc = 0;
                const T *mr = Mb + (int64_t)ai * a.mid.rs;
                for (int bb = 0; bb < q; ++bb) {
                    const T rv = j <= ipr[bb] ? Wr[(size_t)bb * ldr + j] : (T)0;
                    const T mv = Sb ? (mr[(int64_t)bb * a.mid.cs] * scm) * (Sb[bb] * scs) : mr[(int64_t)bb * a.mid.cs] * scm;
                    acc = fma(mv, rv, acc);
                }
            } else {
                const T rv = j <= ipr[ai] ? Wr[(size_t)ai * ldr + j] : (T)0;
                acc = Sb ? (Sb[ai] * scs) * rv : rv;
            }
            J[(size_t)ai * ldj + j] = acc;
        }
        __syncthreads();
        // ---- G = C^T: G[i * ldg + j] = sum_a Rl[i, a] T1[a, j] ----------------------------------------------------------------------
        for (int idx = tid; idx < q * q; idx += BID_THREADS) {
            const int i = idx / q, j = idx - i * q;
            T acc = 0;
            for (int aa = 0; aa < q; ++aa) {
                const T lv = i <= ipl[aa] ? Wl[(size_t)aa * ldl + i] : (T)0;
                acc = fma(lv, J[(size_t)aa * ldj + j], acc);
            }
            G[(size_t)i * ldg + j] = acc;
        }
        __syncthreads();
        for (int idx = tid; idx < q * q; idx += BID_THREADS) {
            const int j = idx / q, i = idx - j * q;
            J[(size_t)j * ldj + i] = i == j ? (T)1 : (T)0;
        }
        __syncthreads();
        bool conv;
        if (q <= 16) conv = bsv_jacobi<T, 1>(G, ldg, J, ldj, q, tid, flag);
        else if (q <= 32) conv = bsv_jacobi<T, 2>(G, ldg, J, ldj, q, tid, flag);
        else if (q <= 64) conv = bsv_jacobi<T, 4>(G, ldg, J, ldj, q, tid, flag);
        else conv = bsv_jacobi<T, 8>(G, ldg, J, ldj, q, tid, flag);
        if (!conv && tid == 0) atomicOr(a.health, 16);  // the sweep budget ran out: bit 16, as the batched SVD reports it
        // ---- singular values: column norms, sorted descending (a strict total order: NaN last, ties by column) ----------------------
        for (int j = tid >> 4; j < q; j += BID_THREADS / 16) {
            const T *gj = G + (size_t)j * ldg;
            T acc = 0;
            for (int i = tid & 15; i < q; i += 16) acc = fma(gj[i], gj[i], acc);
            acc = group_sum_dpp<16>(acc);
            if ((tid & 15) == 0) sig[j] = sqrt(acc);
        }
        __syncthreads();
        for (int i = tid; i < q; i += BID_THREADS) {
            const T ki = sig[i] >= (T)0 ? sig[i] : (T)-1;
            int pos = 0;
            for (int j = 0; j < q; ++j) {
                const T kj = sig[j] >= (T)0 ? sig[j] : (T)-1;
                pos += (kj > ki || (kj == ki && j < i)) ? 1 : 0;
            }
            srt[pos] = i;
            sb[pos] = ldexp(sig[i], el + er + em + es);  // the operands entered as 2^-el left, 2^-em mid, 2^-es s and 2^-er right
        }
        __syncthreads();
        // ---- rank: the first j < min(kk, q) with s_j == 0 or (tol > 0 and s_j / s_0 < tol), else min(kk, q) -------------------------
        if (tid == 0) {
            const T s0 = sig[srt[0]];
            const int kq = kk < q ? kk : q;
            int r = kq;
            for (int j = 0; j < kq; ++j) {
                const T sj = sig[srt[j]];
                if (sj == (T)0 || (a.tol > 0.0 && (double)(sj / s0) < a.tol)) { r = j; break; }
            }
            flag[1] = r;
            a.ranks[b] = r;
        }
        __syncthreads();
        const int r = flag[1];
        // ---- U = Q_L [J_r; 0] with the signs fixed on its columns ----------------------------------------------------------------------
        if (TALL && S > 1) brt_form_u<T>(Wl0, brt_stage_elems(K), S, K, q, m, J, ldj, kk, r, srt, sgn, Ub, a.u.rs, a.u.cs, wv, lane);
        else if (m <= 64) bsv_form_u<T, 1>(Wl, ldl, J, ldj, m, q, kk, r, jpl, taul, srt, sgn, true, Ub, a.u.rs, a.u.cs, wv, lane);
        else if (m <= 128) bsv_form_u<T, 2>(Wl, ldl, J, ldj, m, q, kk, r, jpl, taul, srt, sgn, true, Ub, a.u.rs, a.u.cs, wv, lane);
        else if (m <= 256) bsv_form_u<T, 4>(Wl, ldl, J, ldj, m, q, kk, r, jpl, taul, srt, sgn, true, Ub, a.u.rs, a.u.cs, wv, lane);
        else bsv_form_u<T, 8>(Wl, ldl, J, ldj, m, q, kk, r, jpl, taul, srt, sgn, true, Ub, a.u.rs, a.u.cs, wv, lane);
        // ---- V_c = G Sigma^-1 in place (kept columns), then V = Q_R [V_c; 0] through vt's transposed view, with u's signs ---------------
        for (int c = wv; c < r; c += BID_WAVES) {
            T *gc = G + (size_t)srt[c] * ldg;
            const T sj = sig[srt[c]], inv = sj > (T)0 ? (T)1 / sj : (T)0;
            for (int i = lane; i < q; i += 64) gc[i] *= inv;
        }
        __syncthreads();  // sgn and the scaled columns are read by other waves below
        if constexpr (LARGE) brl_form_vt<T>(Wr0, brt_stage_elems(K), Sr, K, q, n, G, ldg, kk, r, srt, sgn, Vb, a.vt.cs, a.vt.rs, wv, lane);
        else if (n <= 64) bsv_form_u<T, 1>(Wr, ldr, G, ldg, n, q, kk, r, jpr, taur, srt, sgn, false, Vb, a.vt.cs, a.vt.rs, wv, lane);
        else if (n <= 128) bsv_form_u<T, 2>(Wr, ldr, G, ldg, n, q, kk, r, jpr, taur, srt, sgn, false, Vb, a.vt.cs, a.vt.rs, wv, lane);
        else if (n <= 256) bsv_form_u<T, 4>(Wr, ldr, G, ldg, n, q, kk, r, jpr, taur, srt, sgn, false, Vb, a.vt.cs, a.vt.rs, wv, lane);
        else bsv_form_u<T, 8>(Wr, ldr, G, ldg, n, q, kk, r, jpr, taur, srt, sgn, false, Vb, a.vt.cs, a.vt.rs, wv, lane);
        __syncthreads();  // the working copies, G, J and the small arrays are rewritten by the next block
    }
}


// ---- batched sketched column ID (rc_sketch_column_id_rank_batched_*) ------------------------------------------------------------
// Per block, the reference's randomized path (sample, project, factor the small projected matrix: sample_range_by_rank in
// src/random_sampling.rs, QR::compute_from_range_estimate + column_id, src/qr.rs:311-323): the sketch Y = Omega A (l x n, l <= 128) is
// formed straight into the working copy W that bid_qrcp factors, then the stages of k_batched_id run on W with l rows instead of m:
// pivots, rank and Z are those of the column ID of Y, C is gathered from A.  A is read from HBM once (plus the kept columns for C),
// so m is bounded by the index range, not by what a workgroup can hold.
//
// The sketch.  Column panels of BSI_COLS = 64 columns of Y, one 16-column MFMA tile per wave, all TL = ceil(l / 16) row tiles of the
// panel in the wave's accumulators (v_mfma_f64_16x16x4_f64 / v_mfma_f32_16x16x4_f32, Acc<T> of rc_gemm.hpp).  The panel's rows of A
// stream through LDS in chunks of BSI_ROWS = 32 rows beside the matching 32 columns of Omega, which is re-read per panel (from L2).
// Both chunks are read with the lanes along the operand's smaller stride and keep that index fastest in LDS (pitch 34 along the
// reduction index, or a pitch of 16 modulo 32 along the other: the fragment reads of either image are bank-conflict free); rows past
// m, columns past n and rows of Omega past l are zeros in LDS, so the MFMA loop has no edge branch.  An element of Y is summed in
// ascending row order: chunk after chunk, four rows per MFMA: a function of (l, m, n) and the two constants alone.
// (BSI_ROWS, BSI_COLS and the pitches of the chunk images are in rc_gemm.hpp, shared with the complex kernel.)
// dynamic LDS: [W: n x (l|1), LDS plan only] A chunk [BSI_A_ELEMS] Omega chunk [bsi_o_elems(l)] vn1[n] vn2[n] tile[16 x 17] red[8] | jp[n]
template <typename T>
size_t bsi_lds_bytes(int l, int n, bool in_lds) {
    size_t t = (size_t)BSI_A_ELEMS + (size_t)bsi_o_elems(l) + (size_t)2 * n + BID_NB * (BID_NB + 1) + 8;
    if (in_lds) t += (size_t)n * (size_t)(l | 1);
    return t * sizeof(T) + (size_t)n * sizeof(int);
}

template <typename T>
struct BsiArgs {
    Mat<T> a, omega, y, c, z;  // y.p == nullptr: the sketch is not written
    int64_t abs, obs, ybs, cbs, zbs;
    int64_t *col_ind, *ranks;
    T *ws;
    double tol;
    int count, kk;
    bool w_lds;  // the working copy in LDS (else in the workgroup's workspace slot)
};

// W[c * ldw + i] = Y[i, c] = sum_r Om[i, r] A[r, c] for the l x n sketch of one block (and Y to Yb when it is not null).
// AR / OR: the lanes of the staging loads run along the rows of a / of omega (the operand's smaller stride), else along its columns;
// each thread's elements of a chunk are then a fixed step apart in memory and in the LDS image, whose offsets are compile-time constants.
// WM: where the sketch goes besides Yb.  BSI_W_COLS: W[c * ldw + i] as above; BSI_W_ROWS: W[i * ldw + c], the working copy of Y^T
// (k_batched_range_step's row basis); BSI_W_NONE: W is not written (its projection, whose l x m "sketch" only goes to Yb).
enum { BSI_W_COLS = 0, BSI_W_ROWS = 1, BSI_W_NONE = 2 };
template <typename T, int TL, bool AR, bool OR, int WM = BSI_W_COLS>
__device__ __forceinline__ void bsi_sketch(const BsiArgs<T> &g, const T *__restrict__ A, const T *__restrict__ Om, T *Yb, T *W, int ldw, T *As, T *Os, int tid,
                                           int wv, int lane) {
    constexpr int PO = bsi_po(16 * TL);
    constexpr int A_PER = BSI_ROWS * BSI_COLS / BID_THREADS;    // 8 elements of A per thread and chunk
    constexpr int O_PER = BSI_ROWS * 16 * TL / BID_THREADS;     // 2 TL elements of Omega
    constexpr int A_SR = AR ? 1 : BSI_PA, A_SC = AR ? BSI_PK : 1;   // A's image: As[r * A_SR + c * A_SC]
    constexpr int O_SI = OR ? 1 : BSI_PK, O_SR = OR ? PO : 1;       // Omega's image: Os[i * O_SI + r * O_SR]
    const int m = (int)g.a.rows, n = (int)g.a.cols, l = (int)g.omega.rows;
    const int64_t ars = g.a.rs, acs = g.a.cs, ors = g.omega.rs, ocs = g.omega.cs;
    // this thread's elements of a chunk: A[ar + AR_STEP e, ac + AC_STEP e], Om[oi + 16 (e / 2) or 8 e, orr + 16 (e % 2) or 0]
    const int ar = AR ? (tid & (BSI_ROWS - 1)) : (tid / BSI_COLS), ac = AR ? (tid / BSI_ROWS) : (tid & (BSI_COLS - 1));
    constexpr int AR_STEP = AR ? 0 : BID_THREADS / BSI_COLS, AC_STEP = AR ? BID_THREADS / BSI_ROWS : 0;
    const int oi = OR ? (tid & 15) : (tid / BSI_ROWS), orr = OR ? (tid >> 4) : (tid & (BSI_ROWS - 1));
    const int r16 = lane & 15, k4 = lane >> 4;
    T *as_st = As + ar * A_SR + ac * A_SC, *os_st = Os + oi * O_SI + orr * O_SR;
    const T *as_ld = As + k4 * A_SR + (wv * 16 + r16) * A_SC, *os_ld = Os + r16 * O_SI + k4 * O_SR;
    for (int c0 = 0; c0 < n; c0 += BSI_COLS) {
        typename Acc<T>::type acc[TL];
#pragma unroll
        for (int i = 0; i < TL; ++i) acc[i] = typename Acc<T>::type{0, 0, 0, 0};
        for (int m0 = 0; m0 < m; m0 += BSI_ROWS) {
            T av[A_PER], ov[O_PER];
            const T *pa = A + (int64_t)(m0 + ar) * ars + (int64_t)(c0 + ac) * acs;
            const T *po = Om + (int64_t)oi * ors + (int64_t)(m0 + orr) * ocs;
            // the steps between a thread's elements are uniform; hidden from the optimizer here, every address is the thread's one base plus a
            // scalar offset (otherwise each of the 8 + 2 TL addresses becomes a loop-carried 64-bit register pair of its own)
            int64_t sa = AR ? AC_STEP * acs : AR_STEP * ars, so_i = ors, so_r = ocs;
            asm volatile("" : "+s"(sa), "+s"(so_i), "+s"(so_r));
#pragma unroll
            for (int e = 0; e < A_PER; ++e) {
                const bool ok = m0 + ar + AR_STEP * e < m && c0 + ac + AC_STEP * e < n;
                av[e] = ok ? pa[e * sa] : (T)0;
            }
#pragma unroll
            for (int e = 0; e < O_PER; ++e) {
                const int di = OR ? 16 * (e / 2) : 8 * e, dr = OR ? 16 * (e % 2) : 0;
                const bool ok = oi + di < l && m0 + orr + dr < m;
                ov[e] = ok ? po[di * so_i + dr * so_r] : (T)0;
            }
#pragma unroll
            for (int e = 0; e < A_PER; ++e) as_st[AR_STEP * e * A_SR + AC_STEP * e * A_SC] = av[e];
#pragma unroll
            for (int e = 0; e < O_PER; ++e) {
                const int di = OR ? 16 * (e / 2) : 8 * e, dr = OR ? 16 * (e % 2) : 0;
                os_st[di * O_SI + dr * O_SR] = ov[e];
            }
            __syncthreads();
#pragma unroll
            for (int ks = 0; ks < BSI_ROWS / 4; ++ks) {
                const T bf = as_ld[ks * 4 * A_SR];
#pragma unroll
                for (int i = 0; i < TL; ++i) acc[i] = Acc<T>::mfma(os_ld[i * 16 * O_SI + ks * 4 * O_SR], bf, acc[i]);
            }
            __syncthreads();  // the chunk images are rewritten by the next chunk
        }
        const int col = c0 + wv * 16 + r16;
#pragma unroll
        for (int i = 0; i < TL; ++i)
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int row = i * 16 + Acc<T>::row(lane, reg);
                if (row < l && col < n) {
                    const T v = acc[i][reg];
                    if constexpr (WM == BSI_W_COLS) W[(size_t)col * ldw + row] = v;
                    if constexpr (WM == BSI_W_ROWS) W[(size_t)row * ldw + col] = v;
                    if (Yb) Yb[row * g.y.rs + col * g.y.cs] = v;
                }
            }
    }
    __syncthreads();
}

template <typename T, bool AR, bool OR>
__global__ __launch_bounds__(BID_THREADS, 2) void k_batched_sketch_id(BsiArgs<T> g) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const int m = (int)g.a.rows, n = (int)g.a.cols, l = (int)g.omega.rows, kk = g.kk;
    const int ldw = g.w_lds ? (l | 1) : l;
    T *lds = reinterpret_cast<T *>(smem_raw);
    T *W = g.w_lds ? lds : g.ws + (size_t)blockIdx.x * (size_t)l * (size_t)n;
    T *As = lds + (g.w_lds ? (size_t)n * ldw : 0);
    T *Os = As + BSI_A_ELEMS;
    T *vn1 = Os + bsi_o_elems(l);
    T *vn2 = vn1 + n;
    T(*tile)[BID_NB + 1] = reinterpret_cast<T(*)[BID_NB + 1]>(vn2 + n);
    T *red = vn2 + n + BID_NB * (BID_NB + 1);
    int *jp = reinterpret_cast<int *>(red + 8);
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;

    for (int b = blockIdx.x; b < g.count; b += gridDim.x) {
        const T *__restrict__ A = g.a.p + (int64_t)b * g.abs;
        const T *__restrict__ Om = g.omega.p + (int64_t)b * g.obs;
        T *Yb = g.y.p ? g.y.p + (int64_t)b * g.ybs : nullptr;
        // ---- the sketch into W (and y), one instance per number of 16-row tiles so that the accumulators stay in registers ------------
        switch ((l + 15) >> 4) {
            case 1: bsi_sketch<T, 1, AR, OR>(g, A, Om, Yb, W, ldw, As, Os, tid, wv, lane); break;
            case 2: bsi_sketch<T, 2, AR, OR>(g, A, Om, Yb, W, ldw, As, Os, tid, wv, lane); break;
            case 3: bsi_sketch<T, 3, AR, OR>(g, A, Om, Yb, W, ldw, As, Os, tid, wv, lane); break;
            case 4: bsi_sketch<T, 4, AR, OR>(g, A, Om, Yb, W, ldw, As, Os, tid, wv, lane); break;
            case 5: bsi_sketch<T, 5, AR, OR>(g, A, Om, Yb, W, ldw, As, Os, tid, wv, lane); break;
            case 6: bsi_sketch<T, 6, AR, OR>(g, A, Om, Yb, W, ldw, As, Os, tid, wv, lane); break;
            case 7: bsi_sketch<T, 7, AR, OR>(g, A, Om, Yb, W, ldw, As, Os, tid, wv, lane); break;
            default: bsi_sketch<T, 8, AR, OR>(g, A, Om, Yb, W, ldw, As, Os, tid, wv, lane); break;
        }
        // ---- the column ID of Y: k_batched_id's stages on l rows ----------------------------------------------------------------------
        bid_norms_pow2(W, ldw, l, n, vn1, vn2, jp, red + 4, wv, lane);
        const int r = bid_qrcp(W, ldw, l, n, kk, g.tol, jp, vn1, vn2, red, tid, wv, lane);
        for (int p = tid; p < n; p += BID_THREADS) g.col_ind[(int64_t)b * n + p] = jp[p];
        if (tid == 0) g.ranks[b] = r;
        // C[:, j] = A[:, jp[j]] (zero for j >= r), the lanes along a's smaller stride
        T *Cb = g.c.p + (int64_t)b * g.cbs;
        if (g.a.rs <= g.a.cs) {
            for (int j = wv; j < kk; j += BID_WAVES) {
                const T *src = A + (int64_t)jp[j] * g.a.cs;
                for (int i = lane; i < m; i += 64) Cb[i * g.c.rs + j * g.c.cs] = j < r ? src[i * g.a.rs] : (T)0;
            }
        } else {
            const int total = m * kk;  // <= 65536 * 128
            for (int idx = tid; idx < total; idx += BID_THREADS) {
                const int i = idx / kk, j = idx - i * kk;
                Cb[i * g.c.rs + j * g.c.cs] = j < r ? A[i * g.a.rs + (int64_t)jp[j] * g.a.cs] : (T)0;
            }
        }
        bid_z(W, ldw, n, r, kk, jp, tile, g.z.p + (int64_t)b * g.zbs, g.z.rs, g.z.cs, tid);
        __syncthreads();  // W, jp and the norms are rewritten by the next block
    }
}

// ---- batched sketch product (rc_sketch_product_batched_*) ----------------------------------------------------------------------------
// Per block Y = Omega A and nothing else, for n up to 65536: bsi_sketch's panel (BSI_COLS columns of Y, all TL row tiles in the wave's
// accumulators, A and Omega through LDS in chunks of BSI_ROWS rows, the same images, the same zero padding, the same MFMA sequence from
// zero over ascending rows of A), so an element of Y has bsi_sketch's bits and column j of Y depends on column j of A, on Omega and on m
// alone.  What differs is around the chain: a work unit of the persistent grid is one (block, panel) pair, units = count * ceil(n / 64), so
// a few large blocks fill the chip; and the kernel carries no QR state, so chunk i + 1 of A and Omega is loaded into registers before the
// MFMAs of chunk i and stored to LDS after them.  Nothing is split along m; no workspace, no atomics.
// dynamic LDS: A chunk [BSI_A_ELEMS] Omega chunk [bsi_o_elems(l)]
template <typename T>
struct BspArgs {
    Mat<T> a, omega, y;
    int64_t abs, obs, ybs;
    int64_t units;  // count * panels
    int panels;     // ceil(n / BSI_COLS)
};

// every unit of this workgroup for TL = ceil(l / 16) row tiles; AR / OR as in bsi_sketch.  All in-block offsets are 64-bit: m * n reaches 2^32.
template <typename T, int TL, bool AR, bool OR>
__device__ __forceinline__ void bsp_units(const BspArgs<T> &g, T *As, T *Os, int wv) {
    // the thread index from the wave's number (uniform, a scalar register) and the lane's count under a mask behind an empty asm: the
    // per-thread staging offsets are then this instance's own, and no vector register stays live across the dispatch (threadIdx.x in v0 was
    // spilled there: the one f64 instance that fills all 256 registers had 8 bytes of scratch)
    unsigned all = ~0u;
    asm volatile("" : "+s"(all));
    const int lane = (int)__builtin_amdgcn_mbcnt_hi(all, __builtin_amdgcn_mbcnt_lo(all, 0u));
    const int tid = wv * 64 + lane;
    constexpr int PO = bsi_po(16 * TL);
    constexpr int A_PER = BSI_ROWS * BSI_COLS / BID_THREADS;    // 8 elements of A per thread and chunk
    constexpr int O_PER = BSI_ROWS * 16 * TL / BID_THREADS;     // 2 TL elements of Omega
    constexpr int A_SR = AR ? 1 : BSI_PA, A_SC = AR ? BSI_PK : 1;   // A's image: As[r * A_SR + c * A_SC]
    constexpr int O_SI = OR ? 1 : BSI_PK, O_SR = OR ? PO : 1;       // Omega's image: Os[i * O_SI + r * O_SR]
    const int m = (int)g.a.rows, n = (int)g.a.cols, l = (int)g.omega.rows;
    const int64_t ars = g.a.rs, acs = g.a.cs, ors = g.omega.rs, ocs = g.omega.cs;
    const int ar = AR ? (tid & (BSI_ROWS - 1)) : (tid / BSI_COLS), ac = AR ? (tid / BSI_ROWS) : (tid & (BSI_COLS - 1));
    constexpr int AR_STEP = AR ? 0 : BID_THREADS / BSI_COLS, AC_STEP = AR ? BID_THREADS / BSI_ROWS : 0;
    const int oi = OR ? (tid & 15) : (tid / BSI_ROWS), orr = OR ? (tid >> 4) : (tid & (BSI_ROWS - 1));
    const int r16 = lane & 15, k4 = lane >> 4;
    T *as_st = As + ar * A_SR + ac * A_SC, *os_st = Os + oi * O_SI + orr * O_SR;
    const T *as_ld = As + k4 * A_SR + (wv * 16 + r16) * A_SC, *os_ld = Os + r16 * O_SI + k4 * O_SR;
    for (int64_t u = blockIdx.x; u < g.units; u += gridDim.x) {
        const int64_t b = u / g.panels;
        const int c0 = (int)(u - b * g.panels) * BSI_COLS;
        const T *__restrict__ A = g.a.p + b * g.abs;
        const T *__restrict__ Om = g.omega.p + b * g.obs;
        T *Yb = g.y.p + b * g.ybs;
        T av[A_PER], ov[O_PER];
        // this thread's elements of the chunk at row m0 (bsi_sketch's, with its uniform steps behind an empty asm), zeros past m, n and l
        auto load = [&](int m0) {
            const T *pa = A + (int64_t)(m0 + ar) * ars + (int64_t)(c0 + ac) * acs;
            const T *po = Om + (int64_t)oi * ors + (int64_t)(m0 + orr) * ocs;
            int64_t sa = AR ? AC_STEP * acs : AR_STEP * ars, so_i = ors, so_r = ocs;
            asm volatile("" : "+s"(sa), "+s"(so_i), "+s"(so_r));
#pragma unroll
            for (int e = 0; e < A_PER; ++e) {
                const bool ok = m0 + ar + AR_STEP * e < m && c0 + ac + AC_STEP * e < n;
                av[e] = ok ? pa[e * sa] : (T)0;
            }
#pragma unroll
            for (int e = 0; e < O_PER; ++e) {
                const int di = OR ? 16 * (e / 2) : 8 * e, dr = OR ? 16 * (e % 2) : 0;
                const bool ok = oi + di < l && m0 + orr + dr < m;
                ov[e] = ok ? po[di * so_i + dr * so_r] : (T)0;
            }
        };
        typename Acc<T>::type acc[TL];
#pragma unroll
        for (int i = 0; i < TL; ++i) acc[i] = typename Acc<T>::type{0, 0, 0, 0};
        load(0);
        for (int m0 = 0; m0 < m; m0 += BSI_ROWS) {
#pragma unroll
            for (int e = 0; e < A_PER; ++e) as_st[AR_STEP * e * A_SR + AC_STEP * e * A_SC] = av[e];
#pragma unroll
            for (int e = 0; e < O_PER; ++e) {
                const int di = OR ? 16 * (e / 2) : 8 * e, dr = OR ? 16 * (e % 2) : 0;
                os_st[di * O_SI + dr * O_SR] = ov[e];
            }
            __syncthreads();
            if (m0 + BSI_ROWS < m) load(m0 + BSI_ROWS);  // in flight during the MFMAs below
#pragma unroll
            for (int ks = 0; ks < BSI_ROWS / 4; ++ks) {
                const T bf = as_ld[ks * 4 * A_SR];
#pragma unroll
                for (int i = 0; i < TL; ++i) acc[i] = Acc<T>::mfma(os_ld[i * 16 * O_SI + ks * 4 * O_SR], bf, acc[i]);
            }
            __syncthreads();  // the chunk images are rewritten by the next chunk (and by the next unit)
        }
        const int col = c0 + wv * 16 + r16;
#pragma unroll
        for (int i = 0; i < TL; ++i)
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int row = i * 16 + Acc<T>::row(lane, reg);
                if (row < l && col < n) Yb[row * g.y.rs + col * g.y.cs] = acc[i][reg];
            }
    }
}

template <typename T, bool AR, bool OR>
__global__ __launch_bounds__(BID_THREADS, 2) void k_batched_sketch_product(BspArgs<T> g) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    T *As = reinterpret_cast<T *>(smem_raw);
    T *Os = As + BSI_A_ELEMS;
    const int wv = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    // one instance per number of 16-row tiles, each with its own unit loop
    switch (((int)g.omega.rows + 15) >> 4) {
        case 1: bsp_units<T, 1, AR, OR>(g, As, Os, wv); break;
        case 2: bsp_units<T, 2, AR, OR>(g, As, Os, wv); break;
        case 3: bsp_units<T, 3, AR, OR>(g, As, Os, wv); break;
        case 4: bsp_units<T, 4, AR, OR>(g, As, Os, wv); break;
        case 5: bsp_units<T, 5, AR, OR>(g, As, Os, wv); break;
        case 6: bsp_units<T, 6, AR, OR>(g, As, Os, wv); break;
        case 7: bsp_units<T, 7, AR, OR>(g, As, Os, wv); break;
        default: bsp_units<T, 8, AR, OR>(g, As, Os, wv); break;
    }
}

// ---- batched range step (rc_sketch_range_step_batched_*) ------------------------------------------------------------------------------
// One half-iteration pair of the reference's sample_range_power_iteration (src/random_sampling.rs:131-158) per block, without the second
// orthonormalisation (rc_lowrank_recompress_tall_batched_* with right = I does that to p): the sketch Y = Omega A by bsi_sketch, the same
// instances as k_batched_sketch_id but stored as the working copy of Y^T (n x l, column i = row i of Y); the pivoted Householder QR of
// Y^T by bid_qrcp run to all l steps with the reflectors kept; the rank r, the first step whose R_jj is exactly zero or not finite; Q
// (l x n) formed explicitly, row c = (H_0 .. H_c e_c)^T for c < r and exactly zero from r on, written to q and, n fastest, to the
// workgroup's slot; then the projection P^T = Q A^T, which is bsi_sketch once more on the transposed view of A with the slot's Q as the test
// matrix (the lanes of its staging loads along n) and P^T's only destination the transposed view of p.  So an element of P is one MFMA
// accumulator chain from zero over ascending column index of A, four columns per instruction, and a zero row of Q is a zero column of P.
// A streams from HBM twice; Q is re-read per 64-row panel of A from L2, as Omega is per column panel in the sketch.
// dynamic LDS: [W: l x (n|1), LDS plan only] A chunk [BSI_A_ELEMS] Omega chunk [bsi_o_elems(l)] vn1[l] vn2[l] taus[l] red[8] | jp[l] rk[4]
// slot: Q [l x n] [W: l x n, workspace plan only]
template <typename T>
size_t brs_lds_bytes(int l, int n, bool in_lds) {
    size_t t = (size_t)BSI_A_ELEMS + (size_t)bsi_o_elems(l) + (size_t)3 * l + 8;
    if (in_lds) t += (size_t)l * (size_t)(n | 1);
    return t * sizeof(T) + (size_t)(l + 4) * sizeof(int);
}

template <typename T>
struct BrsArgs {
    Mat<T> a, omega, y, q, p;  // y.p == nullptr: the sketch is not written
    int64_t abs, obs, ybs, qbs, pbs;
    int64_t *ranks;
    T *ws;
    size_t slot;  // elements of one workgroup's slot
    int count;
    bool w_lds;   // the working copy of Y^T in LDS (else behind Q in the slot)
};

// Q[c, :] = (H_0 .. H_c e_c)^T for c < r, zero for r <= c < l, to Qs[c * n + i] and Qb[c * qrs + i * qcs]: one wave per row of Q, its n
// entries in registers (entry lane + 64 e), H_j = I - tau_j v_j v_j^T with v_j in W's column jp[j] below row j (bsv_form_u's application)
template <typename T, int NE>
__device__ __forceinline__ void brs_form_q(const T *W, int ldw, int n, int l, int r, const int *jp, const T *taus, T *Qs, T *Qb, int64_t qrs, int64_t qcs,
                                           int wv, int lane) {
    for (int c = wv; c < l; c += BID_WAVES) {
        T x[NE];
#pragma unroll
        for (int e = 0; e < NE; ++e) x[e] = (c < r && lane + 64 * e == c) ? (T)1 : (T)0;
        for (int j = c < r ? c : -1; j >= 0; --j) {
            const T tau = taus[j];
            if (tau == (T)0) continue;  // H_j = I (uniform)
            const T *vc = W + (size_t)jp[j] * ldw;
            T v[NE];
            T dot = 0;
#pragma unroll
            for (int e = 0; e < NE; ++e) {
                const int i = lane + 64 * e;
                const T vv = vc[i < n ? i : j];  // branch-free: lanes out of range read row j and are masked below
                v[e] = i > j && i < n ? vv : (i == j ? (T)1 : (T)0);
                dot = fma(v[e], x[e], dot);
            }
            const T f = tau * wave_sum_dpp(dot);
#pragma unroll
            for (int e = 0; e < NE; ++e) x[e] = fma(-f, v[e], x[e]);
        }
#pragma unroll
        for (int e = 0; e < NE; ++e) {
            const int i = lane + 64 * e;
            if (i < n) {
                Qs[(size_t)c * n + i] = x[e];
                Qb[c * qrs + i * qcs] = x[e];
            }
        }
    }
}

// bsi_sketch's instance for TL = ceil(l / 16) row tiles
#define RC_BSI_DISPATCH(AR_, OR_, WM_, ...)                                             \
    switch ((l + 15) >> 4) {                                                            \
        case 1: bsi_sketch<T, 1, AR_, OR_, WM_>(__VA_ARGS__); break;                    \
        case 2: bsi_sketch<T, 2, AR_, OR_, WM_>(__VA_ARGS__); break;                    \
        case 3: bsi_sketch<T, 3, AR_, OR_, WM_>(__VA_ARGS__); break;                    \
        case 4: bsi_sketch<T, 4, AR_, OR_, WM_>(__VA_ARGS__); break;                    \
        case 5: bsi_sketch<T, 5, AR_, OR_, WM_>(__VA_ARGS__); break;                    \
        case 6: bsi_sketch<T, 6, AR_, OR_, WM_>(__VA_ARGS__); break;                    \
        case 7: bsi_sketch<T, 7, AR_, OR_, WM_>(__VA_ARGS__); break;                    \
        default: bsi_sketch<T, 8, AR_, OR_, WM_>(__VA_ARGS__); break;                   \
    }

template <typename T, bool AR, bool OR>
__global__ __launch_bounds__(BID_THREADS, 2) void k_batched_range_step(BrsArgs<T> g) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const int m = (int)g.a.rows, n = (int)g.a.cols, l = (int)g.omega.rows;
    const int ldw = g.w_lds ? (n | 1) : n;
    T *lds = reinterpret_cast<T *>(smem_raw);
    T *Qs = g.ws + (size_t)blockIdx.x * g.slot;
    T *W = g.w_lds ? lds : Qs + (size_t)l * (size_t)n;
    T *As = lds + (g.w_lds ? (size_t)l * ldw : 0);
    T *Os = As + BSI_A_ELEMS;
    T *vn1 = Os + bsi_o_elems(l);
    T *vn2 = vn1 + l;
    T *taus = vn2 + l;
    T *red = taus + l;
    int *jp = reinterpret_cast<int *>(red + 8);
    int *rk = jp + l;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;

    for (int b = blockIdx.x; b < g.count; b += gridDim.x) {
        const T *__restrict__ A = g.a.p + (int64_t)b * g.abs;
        const T *__restrict__ Om = g.omega.p + (int64_t)b * g.obs;
        T *Yb = g.y.p ? g.y.p + (int64_t)b * g.ybs : nullptr;
        // ---- the sketch, k_batched_sketch_id's, into the working copy of Y^T (and y) -----------------------------------------------------
        {
            BsiArgs<T> s;
            s.a = g.a; s.omega = g.omega; s.y = g.y;
            // the thread index behind an empty asm: the sketch's per-thread staging offsets (16 instances of them with the projection's) are then
            // recomputed per block instead of being hoisted out of the block loop and spilled there
            int t = tid;
            asm volatile("" : "+v"(t));
            RC_BSI_DISPATCH(AR, OR, BSI_W_ROWS, s, A, Om, Yb, W, ldw, As, Os, t, t >> 6, t & 63)
        }
        // ---- the row basis: Y^T P = Q R to all l steps, the rank from R's diagonal, Q formed from the first r reflectors -----------------
        bid_norms_pow2(W, ldw, n, l, vn1, vn2, jp, red + 4, wv, lane);
        if (tid == 0) *rk = l;
        bid_qrcp<T, true>(W, ldw, n, l, l, 0.0, jp, vn1, vn2, red, tid, wv, lane, taus);
        if (tid < l) {
            const T d = W[(size_t)jp[tid] * ldw + tid];
            if (d == (T)0 || !isfinite(d)) atomicMin(rk, tid);
        }
        __syncthreads();
        const int r = *rk;
        if (tid == 0) g.ranks[b] = r;
        T *Qb = g.q.p + (int64_t)b * g.qbs;
        if (n <= 128) brs_form_q<T, 2>(W, ldw, n, l, r, jp, taus, Qs, Qb, g.q.rs, g.q.cs, wv, lane);
        else if (n <= 256) brs_form_q<T, 4>(W, ldw, n, l, r, jp, taus, Qs, Qb, g.q.rs, g.q.cs, wv, lane);
        else brs_form_q<T, 8>(W, ldw, n, l, r, jp, taus, Qs, Qb, g.q.rs, g.q.cs, wv, lane);
        __syncthreads();  // the slot's Q is read by every wave below
        // ---- the projection P^T = Q A^T: the sketch of a's transposed view with the slot's Q, into p's transposed view --------------------
        {
            BsiArgs<T> s;
            s.a = Mat<T>(g.a.p, n, m, g.a.cs, g.a.rs);
            s.omega = Mat<T>(Qs, l, n, n, 1);
            s.y = Mat<T>(g.p.p, l, m, g.p.cs, g.p.rs);
            int t = tid;
            asm volatile("" : "+v"(t));
            RC_BSI_DISPATCH(!AR, false, BSI_W_NONE, s, A, Qs, g.p.p + (int64_t)b * g.pbs, nullptr, 0, As, Os, t, t >> 6, t & 63)
        }
        __syncthreads();  // W, Q, jp and the small arrays are rewritten by the next block
    }
}
#undef RC_BSI_DISPATCH

// ---- what the shared plans and launchers take from this family (batched_launchers.hpp) ------------------------------------------------------
template <typename T>
struct RealFamily {
    using RecompressArgs = BrcArgs<T>;
    using SketchIdArgs = BsiArgs<T>;
    using RangeStepArgs = BrsArgs<T>;
    static size_t svd_lds_bytes(int M, int N, BsvPlace p) { return bsv_lds_bytes<T>(M, N, p.ld, p.w, p.v); }
    static size_t svd_ws_elems(int M, int N, BsvPlace p) { return (p.w ? 0 : (size_t)M * N) + (p.v ? 0 : (size_t)N * N); }
    static auto svd_kernel(BsvPlace p) { return p.w ? k_batched_svd<T, true, true> : p.v ? k_batched_svd<T, false, true> : k_batched_svd<T, false, false>; }
    static size_t recompress_lds_bytes(int m, int n, int K, BrcPlace p) { return brc_lds_bytes<T>(m, n, K, p.ld, p.l, p.r, p.v); }
    static size_t recompress_ws_elems(int form, int m, int n, int K, BrcPlace p) {
        return form == BRC_LARGE ? brl_ws_elems(m, n, K, p.l, p.r, p.v) : form == BRC_TALL ? brt_ws_elems(m, n, K, p.l, p.r, p.v) : brc_ws_elems(m, n, K, p.l, p.r, p.v);
    }
    // n <= BRT_H under the large call is the tall instance under the tall plan (brc_plan returns it): the same kernel, the same bits
    template <int FORM>
    static auto recompress_kernel(int, int n) {
        constexpr bool TALL = FORM != BRC_SMALL, LARGE = FORM == BRC_LARGE;
        return LARGE && n > BRT_H ? k_batched_recompress<T, TALL, LARGE> : k_batched_recompress<T, TALL, false>;
    }
    static size_t sketch_id_lds_bytes(int l, int n, bool w_lds) { return bsi_lds_bytes<T>(l, n, w_lds); }
    static auto sketch_id_kernel(bool a_rows, bool o_rows) {
        void (*const kerns[4])(BsiArgs<T>) = {k_batched_sketch_id<T, false, false>, k_batched_sketch_id<T, false, true>, k_batched_sketch_id<T, true, false>,
                                              k_batched_sketch_id<T, true, true>};
        return kerns[(a_rows ? 2 : 0) + (o_rows ? 1 : 0)];
    }
    static size_t range_step_lds_bytes(int l, int n, bool w_lds) { return brs_lds_bytes<T>(l, n, w_lds); }
    static auto range_step_kernel(bool a_rows, bool o_rows) {
        void (*const kerns[4])(BrsArgs<T>) = {k_batched_range_step<T, false, false>, k_batched_range_step<T, false, true>, k_batched_range_step<T, true, false>,
                                              k_batched_range_step<T, true, true>};
        return kerns[(a_rows ? 2 : 0) + (o_rows ? 1 : 0)];
    }
};

}  // namespace

template <> struct BatchedFamily<double> : RealFamily<double> {};
template <> struct BatchedFamily<float> : RealFamily<float> {};

// (the launchers of the two IDs, the SVD, the recompressions, the sketched column ID and the range step: batched_launchers.hpp)

// No plan: the two chunk images are the whole LDS and there is no workspace.  The grid is bid_grid's over the (block, panel) units, so it
// does not move a unit's bits either; the four instances are the sketched ID's.  The label carries the units and the scratch bytes per
// thread, which are 0 in every instance (accumulators and one staging set in flight: DESIGN.md 7u).
template <typename T>
void batched_sketch_product(rc_context *c, Mat<T> a, int64_t abs, Mat<T> omega, int64_t obs, int32_t count, Mat<T> y, int64_t ybs) {
    const int m = (int)a.rows, n = (int)a.cols, l = (int)omega.rows;
    if (count <= 0) return;
    const int panels = (n + BSI_COLS - 1) / BSI_COLS;
    const int64_t units = (int64_t)count * panels;
    const size_t lds = ((size_t)BSI_A_ELEMS + (size_t)bsi_o_elems(l)) * sizeof(T);
    const bool a_rows = a.rs <= a.cs, o_rows = omega.rs < omega.cs;
    void (*const kerns[4])(BspArgs<T>) = {k_batched_sketch_product<T, false, false>, k_batched_sketch_product<T, false, true>,
                                          k_batched_sketch_product<T, true, false>, k_batched_sketch_product<T, true, true>};
    const auto lch = batched_prepare(c, kerns[(a_rows ? 2 : 0) + (o_rows ? 1 : 0)], "sketch_product_batched", lds, 0, units);
    ProfScope ps(c, "op:batched_sketch_product %dx%d l=%d count=%d grid=%lld slots=%lld plan=units=%lld,rows=%d,cols=%d,scratch=%d", m, n, l, (int)count,
                 (long long)lch.grid, (long long)lch.slots, (long long)units, BSI_ROWS, BSI_COLS, lch.scratch);
    BspArgs<T> g;
    g.a = a; g.omega = omega; g.y = y;
    g.abs = abs; g.obs = obs; g.ybs = ybs;
    g.units = units; g.panels = panels;
    lch.launch(g);
}

template void batched_sketch_product<double>(rc_context *, Mat<double>, int64_t, Mat<double>, int64_t, int32_t, Mat<double>, int64_t);
template void batched_sketch_product<float>(rc_context *, Mat<float>, int64_t, Mat<float>, int64_t, int32_t, Mat<float>, int64_t);

RC_INSTANTIATE_BATCHED_SKETCH(double, float)
RC_INSTANTIATE_BATCHED_RECOMPRESS(double, float)
RC_INSTANTIATE_BATCHED_ID_SVD(double, float)

}  // namespace rc
