// Batched column and two-sided IDs and truncated SVDs of many small same-shaped COMPLEX matrices in one launch
// (rc_column_id_rank_batched_c64 / _c32, rc_two_sided_id_rank_batched_c64 / _c32, rc_svd_rank_batched_c64 / _c32), and the
// recompression of complex low-rank factors (rc_lowrank_recompress_complex_batched_c64 / _c32 and, for tall left factors,
// rc_lowrank_recompress_tall_complex_batched_c64 / _c32, for two tall factors rc_lowrank_recompress_complex_large_batched_c64 / _c32:
// k_batched_recompress_c<R, TALL, LARGE> below) and the sketched
// column ID of complex tall blocks (rc_sketch_column_id_rank_complex_batched_c64 / _c32, k_batched_sketch_id_c below) and the range step
// of their power iteration (rc_sketch_range_step_complex_batched_c64 / _c32, k_batched_range_step_c below).
//
// The structure of kernels_batched_id.hip (one persistent workgroup of 256 threads per matrix, the same three device stages, the same
// grid and workspace rule, and the launch path of rc_batched_launch.hpp).  The stages that read the same for real and complex elements
// are that file's too: they stand once in batched_stages.hpp, which this file instantiates for cplx<double> and cplx<float> (the fill,
// the norms, bid_qrcp, bid_z, k_batched_id and k_batched_two_sided with their plans, bsv_jacobi, brt_stack_load).
// Here stay the complex family's own routines (bic_apply, bsc_round, bsc_phase, the form_u routines, the core products) and the SVD,
// recompression, sketch and range-step kernels.  No plan and no launcher body stands here: they are written once for all four element
// types in batched_launchers.hpp, and the file ends with what they take from this family (ComplexFamily: the Args structs, the LDS and
// workspace sizes and the instance to launch) and their instantiation for cplx<double> and cplx<float>.  The arithmetic is that of the lone complex path in rc_complex.hip:
//   * interleaved (re, im) data (cplx<R>, CV<R> and their arithmetic: rc_cplx.hpp); the partial norms vn1 / vn2 are real, W and the tile complex;
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
// The truncated SVD (k_batched_svd_c) runs the first two stages to all N steps, then k_batched_svd's complex Jacobi and U forming (see
// its comment below).
//
// Every operation below commutes exactly with negating all imaginary parts (round to nearest is sign-symmetric, and each real part
// is even, each imaginary part odd in the imaginary inputs), so conj(A) gives the same permutations and ranks and the conjugate
// of every factor, bit for bit.
#include "batched_launchers.hpp"
#include "batched_stages.hpp"
#include "rc_batched_launch.hpp"
#include "rc_common.hpp"
#include "rc_cplx.hpp"
#include "rc_device.hpp"
#include "rc_gemm.hpp"

namespace rc {

namespace {

// H_j^H = I - conj(tau) v v^H applied to the trailing columns p = j+1 .. n-1, one wave per column; rows j + lane + 64 e of the column
// in registers (NE * 64 >= m - j), then the ?laqp2 down-date of the column's partial norm with |x_j|
template <typename R, int NE>
__device__ __forceinline__ void bic_apply(cplx<R> *W, int ldw, int m, int n, int j, const int *jp, R *vn1, R *vn2, cplx<R> tj, int wv, int lane) {
    const int mrem = m - j;
    const cplx<R> *vc = W + (size_t)jp[j] * ldw + j;
    cplx<R> v[NE];
#pragma unroll
    for (int e = 0; e < NE; ++e) {
        // branch-free: lanes past the end read row j (always valid) and are masked by a select
        const int li = lane + 64 * e;
        const bool ok = li < mrem;
        const cplx<R> vv = vc[ok ? li : 0];
        v[e] = ok ? (li == 0 ? cone<R>() : vv) : czero<R>();
    }
    const bool reflect = tj.re != (R)0 || tj.im != (R)0;  // tau == 0: H = I
    const cplx<R> ctj = cj(tj);
    for (int p = j + 1 + wv; p < n; p += BID_WAVES) {
        cplx<R> *xc = W + (size_t)jp[p] * ldw + j;
        cplx<R> x[NE];
#pragma unroll
        for (int e = 0; e < NE; ++e) {
            const int li = lane + 64 * e;
            const bool ok = li < mrem;
            const cplx<R> xv = xc[ok ? li : 0];
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
            const cplx<R> f = ctj * cplx<R>{wave_sum_dpp(dre), wave_sum_dpp(dim)};
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
            const cplx<R> x0{read_lane(x[0].re, 0), read_lane(x[0].im, 0)};
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

// ---- batched truncated SVD (rc_svd_rank_batched_c64 / _c32) --------------------------------------------------------------------
// k_batched_svd's stages with the arithmetic above.  Per matrix, in the tall orientation M x N (N = min(m, n)): the pivoted QR of
// bid_qrcp run to N steps (W P = Q R with Q = H_0 .. H_{N-1}, the complex tau_j kept), one-sided Jacobi on the N x N core G = R^H
// (the rows of the graded R, as the real kernel takes R^T) with the rotations accumulated in J: G J = U_G S, so R = J S U_G^H;
// singular values = the column norms of G, U = Q [J_k; 0] with the k kept columns in registers, and V_W[jp[i], :] = (G S^-1)[i, :].
// A wide matrix is read through its plain (unconjugated) transposed view: A^T = U' S V'^H gives A = conj(V') S U'^T, so u is the work
// orientation's V^H written through u^T and vt its U written through vt^T, no conjugation on either side.  A Jacobi step on (g_p, g_q)
// turns g_q by the phase e^{-i phi} = conj(apq) / |apq| (apq = g_p^H g_q; evaluated in f64 and rounded, as k_c_jacobi_round does),
// then takes the real rotation of (app, aqq, |apq|).  Everything stays inside one workgroup.

// Jacobi rows per lane of a 16-lane pair group (N <= 16 NE): the complex twin of bsv_round
// (both threshold tests are evaluated in f64 on |apq|^2 formed in f64, as bsv_round's are, so that in c32 two columns of norm 1e-9
// or less, whose app aqq and |apq|^2 pass the smallest f32 number, are still rotated until they are orthogonal)
template <typename R, int NE>
__device__ __forceinline__ void bsc_round(cplx<R> *G, int ldg, cplx<R> *J, int ldj, int N, int p, int q, R tol, R tol2, int ll, int *flag) {
    cplx<R> *gp = G + (size_t)p * ldg, *gq = G + (size_t)q * ldg;
    cplx<R> a[NE], b[NE];
    R app = 0, aqq = 0, are = 0, aim = 0;  // apq = g_p^H g_q = (are, aim)
#pragma unroll
    for (int e = 0; e < NE; ++e) {
        const int i = ll + 16 * e;
        a[e] = i < N ? gp[i] : czero<R>();
        b[e] = i < N ? gq[i] : czero<R>();
        app = fma(a[e].re, a[e].re, app);
        app = fma(a[e].im, a[e].im, app);
        aqq = fma(b[e].re, b[e].re, aqq);
        aqq = fma(b[e].im, b[e].im, aqq);
        are = fma(a[e].re, b[e].re, are);
        are = fma(a[e].im, b[e].im, are);
        aim = fma(a[e].re, b[e].im, aim);
        aim = fma(-a[e].im, b[e].re, aim);
    }
    app = group_sum_dpp<16>(app);
    aqq = group_sum_dpp<16>(aqq);
    are = group_sum_dpp<16>(are);
    aim = group_sum_dpp<16>(aim);
    // bsv_round's test with |apq|^2: rotate iff |apq| > tol sqrt(app aqq) (uniform over the 16 lanes)
    const double h2 = (double)are * (double)are + (double)aim * (double)aim;
    if (!jacobi_pair_is_coupled(app, aqq, h2, tol2)) return;
    const double hd = sqrt(h2), ih = 1.0 / hd;
    const cplx<R> ph{(R)((double)are * ih), (R)(-((double)aim * ih))};  // e^{-i phi}
    double cd, sd;
    jacobi_rotation<double>((double)app, (double)aqq, hd, cd, sd);
    const R c = (R)cd, s = (R)sd;
    cplx<R> *vp = J + (size_t)p * ldj, *vq = J + (size_t)q * ldj;
#pragma unroll
    for (int e = 0; e < NE; ++e) {
        const int i = ll + 16 * e;
        if (i < N) {
            const cplx<R> bq = ph * b[e];
            gp[i] = cplx<R>{c * a[e].re - s * bq.re, c * a[e].im - s * bq.im};
            gq[i] = cplx<R>{s * a[e].re + c * bq.re, s * a[e].im + c * bq.im};
            const cplx<R> x = vp[i], y = ph * vq[i];
            vp[i] = cplx<R>{c * x.re - s * y.re, c * x.im - s * y.im};
            vq[i] = cplx<R>{s * x.re + c * y.re, s * x.im + c * y.im};
        }
    }
    if (ll == 0 && jacobi_rotation_was_large(app, aqq, h2, s, tol)) *flag = 2;  // plain store: every writer writes 2
}

// the phase rule on a column held by one wave (x[e] at output row orow(e), -1: none): i* = the first output row of the largest
// |x|^2; the column is multiplied by ph = conj(x_i*) / |x_i*| (f64, rounded) and x_i* becomes exactly (|x_i*|, 0).  Returns ph;
// (1, 0) with the column unchanged when |x_i*| is not positive and finite (a zero or non-finite column)
template <typename R, int NE, typename Row>
__device__ __forceinline__ cplx<R> bsc_phase(cplx<R> (&x)[NE], Row orow, int lane) {
    R mx = 0;
#pragma unroll
    for (int e = 0; e < NE; ++e)
        if (orow(e) >= 0) mx = max(mx, abs2(x[e]));
    mx = wave_max_dpp(mx);
    int key = 0x7fffffff;
#pragma unroll
    for (int e = 0; e < NE; ++e) {
        const int o = orow(e);
        if (o >= 0 && abs2(x[e]) == mx) key = min(key, o);
    }
    key = wave_min_dpp(key);
    int who = 0x7fffffff;  // the lane and element holding row key
#pragma unroll
    for (int e = 0; e < NE; ++e)
        if (key != 0x7fffffff && orow(e) == key) who = 64 * e + lane;
    who = wave_min_dpp(who);
    if (who == 0x7fffffff) return cone<R>();
    cplx<R> xs = czero<R>();
#pragma unroll
    for (int e = 0; e < NE; ++e)
        if (e == (who >> 6)) xs = cplx<R>{read_lane(x[e].re, who & 63), read_lane(x[e].im, who & 63)};
    const double md = hypot((double)xs.re, (double)xs.im);
    if (!(md > 0.0 && md <= 1.7976931348623157e308)) return cone<R>();
    const cplx<R> ph{(R)((double)xs.re / md), (R)(-((double)xs.im / md))};
    const R mr = (R)md;
#pragma unroll
    for (int e = 0; e < NE; ++e) x[e] = orow(e) == key ? cplx<R>{mr, (R)0} : x[e] * ph;
    return ph;
}

// U[:, c] = Q [J[:, srt[c]]; 0] times its phase for the kept columns c < r (zero for r <= c < k): one wave per column, the M rows in
// registers (row lane + 64 e), the N reflectors applied backward as x -= tau_j v_j (v_j^H x) (Q = H_0 .. H_{N-1}: the factorization
// applied H_j^H, forming Q applies H_j), v_j in W's column jp[j] below row j.  phase_here: the phase rule is applied to this column
// and its phase stored in phs[c]; otherwise the column is multiplied by conj(phs[c]).
template <typename R, int NE>
__device__ __forceinline__ void bsc_form_u(const cplx<R> *W, int ldw, const cplx<R> *J, int ldj, int M, int N, int k, int r, const int *jp, const cplx<R> *taus,
                                           const int *srt, cplx<R> *phs, bool phase_here, cplx<R> *U, int64_t urs, int64_t ucs, int wv, int lane) {
    for (int c = wv; c < k; c += BID_WAVES) {
        cplx<R> *uc = U + (int64_t)c * ucs;
        if (c >= r) {
            for (int i = lane; i < M; i += 64) uc[i * urs] = czero<R>();
            continue;
        }
        const cplx<R> *jc = J + (size_t)srt[c] * ldj;
        cplx<R> x[NE];
#pragma unroll
        for (int e = 0; e < NE; ++e) {
            const int i = lane + 64 * e;
            x[e] = i < N ? jc[i] : czero<R>();
        }
        for (int j = N - 1; j >= 0; --j) {
            const cplx<R> tau = taus[j];
            if (tau.re == (R)0 && tau.im == (R)0) continue;  // H_j = I (uniform)
            const cplx<R> *vc = W + (size_t)jp[j] * ldw;
            cplx<R> v[NE];
            R dre = 0, dim = 0;  // v^H x
#pragma unroll
            for (int e = 0; e < NE; ++e) {
                const int i = lane + 64 * e;
                const cplx<R> vv = vc[i < M ? i : j];  // branch-free: lanes out of range read row j and are masked below
                v[e] = i > j && i < M ? vv : (i == j ? cone<R>() : czero<R>());
                dre = fma(v[e].re, x[e].re, dre);
                dre = fma(v[e].im, x[e].im, dre);
                dim = fma(v[e].re, x[e].im, dim);
                dim = fma(-v[e].im, x[e].re, dim);
            }
            const cplx<R> f = tau * cplx<R>{wave_sum_dpp(dre), wave_sum_dpp(dim)};
#pragma unroll
            for (int e = 0; e < NE; ++e) {
                x[e].re = fma(-f.re, v[e].re, x[e].re);
                x[e].re = fma(f.im, v[e].im, x[e].re);
                x[e].im = fma(-f.re, v[e].im, x[e].im);
                x[e].im = fma(-f.im, v[e].re, x[e].im);
            }
        }
        if (phase_here) {
            const cplx<R> ph = bsc_phase<R, NE>(x, [&](int e) { const int i = lane + 64 * e; return i < M ? i : -1; }, lane);
            if (lane == 0) phs[c] = ph;
        } else {
            const cplx<R> ph = cj(phs[c]);
#pragma unroll
            for (int e = 0; e < NE; ++e) x[e] = x[e] * ph;
        }
#pragma unroll
        for (int e = 0; e < NE; ++e) {
            const int i = lane + 64 * e;
            if (i < M) uc[i * urs] = x[e];
        }
    }
}

// LDS of k_batched_svd_c: [W: N x (M|1), W_LDS only] [G: N x ldg, G_LDS only] [J: N x ldg, V_LDS only] taus[N] phs[128] complex
// | vn1[N] vn2[N] sig[N] red[8] real | jp[N] srt[N] flag[4]
template <typename R>
size_t bsc_lds_bytes(int M, int N, int ldg, bool w_lds, bool v_lds, bool g_lds) {
    size_t c = (size_t)N + 128;
    if (w_lds) c += (size_t)N * (size_t)(M | 1);
    if (g_lds) c += (size_t)N * ldg;
    if (v_lds) c += (size_t)N * ldg;
    return c * sizeof(cplx<R>) + ((size_t)3 * N + 8) * sizeof(R) + (size_t)(2 * N + 4) * sizeof(int);
}
// complex elements of one workgroup's workspace slot: W (M x N), G (N x ldg), J (N x N), each unless it is in LDS
__host__ __device__ inline size_t bsc_ws_elems(int M, int N, int ldg, bool w_lds, bool v_lds, bool g_lds) {
    return (w_lds ? 0 : (size_t)M * N) + (g_lds ? 0 : (size_t)N * ldg) + (v_lds ? 0 : (size_t)N * N);
}

// a: m x n input view; uo (M x k) and vo (k x N) are the views the work orientation's U and V^H go to (u and vt for a tall matrix,
// vt^T and u^T for a wide one), each moved by its own batch stride; s (count x N) and ranks contiguous.  W_LDS / G_LDS / V_LDS: the
// working copy W / the core G / the rotations J live in LDS, else in the workgroup's workspace slot (in that order, ldg = N there).
template <typename R, bool W_LDS, bool V_LDS, bool G_LDS>
__global__ __launch_bounds__(BID_THREADS) void k_batched_svd_c(CV<R> a, int64_t abs, int count, int k, double tol, CV<R> uo, int64_t ubs, CV<R> vo,
                                                               int64_t vbs, R *__restrict__ s_out, int64_t *__restrict__ ranks, cplx<R> *__restrict__ ws,
                                                               int *health, int ldg) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const bool wide = a.rows < a.cols;
    const int M = (int)(wide ? a.cols : a.rows), N = (int)(wide ? a.rows : a.cols);
    const int ldw = W_LDS ? (M | 1) : M, ldj = V_LDS ? ldg : N;
    cplx<R> *lp = reinterpret_cast<cplx<R> *>(smem_raw);                                    // next free LDS element
    cplx<R> *wp = ws + (size_t)blockIdx.x * bsc_ws_elems(M, N, ldg, W_LDS, V_LDS, G_LDS);  // next free element of the workspace slot
    cplx<R> *W, *G, *J;
    if (W_LDS) { W = lp; lp += (size_t)N * ldw; } else { W = wp; wp += (size_t)N * ldw; }
    if (G_LDS) { G = lp; lp += (size_t)N * ldg; } else { G = wp; wp += (size_t)N * ldg; }
    if (V_LDS) { J = lp; lp += (size_t)N * ldj; } else { J = wp; }
    cplx<R> *taus = lp, *phs = taus + N;
    R *vn1 = reinterpret_cast<R *>(phs + 128);
    R *vn2 = vn1 + N, *sig = vn2 + N, *red = sig + N;
    int *jp = reinterpret_cast<int *>(red + 8);
    int *srt = jp + N, *flag = srt + N;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    // the input in the work orientation and its fast direction
    const int64_t ars = wide ? a.cs : a.rs, acs = wide ? a.rs : a.cs;

    for (int b = blockIdx.x; b < count; b += gridDim.x) {
        const cplx<R> *__restrict__ A = a.p + (int64_t)b * abs;
        // ---- QR: W P = Q R, all N steps (exact zero pivots are steps with H = I), complex taus kept -------------------------------
        const int e2 = bid_load_pow2(W, ldw, M, N, ars <= acs, [&](int i, int c) { return A[i * ars + c * acs]; }, vn1, vn2, jp, red + 4, wv, lane);
        bid_qrcp<cplx<R>, true>(W, ldw, M, N, N, 0.0, jp, vn1, vn2, red, tid, wv, lane, taus);
        // ---- core G = R^H (R in pivoted column order: G[:, j] = conj(row j of R)) and J = I -----------------------------------------
        for (int j = wv; j < N; j += BID_WAVES) {
            for (int i = lane; i < N; i += 64) {
                G[(size_t)j * ldg + i] = i >= j ? cj(W[(size_t)jp[i] * ldw + j]) : czero<R>();
                J[(size_t)j * ldj + i] = i == j ? cone<R>() : czero<R>();
            }
        }
        __syncthreads();
        bool conv;
        if (N <= 16) conv = bsv_jacobi<cplx<R>, 1>(G, ldg, J, ldj, N, tid, flag);
        else if (N <= 32) conv = bsv_jacobi<cplx<R>, 2>(G, ldg, J, ldj, N, tid, flag);
        else if (N <= 64) conv = bsv_jacobi<cplx<R>, 4>(G, ldg, J, ldj, N, tid, flag);
        else conv = bsv_jacobi<cplx<R>, 8>(G, ldg, J, ldj, N, tid, flag);
        if (!conv && tid == 0) atomicOr(health, 16);  // the sweep budget ran out: bit 16, as the lone Jacobi reports it
        // ---- singular values: column norms, sorted descending (a strict total order: NaN last, ties by column) ----------------------
        for (int j = tid >> 4; j < N; j += BID_THREADS / 16) {
            const cplx<R> *gj = G + (size_t)j * ldg;
            R acc = 0;
            for (int i = tid & 15; i < N; i += 16) {
                acc = fma(gj[i].re, gj[i].re, acc);
                acc = fma(gj[i].im, gj[i].im, acc);
            }
            acc = group_sum_dpp<16>(acc);
            if ((tid & 15) == 0) sig[j] = sqrt(acc);
        }
        __syncthreads();
        R *sb = s_out + (int64_t)b * N;
        for (int i = tid; i < N; i += BID_THREADS) {
            const R ki = sig[i] >= (R)0 ? sig[i] : (R)-1;
            int pos = 0;
            for (int j = 0; j < N; ++j) {
                const R kj = sig[j] >= (R)0 ? sig[j] : (R)-1;
                pos += (kj > ki || (kj == ki && j < i)) ? 1 : 0;
            }
            srt[pos] = i;
            sb[pos] = ldexp(sig[i], e2);  // W was 2^-e2 times the block: the one output that carries its scale
        }
        __syncthreads();
        // ---- rank: the first j < k with s_j == 0 or (tol > 0 and s_j / s_0 < tol), else k ---------------------------------------
        if (tid == 0) {
            const R s0 = sig[srt[0]];
            int r = k;
            for (int j = 0; j < k; ++j) {
                const R sj = sig[srt[j]];
                if (sj == (R)0 || (tol > 0.0 && (double)(sj / s0) < tol)) { r = j; break; }
            }
            flag[1] = r;
            ranks[b] = r;
        }
        __syncthreads();
        const int r = flag[1];
        cplx<R> *Vb = vo.p + (int64_t)b * vbs;
        // ---- phases on the caller's u.  Wide: u[:, c] is row c of vo, u[jp[i], c] = conj(G[i, srt[c]]) / s_c; its phase is fixed
        // and the row written here, before U is formed.  Tall: in bsc_form_u. ------------------------------------------------------
        if (wide) {
            for (int c = wv; c < k; c += BID_WAVES) {
                const int j0 = c < r ? srt[c] : 0;
                const cplx<R> *gc = G + (size_t)j0 * ldg;
                const R sj = sig[j0], inv = sj > (R)0 ? (R)1 / sj : (R)0;
                cplx<R> x[2];
#pragma unroll
                for (int e = 0; e < 2; ++e) {
                    const int i = lane + 64 * e;
                    const cplx<R> g = i < N ? gc[i] : czero<R>();
                    x[e] = c < r ? cplx<R>{g.re * inv, -(g.im * inv)} : czero<R>();
                }
                if (c < r) {
                    const cplx<R> ph = bsc_phase<R, 2>(x, [&](int e) { const int i = lane + 64 * e; return i < N ? jp[i] : -1; }, lane);
                    if (lane == 0) phs[c] = ph;
                }
#pragma unroll
                for (int e = 0; e < 2; ++e) {
                    const int i = lane + 64 * e;
                    if (i < N) Vb[c * vo.rs + (int64_t)jp[i] * vo.cs] = x[e];
                }
            }
            __syncthreads();
        }
        // ---- U = Q [J_k; 0] straight into the output view -------------------------------------------------------------------------
        cplx<R> *Ub = uo.p + (int64_t)b * ubs;
        if (M <= 64) bsc_form_u<R, 1>(W, ldw, J, ldj, M, N, k, r, jp, taus, srt, phs, !wide, Ub, uo.rs, uo.cs, wv, lane);
        else if (M <= 128) bsc_form_u<R, 2>(W, ldw, J, ldj, M, N, k, r, jp, taus, srt, phs, !wide, Ub, uo.rs, uo.cs, wv, lane);
        else if (M <= 256) bsc_form_u<R, 4>(W, ldw, J, ldj, M, N, k, r, jp, taus, srt, phs, !wide, Ub, uo.rs, uo.cs, wv, lane);
        else bsc_form_u<R, 8>(W, ldw, J, ldj, M, N, k, r, jp, taus, srt, phs, !wide, Ub, uo.rs, uo.cs, wv, lane);
        if (!wide) {
            __syncthreads();  // phs is written in bsc_form_u
            // ---- V^H: row c of vo is conj(V_W[:, c] ph_c), V_W[jp[i], c] = G[i, srt[c]] / s_c; rows r..k-1 zero ----------------------
            for (int c = wv; c < k; c += BID_WAVES) {
                const int j0 = c < r ? srt[c] : 0;
                const cplx<R> *gc = G + (size_t)j0 * ldg;
                const R sj = sig[j0], inv = sj > (R)0 ? (R)1 / sj : (R)0;
                const cplx<R> ph = c < r ? phs[c] : czero<R>();
                for (int i = lane; i < N; i += 64) {
                    const cplx<R> t = gc[i] * ph;
                    Vb[c * vo.rs + (int64_t)jp[i] * vo.cs] = c < r ? cplx<R>{t.re * inv, -(t.im * inv)} : czero<R>();
                }
            }
        }
        __syncthreads();  // W, G, J and the small arrays are rewritten by the next matrix
    }
}

// ---- batched recompression of complex low-rank factors (rc_lowrank_recompress_complex_batched_c64 / _c32) ----------------------
// k_batched_recompress's stages with the arithmetic above.  Per block, with q = in_ranks[b] clamped to [0, K]:
// A = left[:, :q] mid[:q, :q] diag(s[:q]) right[:q, :] (nothing conjugated, s real) is never formed.  The two thin factors are
// factored where they stand, left[:, :q] P_L = Q_L R_L and the PLAIN transpose right[:q, :]^T P_R = Q_R R_R (bid_qrcp to q steps
// each, reflectors and the complex taus kept).  With Rl = R_L P_L^T and Rr = R_R P_R^T:
//     left = Q_L Rl,  right = Rr^T Q_R^T,  A = Q_L C Q_R^T,  C = Rl mid diag(s) Rr^T   (q x q, no conjugate anywhere).
// One-sided Jacobi on G = C^H with the rotations in J: G J = V_c Sigma, so C = J Sigma V_c^H and
//     A = (Q_L J) Sigma (conj(Q_R) V_c)^H:  U = Q_L [J; 0],  vt = V^H = V_c^H Q_R^T = (Q_R conj(V_c))^T.
// The transpose rather than right^H: vt is then the transposed view of Q_R [conj(V_c); 0], which bsc_form_u writes as it stands once
// the kept columns of G are conjugated in the 1 / sigma scaling pass; with u's phases, u_c -> u_c ph_c needs vt's row c times
// conj(ph_c), which is what bsc_form_u(phase_here = false) multiplies by.  Factoring right^H instead would need a conjugating store.
// G = C^H, not C: an exactly zero column of left is pivoted last and is a step with H = I, which leaves a zero row in R_L, hence a
// zero row of C = a zero column of G, and the rotation test (false for apq = 0) never touches a zero column: its singular value
// comes out as exactly 0.
//
// The core is formed by two q x q x q products, one thread per element, summed over the inner index in ascending order, each term one
// complex FMA in a fixed order (re += a.re b.re, re -= a.im b.im, im += a.re b.im, im += a.im b.re):
//   T1[a, j] = sum_b (mid[a, b] s[b]) Rr[j, b]   (T1 in J's place: J = I only afterwards)
//   C[i, j]  = sum_a Rl[i, a] T1[a, j]           (stored conjugated as G[i * ldg + j]: column i of G = conj(row i of C))
// where Rl[:, c] is the upper-triangular column the factorization keeps for the factor's own column c (rows 0 .. ip[c] of the
// working copy's column c, ip the inverse of the pivot order), Rr likewise.  The lanes run along j: T1, Wr and G are read and
// written at consecutive addresses and mid[a, b], Rl[i, a] are one broadcast address per wave.
// The Jacobi's threshold tests are evaluated in f64 (bsc_round), as the real recompression's are.

template <typename R>
struct BrcCArgs {
    CV<R> left, mid, right, u, vt;
    int64_t lbs, mbs, rbs, ubs, vbs, s_stride;
    const R *s;
    const int64_t *in_ranks;
    R *s_out;
    int64_t *ranks;
    cplx<R> *ws;
    int *health;
    double tol;
    int count, k, ldg;
    bool l_lds, r_lds, v_lds, g_lds;  // the copy of left / of right^T / the rotations J / the core G in LDS (else in the workspace slot)
};

// LDS: [Wl: K x (m|1)] [Wr: K x (n|1)] [G: K x ldg] [J: K x ldg] (each only when its flag is set) taul[K] taur[K] phs[128] complex
// | vn1[K] vn2[K] sig[K] red[8] real | jpl[K] jpr[K] ipl[K] ipr[K] srt[K] flag[4]
template <typename R>
size_t brcc_lds_bytes(int m, int n, int K, int ldg, bool l_lds, bool r_lds, bool v_lds, bool g_lds) {
    size_t c = (size_t)2 * K + 128;
    if (l_lds) c += (size_t)K * (size_t)(m | 1);
    if (r_lds) c += (size_t)K * (size_t)(n | 1);
    if (g_lds) c += (size_t)K * ldg;
    if (v_lds) c += (size_t)K * ldg;
    return c * sizeof(cplx<R>) + ((size_t)3 * K + 8) * sizeof(R) + (size_t)(5 * K + 4) * sizeof(int);
}
// complex elements of one workgroup's workspace slot: Wl (m x K), Wr (n x K), G (K x ldg), J (K x K), each unless it is in LDS
__host__ __device__ inline size_t brcc_ws_elems(int m, int n, int K, int ldg, bool l_lds, bool r_lds, bool v_lds, bool g_lds) {
    return (l_lds ? 0 : (size_t)m * K) + (r_lds ? 0 : (size_t)n * K) + (g_lds ? 0 : (size_t)K * ldg) + (v_lds ? 0 : (size_t)K * K);
}

// ---- tall left factors (rc_lowrank_recompress_tall_complex_batched_c64 / _c32, m <= 65536) --------------------------------------------------
// k_batched_recompress<T, true>'s scheme (kernels_batched_id.hip) on complex elements: left[:, :q] is factored by a flat Householder TSQR with
// stored reflectors inside the one workgroup.  Stage 0 is bid_qrcp on rows 0 .. min(m, H) - 1, H = BRT_H = 512 rows.  Stage s >= 1 factors a
// stack: the upper triangle of the previous stage's R (q rows, the real diagonal (beta, 0) as bid_qrcp leaves it, exact zeros below) on top of
// the next min(H - q, rows left) rows of left, by the same q pivoted steps.  The factor's column c sits at physical column c of every stack and
// jpl (position -> physical column) is carried from stage to stage, so after the last stage (the last stage's copy, jpl) stand where (Wl, jpl)
// stand in the core products.  An exactly zero column of left is an exactly zero column of every stack: pivoted last, tau = 0, a zero row of the
// last R.  The stage height depends on q, not on K: a block's bits are those of a call of inner width q.  Every stage's factored copy, complex
// taus and pivots stay in the workgroup's slot (brt_stage_elems(K) complex elements each) for the backward pass, brtc_form_u.  m <= H is one
// stage, which is the kernel below with TALL = false: the launcher sends such shapes to that instance, so the TALL instances only ever see
// m > H, that is two stages or more at every inner rank.
__host__ __device__ inline size_t brtc_ws_elems(int m, int n, int K, int ldg, bool l_lds, bool r_lds, bool v_lds, bool g_lds) {
    if (m <= BRT_H) return brcc_ws_elems(m, n, K, ldg, l_lds, r_lds, v_lds, g_lds);
    return (size_t)brt_stages(m, K) * brt_stage_elems(K) + brcc_ws_elems(0, n, K, ldg, true, r_lds, v_lds, g_lds);
}

// x <- H_0 .. H_{N-1} x for a column held by one wave (row lane + 64 e in x[e], M rows): bsc_form_u's reflector loop, FMA for FMA, as a routine
// of its own for a column that goes through several factorizations (bsc_form_u keeps its loop, as bsv_form_u does beside bsv_reflect_back)
template <typename R, int NE>
__device__ __forceinline__ void bsc_reflect_back(const cplx<R> *W, int ldw, int M, int N, const int *jp, const cplx<R> *taus, cplx<R> (&x)[NE], int lane) {
    for (int j = N - 1; j >= 0; --j) {
        const cplx<R> tau = taus[j];
        if (tau.re == (R)0 && tau.im == (R)0) continue;  // H_j = I (uniform)
        const cplx<R> *vc = W + (size_t)jp[j] * ldw;
        cplx<R> v[NE];
        R dre = 0, dim = 0;  // v^H x
#pragma unroll
        for (int e = 0; e < NE; ++e) {
            const int i = lane + 64 * e;
            const cplx<R> vv = vc[i < M ? i : j];  // branch-free: lanes out of range read row j and are masked below
            v[e] = i > j && i < M ? vv : (i == j ? cone<R>() : czero<R>());
            dre = fma(v[e].re, x[e].re, dre);
            dre = fma(v[e].im, x[e].im, dre);
            dim = fma(v[e].re, x[e].im, dim);
            dim = fma(-v[e].im, x[e].re, dim);
        }
        const cplx<R> f = tau * cplx<R>{wave_sum_dpp(dre), wave_sum_dpp(dim)};
#pragma unroll
        for (int e = 0; e < NE; ++e) {
            x[e].re = fma(-f.re, v[e].re, x[e].re);
            x[e].re = fma(f.im, v[e].im, x[e].re);
            x[e].im = fma(-f.re, v[e].im, x[e].im);
            x[e].im = fma(-f.im, v[e].re, x[e].im);
        }
    }
}

// U[:, c] = ph_c Q_0 [Q_1 [.. Q_{S-1} [J[:, srt[c]]; 0] ..; 0]; 0] for S >= 2 stages at stage0 + s * se: one wave per kept column carries x (q
// complex values, 8 per lane) down the stages.  Stage s >= 1 applies its reflectors to [x; 0] (H rows in registers); rows q .. of the result are
// that chunk's rows of u and are written as they are, rows 0 .. q - 1 replace x; stage 0's result fills rows 0 .. H - 1.
// The phase rule runs over all m rows: per chunk the largest abs2 in the working type and the first output row that attains it (bsc_phase's
// key); the chunks are visited from the last rows to the first, so a chunk whose maximum is >= the best so far takes over, which makes the
// winner the first of the largest-modulus entries.  ph = conj(x*) / |x*| as in bsc_phase (f64 hypot, rounded); (1, 0) for a zero or non-finite
// column.  Stage 0's rows are multiplied by ph in registers before they are written; every chunk written earlier is re-read and multiplied by
// the lanes that wrote it (the same element of the same lane: no other lane's store is read back).  The pivot entry becomes exactly (|x*|, 0)
// in whichever chunk holds it.  Every product is operator* of rc_cplx.hpp, so conjugating the inputs conjugates the column bit for bit.
template <typename R>
__device__ __forceinline__ void brtc_form_u(const cplx<R> *stage0, size_t se, int S, int K, int q, int m, const cplx<R> *J, int ldj, int k, int r, const int *srt,
                                            cplx<R> *phs, cplx<R> *U, int64_t urs, int64_t ucs, int wv, int lane) {
    constexpr int NE = BRT_H / 64;
    for (int c = wv; c < k; c += BID_WAVES) {
        cplx<R> *uc = U + (int64_t)c * ucs;
        if (c >= r) {
            for (int i = lane; i < m; i += 64) uc[i * urs] = czero<R>();
            continue;
        }
        const cplx<R> *jc = J + (size_t)srt[c] * ldj;
        cplx<R> x[NE];
#pragma unroll
        for (int e = 0; e < NE; ++e) {
            const int i = lane + 64 * e;
            x[e] = i < q ? jc[i] : czero<R>();
        }
        R best = (R)-1;
        int brow = 0x7fffffff;       // the output row of x*
        cplx<R> xs = czero<R>();  // x*
        for (int s = S - 1; s >= 0; --s) {
            const cplx<R> *Ws = stage0 + (size_t)s * se, *ts = Ws + (size_t)BRT_H * K;
            const int top = s ? q : 0, base = s ? BRT_H + (s - 1) * (BRT_H - q) : 0;
            const int hs = top + min(BRT_H - top, m - base);
            bsc_reflect_back<R, NE>(Ws, BRT_H, hs, q, reinterpret_cast<const int *>(ts + K), ts, x, lane);
            R mx = 0;
#pragma unroll
            for (int e = 0; e < NE; ++e) {
                const int i = lane + 64 * e;
                if (i >= top && i < hs) mx = max(mx, abs2(x[e]));
            }
            mx = wave_max_dpp(mx);
            int who = 0x7fffffff;  // 64 e + lane of the chunk's first row of abs2 == mx: rows ascend with 64 e + lane
#pragma unroll
            for (int e = 0; e < NE; ++e) {
                const int i = lane + 64 * e;
                if (i >= top && i < hs && abs2(x[e]) == mx) who = min(who, i);
            }
            who = wave_min_dpp(who);
            if (who != 0x7fffffff && mx >= best) {  // uniform; this chunk's rows precede every chunk seen so far
                best = mx;
                brow = base + who - top;
#pragma unroll
                for (int e = 0; e < NE; ++e)
                    if (e == (who >> 6)) xs = cplx<R>{read_lane(x[e].re, who & 63), read_lane(x[e].im, who & 63)};
            }
            if (s) {
#pragma unroll
                for (int e = 0; e < NE; ++e) {
                    const int i = lane + 64 * e;
                    if (i >= top && i < hs) uc[(int64_t)(base + i - top) * urs] = x[e];
                    x[e] = i < top ? x[e] : czero<R>();
                }
            }
        }
        const double md = hypot((double)xs.re, (double)xs.im);
        const bool turn = brow != 0x7fffffff && md > 0.0 && md <= 1.7976931348623157e308;
        const cplx<R> ph = turn ? cplx<R>{(R)((double)xs.re / md), (R)(-((double)xs.im / md))} : cone<R>();
        const cplx<R> piv{(R)md, (R)0};
        if (lane == 0) phs[c] = ph;
#pragma unroll
        for (int e = 0; e < NE; ++e) {
            const int i = lane + 64 * e;  // stage 0 of S >= 2 stages holds H rows
            uc[(int64_t)i * urs] = !turn ? x[e] : i == brow ? piv : x[e] * ph;
        }
        if (turn) {
            for (int s = 1; s < S; ++s) {
                const int base = BRT_H + (s - 1) * (BRT_H - q), hs = q + min(BRT_H - q, m - base);
#pragma unroll
                for (int e = 0; e < NE; ++e) {
                    const int i = lane + 64 * e;
                    if (i >= q && i < hs) {
                        cplx<R> *p = uc + (int64_t)(base + i - q) * urs;
                        *p = base + i - q == brow ? piv : *p * ph;
                    }
                }
            }
        }
    }
}

// ---- both factors tall (rc_lowrank_recompress_complex_large_batched_c64 / _c32, m, n <= 65536) -------------------------------------------------
// k_batched_recompress<T, true, true>'s scheme (kernels_batched_id.hip) on complex elements: for n > H the plain transpose right[:q, :]^T (n x q)
// goes through the stages above, jpr carried from stage to stage, every stage's copy, complex taus and pivots in the workgroup's slot behind the
// left factor's part; (the last stage's copy, jpr) stand where (Wr, jpr) stand in T1.  An exactly zero row of right is a zero column of every
// stack: pivoted last, tau = 0.  n <= H is the tall complex call itself: the launcher runs its instances under brtc_plan, so the bits are that
// call's.  The slot: the left factor's part (stage copies for m > H, brcc_ws_elems' copy otherwise), the right factor's stage copies, then G and
// J wherever they are not in LDS.
__host__ __device__ inline size_t brlc_ws_elems(int m, int n, int K, int ldg, bool l_lds, bool r_lds, bool v_lds, bool g_lds) {
    if (n <= BRT_H) return brtc_ws_elems(m, n, K, ldg, l_lds, r_lds, v_lds, g_lds);
    return brtc_ws_elems(m, 0, K, ldg, l_lds, true, true, true) + (size_t)brt_stages(n, K) * brt_stage_elems(K) + (g_lds ? 0 : (size_t)K * ldg) +
           (v_lds ? 0 : (size_t)K * K);
}

// vt^T[:, c] = conj(ph_c) Q_0 [Q_1 [.. Q_{S-1} [Vc[:, srt[c]]; 0] ..; 0]; 0] for S >= 2 stages of the right factor, Vc the kept columns of G already
// conjugated and scaled: brtc_form_u with the phases already fixed on u, so every chunk is written once, multiplied by conj(phs[c]) with operator*
// of rc_cplx.hpp (the product bsc_form_u(phase_here = false) uses: conjugating the inputs conjugates the row bit for bit), and no row is visited
// twice.  V is vt's transposed view (n x k); rows r .. k - 1 of vt are zero over all n columns.
template <typename R>
__device__ __forceinline__ void brlc_form_vt(const cplx<R> *stage0, size_t se, int S, int K, int q, int n, const cplx<R> *Vc, int ldv, int k, int r, const int *srt,
                                             const cplx<R> *phs, cplx<R> *V, int64_t vrs, int64_t vcs, int wv, int lane) {
    constexpr int NE = BRT_H / 64;
    for (int c = wv; c < k; c += BID_WAVES) {
        cplx<R> *vc = V + (int64_t)c * vcs;
        if (c >= r) {
            for (int i = lane; i < n; i += 64) vc[i * vrs] = czero<R>();
            continue;
        }
        const cplx<R> *gc = Vc + (size_t)srt[c] * ldv;
        const cplx<R> ph = cj(phs[c]);
        cplx<R> x[NE];
#pragma unroll
        for (int e = 0; e < NE; ++e) {
            const int i = lane + 64 * e;
            x[e] = i < q ? gc[i] : czero<R>();
        }
        for (int s = S - 1; s >= 0; --s) {
            const cplx<R> *Ws = stage0 + (size_t)s * se, *ts = Ws + (size_t)BRT_H * K;
            const int top = s ? q : 0, base = s ? BRT_H + (s - 1) * (BRT_H - q) : 0;
            const int hs = top + min(BRT_H - top, n - base);
            bsc_reflect_back<R, NE>(Ws, BRT_H, hs, q, reinterpret_cast<const int *>(ts + K), ts, x, lane);
            if (s) {
#pragma unroll
                for (int e = 0; e < NE; ++e) {
                    const int i = lane + 64 * e;
                    if (i >= top && i < hs) vc[(int64_t)(base + i - top) * vrs] = x[e] * ph;
                    x[e] = i < top ? x[e] : czero<R>();
                }
            }
        }
#pragma unroll
        for (int e = 0; e < NE; ++e) vc[(int64_t)(lane + 64 * e) * vrs] = x[e] * ph;  // stage 0 of S >= 2 stages holds H rows
    }
}

// TALL = false: rc_lowrank_recompress_complex_batched_*, and rc_lowrank_recompress_tall_complex_batched_* for m <= 512.  TALL = true:
// rc_lowrank_recompress_tall_complex_batched_* for m > 512, the left factor by stages (see above; the plan keeps the stage copies out of LDS).
// Two waves per SIMD (256 registers), but for the c64 tall instance, which is built for one wave per SIMD.  It fits 256 registers without
// scratch, but the code the compiler makes under that bound is slower than what it makes with room to spare: 52.7k against 74.7k blocks/s at
// 2048 x 2048 x 256, K = 32, and 49.9k against 68.7k at 512 x 8192 x 128, K = 16, at the same grid: the workspace bound leaves
// one workgroup per CU at those shapes either way, and the kernel is latency-bound per Householder step.
// LARGE (with TALL): rc_lowrank_recompress_complex_large_batched_* for n > 512, the right factor by stages too (see "both factors tall"), the left
// one by stages for m > 512 and as one stage below.  The launcher sends n <= 512 to the two instances above, so this one carries neither the
// one-stage path of the right factor nor bsc_form_u for vt.  Both of its instances are built for one wave per SIMD: the c64 one for the reason
// above, and the c32 one because it carries both left paths and spills three registers under the bound of two waves (12 bytes of scratch per
// thread; none with room), while its slot (both factors' stages) leaves one workgroup per CU at the shapes it is for either way.
// With the operands' exponents and scales the c32 tall instance spills 12 bytes per lane under its bound of two waves (measured 1.02 of its
// former time at 1024 x 512, K = 64), and the c64 tall instance, without scratch, measures 1.4 - 1.5 of its former time: DESIGN.md 7r-2.
template <typename R, bool TALL, bool LARGE = false>
__global__ __launch_bounds__(BID_THREADS, ((TALL && sizeof(R) == 8) || LARGE) ? 1 : 2) void k_batched_recompress_c(BrcCArgs<R> a) {
    static_assert(TALL || !LARGE, "the large instance is the tall one with a staged right factor");
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const int m = (int)a.left.rows, n = (int)a.right.cols, K = (int)a.left.cols;
    const int kk = a.k < K ? a.k : K, ldg = a.ldg;
    const bool multi = LARGE ? m > BRT_H : TALL;  // the left factor by stages, its copies in the slot (a constant but in the large instance)
    const int ldl = multi ? BRT_H : a.l_lds ? (m | 1) : m, ldr = LARGE ? BRT_H : a.r_lds ? (n | 1) : n, ldj = a.v_lds ? ldg : K;
    cplx<R> *lp = reinterpret_cast<cplx<R> *>(smem_raw);  // next free LDS element
    cplx<R> *wp = a.ws + (size_t)blockIdx.x * (LARGE  ? brlc_ws_elems(m, n, K, ldg, a.l_lds, a.r_lds, a.v_lds, a.g_lds)
                                               : TALL ? brtc_ws_elems(m, n, K, ldg, a.l_lds, a.r_lds, a.v_lds, a.g_lds)
                                                      : brcc_ws_elems(m, n, K, ldg, a.l_lds, a.r_lds, a.v_lds, a.g_lds));  // next free workspace element
    cplx<R> *Wl0, *Wr0, *G, *J;
    if (a.l_lds) { Wl0 = lp; lp += (size_t)K * ldl; } else { Wl0 = wp; wp += multi ? (size_t)brt_stages(m, K) * brt_stage_elems(K) : (size_t)m * K; }
    if (a.r_lds) { Wr0 = lp; lp += (size_t)K * ldr; } else { Wr0 = wp; wp += LARGE ? (size_t)brt_stages(n, K) * brt_stage_elems(K) : (size_t)n * K; }
    if (a.g_lds) { G = lp; lp += (size_t)K * ldg; } else { G = wp; wp += (size_t)K * ldg; }
    if (a.v_lds) { J = lp; lp += (size_t)K * ldj; } else { J = wp; }
    cplx<R> *taul = lp, *taur = taul + K, *phs = taur + K;
    R *vn1 = reinterpret_cast<R *>(phs + 128);
    R *vn2 = vn1 + K, *sig = vn2 + K, *red = sig + K;
    int *jpl = reinterpret_cast<int *>(red + 8);
    int *jpr = jpl + K, *ipl = jpr + K, *ipr = ipl + K, *srt = ipr + K, *flag = srt + K;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;

    for (int b = blockIdx.x; b < a.count; b += gridDim.x) {
        int q = K;
        if (a.in_ranks) {
            const int64_t rv = a.in_ranks[b];
            q = rv < 0 ? 0 : rv > K ? K : (int)rv;
        }
        q = __builtin_amdgcn_readfirstlane(q);  // one value per block, uniform by construction
        R *sb = a.s_out + (int64_t)b * K;
        cplx<R> *Ub = a.u.p + (int64_t)b * a.ubs, *Vb = a.vt.p + (int64_t)b * a.vbs;
        for (int i = q + tid; i < K; i += BID_THREADS) sb[i] = (R)0;
        if (q == 0) {  // uniform over the workgroup; no input is read
            if (tid == 0) a.ranks[b] = 0;
            for (int c = wv; c < kk; c += BID_WAVES) {
                for (int i = lane; i < m; i += 64) Ub[i * a.u.rs + c * a.u.cs] = czero<R>();
                for (int i = lane; i < n; i += 64) Vb[c * a.vt.rs + i * a.vt.cs] = czero<R>();
            }
            continue;
        }
        // ---- the two pivoted QRs, q steps each (exact zero pivots are steps with H = I), taus and pivots kept -----------------------
        const cplx<R> *__restrict__ L = a.left.p + (int64_t)b * a.lbs;
        const cplx<R> *__restrict__ Rt = a.right.p + (int64_t)b * a.rbs;
        cplx<R> *Wl = Wl0;  // the copy the core and U read: the last stage's
        cplx<R> *Wr = Wr0;  // likewise for T1 (set per block: a workgroup's next block starts at stage 0 again)
        // the operands' exponents, as in k_batched_recompress (red[4..7] and red[0..3] in turn: bid_qrcp writes red only behind the loads'
        // barriers): every operand enters at unit scale and the singular values take 2^(el + em + es + er) back.  mid's and s's are taken
        // behind the two QRs, where they are first needed (red is free again behind the barrier there)
        const int el = brc_exponent(m, q, a.left.rs <= a.left.cs, [&](int i, int c) { return L[(int64_t)i * a.left.rs + c * a.left.cs]; }, red + 4, wv, lane);
        const int er = brc_exponent(n, q, a.right.cs <= a.right.rs, [&](int i, int c) { return Rt[c * a.right.rs + (int64_t)i * a.right.cs]; }, red, wv, lane);
        [[maybe_unused]] int S = 1;
        const R scl = ldexp((R)1, -el);  // each scale is made where it is used
        if (multi) {
            S = brt_stages(m, q);  // >= 2: m > BRT_H
            const size_t se = brt_stage_elems(K);
            for (int j = tid; j < q; j += BID_THREADS) jpl[j] = j;  // ordered before its first read by brt_stack_load's barrier
            for (int s = 0; s < S; ++s) {
                const int top = s ? q : 0, base = s ? BRT_H + (s - 1) * (BRT_H - q) : 0;
                const int hs = top + min(BRT_H - top, m - base);
                cplx<R> *Ws = Wl0 + (size_t)s * se, *ts = Ws + (size_t)BRT_H * K;
                brt_stack_load(Ws, ldl, Ws - (s ? se : 0), top, hs, q, a.left.rs <= a.left.cs,
                                [&](int i, int c) { return escale(L[(int64_t)(base + i) * a.left.rs + c * a.left.cs], scl); }, vn1, vn2, jpl, wv, lane);
                bid_qrcp<cplx<R>, true>(Ws, ldl, hs, q, q, 0.0, jpl, vn1, vn2, red, tid, wv, lane, ts);
                int *js = reinterpret_cast<int *>(ts + K);  // the stage's pivots beside its taus; jpl goes on as the next stage's starting order
                for (int j = tid; j < q; j += BID_THREADS) js[j] = jpl[j];
                Wl = Ws;
            }
        } else {
            bid_load(Wl, ldl, m, q, a.left.rs <= a.left.cs, [&](int i, int c) { return escale(L[i * a.left.rs + c * a.left.cs], scl); }, vn1, vn2, jpl, wv, lane);
            bid_qrcp<cplx<R>, true>(Wl, ldl, m, q, q, 0.0, jpl, vn1, vn2, red, tid, wv, lane, taul);
        }
        [[maybe_unused]] int Sr = 1;
        const R scr = ldexp((R)1, -er);
        if constexpr (LARGE) {  // the left factor's stage loop on right[:q, :]^T, every stage in the slot
            Sr = brt_stages(n, q);  // >= 2: n > BRT_H
            const size_t se = brt_stage_elems(K);
            for (int j = tid; j < q; j += BID_THREADS) jpr[j] = j;  // ordered before its first read by brt_stack_load's barrier
            for (int s = 0; s < Sr; ++s) {
                const int top = s ? q : 0, base = s ? BRT_H + (s - 1) * (BRT_H - q) : 0;
                const int hs = top + min(BRT_H - top, n - base);
                cplx<R> *Ws = Wr0 + (size_t)s * se, *ts = Ws + (size_t)BRT_H * K;
                brt_stack_load(Ws, ldr, Ws - (s ? se : 0), top, hs, q, a.right.cs <= a.right.rs,
                                [&](int i, int c) { return escale(Rt[c * a.right.rs + (int64_t)(base + i) * a.right.cs], scr); }, vn1, vn2, jpr, wv, lane);
                bid_qrcp<cplx<R>, true>(Ws, ldr, hs, q, q, 0.0, jpr, vn1, vn2, red, tid, wv, lane, ts);
                int *js = reinterpret_cast<int *>(ts + K);
                for (int j = tid; j < q; j += BID_THREADS) js[j] = jpr[j];
                Wr = Ws;
            }
        } else {
            bid_load(Wr, ldr, n, q, a.right.cs <= a.right.rs, [&](int i, int c) { return escale(Rt[c * a.right.rs + i * a.right.cs], scr); }, vn1, vn2, jpr, wv, lane);
            bid_qrcp<cplx<R>, true>(Wr, ldr, n, q, q, 0.0, jpr, vn1, vn2, red, tid, wv, lane, taur);
        }
        for (int j = tid; j < q; j += BID_THREADS) { ipl[jpl[j]] = j; ipr[jpr[j]] = j; }
        if constexpr (LARGE) {
            if (tid == 0) { flag[2] = 0; flag[3] = 0; }
        }
        __syncthreads();
        if constexpr (LARGE) {  // the nonzero rows of R_L and of R_R (exact zero pivots come last and leave a zero diagonal): see the core below
            for (int j = tid; j < q; j += BID_THREADS) {
                const cplx<R> dl = Wl[(size_t)jpl[j] * ldl + j], dr = Wr[(size_t)jpr[j] * ldr + j];
                if (!(dl.re == (R)0 && dl.im == (R)0)) atomicAdd(&flag[2], 1);
                if (!(dr.re == (R)0 && dr.im == (R)0)) atomicAdd(&flag[3], 1);
            }
        }
        // ---- T1 = mid diag(s) Rr^T in J's place ----------------------------------------------------------------------------------------
        const cplx<R> *__restrict__ Mb = a.mid.p ? a.mid.p + (int64_t)b * a.mbs : nullptr;
        const R *__restrict__ Sb = a.s ? a.s + (int64_t)b * a.s_stride : nullptr;
        const int em = Mb ? brc_exponent(q, q, a.mid.rs <= a.mid.cs, [&](int i, int c) { return Mb[(int64_t)i * a.mid.rs + c * a.mid.cs]; }, red + 4, wv, lane) : 0;
        const int es = Sb ? brc_exponent(q, 1, true, [&](int i, int) { return Sb[i]; }, red, wv, lane) : 0;
        const R scm = ldexp((R)1, -em), scs = ldexp((R)1, -es);
        for (int idx = tid; idx < q * q; idx += BID_THREADS) {
            const int ai = idx / q, j = idx - ai * q;
            cplx<R> acc;
            if (Mb) {
                acc = czero<R>();
                const cplx<R> *mr = Mb + (int64_t)ai * a.mid.rs;
                for (int bb = 0; bb < q; ++bb) {
                    const cplx<R> rv = j <= ipr[bb] ? Wr[(size_t)bb * ldr + j] : czero<R>();
                    cplx<R> mv = escale(mr[(int64_t)bb * a.mid.cs], scm);
                    if (Sb) { const R sv = Sb[bb] * scs; mv = cplx<R>{mv.re * sv, mv.im * sv}; }
                    cfma(mv, rv, acc);
                }
            } else {
                const cplx<R> rv = j <= ipr[ai] ? Wr[(size_t)ai * ldr + j] : czero<R>();
                acc = rv;
                if (Sb) { const R sv = Sb[ai] * scs; acc = cplx<R>{sv * rv.re, sv * rv.im}; }
            }
            J[(size_t)ai * ldj + j] = acc;
        }
        __syncthreads();
        // ---- G = C^H: G[i * ldg + j] = conj(sum_a Rl[i, a] T1[a, j]) ------------------------------------------------------------------
        // The large instance turns the core when right has fewer nonzero rows of R than left (exactly zero rows of right[:q, :] under
        // nonzero columns of left): G = C^H would then hold q columns in fewer dimensions, dependent columns, on which the iteration is
        // inaccurate.  It runs on G = C instead: the zero rows of R_R are zero columns of C, which no rotation touches, so they are
        // exactly zero singular values as zero columns of left are, and the remaining columns are as many as R_R has rows.  With
        // C J = U_c Sigma: U = Q_L [U_c; 0] from the scaled columns of G, vt^T = Q_R [conj(J); 0]: the two operands change places below.
        [[maybe_unused]] bool turned = false;  // a constant in every instance but the large one
        if constexpr (LARGE) turned = flag[3] < flag[2];  // uniform: read behind the barrier above, rewritten behind the block's last one
        for (int idx = tid; idx < q * q; idx += BID_THREADS) {
            const int i = idx / q, j = idx - i * q;
            cplx<R> acc = czero<R>();
            for (int aa = 0; aa < q; ++aa) {
                const cplx<R> lv = i <= ipl[aa] ? Wl[(size_t)aa * ldl + i] : czero<R>();
                cfma(lv, J[(size_t)aa * ldj + j], acc);
            }
            if constexpr (LARGE) {
                if (turned) G[(size_t)j * ldg + i] = acc;
                else G[(size_t)i * ldg + j] = cj(acc);
            } else {
                G[(size_t)i * ldg + j] = cj(acc);
            }
        }
        __syncthreads();
        for (int idx = tid; idx < q * q; idx += BID_THREADS) {
            const int j = idx / q, i = idx - j * q;
            J[(size_t)j * ldj + i] = i == j ? cone<R>() : czero<R>();
        }
        __syncthreads();
        bool conv;
        if (q <= 16) conv = bsv_jacobi<cplx<R>, 1>(G, ldg, J, ldj, q, tid, flag);
        else if (q <= 32) conv = bsv_jacobi<cplx<R>, 2>(G, ldg, J, ldj, q, tid, flag);
        else if (q <= 64) conv = bsv_jacobi<cplx<R>, 4>(G, ldg, J, ldj, q, tid, flag);
        else conv = bsv_jacobi<cplx<R>, 8>(G, ldg, J, ldj, q, tid, flag);
        if (!conv && tid == 0) atomicOr(a.health, 16);  // the sweep budget ran out: bit 16, as the batched SVD reports it
        // ---- singular values: column norms, sorted descending (a strict total order: NaN last, ties by column) ----------------------
        for (int j = tid >> 4; j < q; j += BID_THREADS / 16) {
            const cplx<R> *gj = G + (size_t)j * ldg;
            R acc = 0;
            for (int i = tid & 15; i < q; i += 16) {
                acc = fma(gj[i].re, gj[i].re, acc);
                acc = fma(gj[i].im, gj[i].im, acc);
            }
            acc = group_sum_dpp<16>(acc);
            if ((tid & 15) == 0) sig[j] = sqrt(acc);
        }
        __syncthreads();
        for (int i = tid; i < q; i += BID_THREADS) {
            const R ki = sig[i] >= (R)0 ? sig[i] : (R)-1;
            int pos = 0;
            for (int j = 0; j < q; ++j) {
                const R kj = sig[j] >= (R)0 ? sig[j] : (R)-1;
                pos += (kj > ki || (kj == ki && j < i)) ? 1 : 0;
            }
            srt[pos] = i;
            sb[pos] = ldexp(sig[i], el + er + em + es);  // the operands entered as 2^-el left, 2^-em mid, 2^-es s and 2^-er right
        }
        __syncthreads();
        // ---- rank: the first j < min(kk, q) with s_j == 0 or (tol > 0 and s_j / s_0 < tol), else min(kk, q) -------------------------
        if (tid == 0) {
            const R s0 = sig[srt[0]];
            const int kq = kk < q ? kk : q;
            int r = kq;
            for (int j = 0; j < kq; ++j) {
                const R sj = sig[srt[j]];
                if (sj == (R)0 || (a.tol > 0.0 && (double)(sj / s0) < a.tol)) { r = j; break; }
            }
            flag[1] = r;
            a.ranks[b] = r;
        }
        __syncthreads();
        const int r = flag[1];
        // ---- U = Q_L [J_r; 0] with the phase rule applied to its columns, the phases kept in phs ------------------------------------------
        if constexpr (LARGE) {
            const cplx<R> *Uc = J;  // the core's left vectors
            int ldc = ldj;
            if (turned) {  // U_c = G Sigma^-1 and conj(J) in place (kept columns), before either is read
                for (int c = wv; c < r; c += BID_WAVES) {
                    cplx<R> *gc = G + (size_t)srt[c] * ldg, *jc = J + (size_t)srt[c] * ldj;
                    const R sj = sig[srt[c]], inv = sj > (R)0 ? (R)1 / sj : (R)0;
                    for (int i = lane; i < q; i += 64) {
                        const cplx<R> g = gc[i];
                        gc[i] = cplx<R>{g.re * inv, g.im * inv};
                        jc[i] = cj(jc[i]);
                    }
                }
                __syncthreads();
                Uc = G;
                ldc = ldg;
            }
            if (multi) brtc_form_u<R>(Wl0, brt_stage_elems(K), S, K, q, m, Uc, ldc, kk, r, srt, phs, Ub, a.u.rs, a.u.cs, wv, lane);
            else if (m <= 64) bsc_form_u<R, 1>(Wl, ldl, Uc, ldc, m, q, kk, r, jpl, taul, srt, phs, true, Ub, a.u.rs, a.u.cs, wv, lane);
            else if (m <= 128) bsc_form_u<R, 2>(Wl, ldl, Uc, ldc, m, q, kk, r, jpl, taul, srt, phs, true, Ub, a.u.rs, a.u.cs, wv, lane);
            else if (m <= 256) bsc_form_u<R, 4>(Wl, ldl, Uc, ldc, m, q, kk, r, jpl, taul, srt, phs, true, Ub, a.u.rs, a.u.cs, wv, lane);
            else bsc_form_u<R, 8>(Wl, ldl, Uc, ldc, m, q, kk, r, jpl, taul, srt, phs, true, Ub, a.u.rs, a.u.cs, wv, lane);
        } else {
            if (multi) brtc_form_u<R>(Wl0, brt_stage_elems(K), S, K, q, m, J, ldj, kk, r, srt, phs, Ub, a.u.rs, a.u.cs, wv, lane);
            else if (m <= 64) bsc_form_u<R, 1>(Wl, ldl, J, ldj, m, q, kk, r, jpl, taul, srt, phs, true, Ub, a.u.rs, a.u.cs, wv, lane);
            else if (m <= 128) bsc_form_u<R, 2>(Wl, ldl, J, ldj, m, q, kk, r, jpl, taul, srt, phs, true, Ub, a.u.rs, a.u.cs, wv, lane);
            else if (m <= 256) bsc_form_u<R, 4>(Wl, ldl, J, ldj, m, q, kk, r, jpl, taul, srt, phs, true, Ub, a.u.rs, a.u.cs, wv, lane);
            else bsc_form_u<R, 8>(Wl, ldl, J, ldj, m, q, kk, r, jpl, taul, srt, phs, true, Ub, a.u.rs, a.u.cs, wv, lane);
        }
        // ---- conj(V_c) = conj(G Sigma^-1) in place (kept columns), then vt^T = Q_R [conj(V_c); 0] conj(ph) through vt's transposed view ---
        if (!turned) {  // (false in every instance but the large one)
            for (int c = wv; c < r; c += BID_WAVES) {
                cplx<R> *gc = G + (size_t)srt[c] * ldg;
                const R sj = sig[srt[c]], inv = sj > (R)0 ? (R)1 / sj : (R)0;
                for (int i = lane; i < q; i += 64) {
                    const cplx<R> g = gc[i];
                    gc[i] = cplx<R>{g.re * inv, -(g.im * inv)};
                }
            }
        }
        __syncthreads();  // phs and the scaled columns are read by other waves below
        if constexpr (LARGE) brlc_form_vt<R>(Wr0, brt_stage_elems(K), Sr, K, q, n, turned ? J : G, turned ? ldj : ldg, kk, r, srt, phs, Vb, a.vt.cs, a.vt.rs, wv, lane);
        else if (n <= 64) bsc_form_u<R, 1>(Wr, ldr, G, ldg, n, q, kk, r, jpr, taur, srt, phs, false, Vb, a.vt.cs, a.vt.rs, wv, lane);
        else if (n <= 128) bsc_form_u<R, 2>(Wr, ldr, G, ldg, n, q, kk, r, jpr, taur, srt, phs, false, Vb, a.vt.cs, a.vt.rs, wv, lane);
        else if (n <= 256) bsc_form_u<R, 4>(Wr, ldr, G, ldg, n, q, kk, r, jpr, taur, srt, phs, false, Vb, a.vt.cs, a.vt.rs, wv, lane);
        else bsc_form_u<R, 8>(Wr, ldr, G, ldg, n, q, kk, r, jpr, taur, srt, phs, false, Vb, a.vt.cs, a.vt.rs, wv, lane);
        __syncthreads();  // the working copies, G, J and the small arrays are rewritten by the next block
    }
}

// ---- batched sketched column ID of complex tall blocks (rc_sketch_column_id_rank_complex_batched_c64 / _c32) --------------------
// k_batched_sketch_id's structure (kernels_batched_id.hip) with the stages above: per block the sketch Y = Omega A (l x n, l <= 128, nothing
// conjugated) is formed straight into the complex working copy W, then bid_norms, bid_qrcp and bid_z run on W with l rows: the same
// routines on the same values as k_batched_id<cplx<R>> given Y, hence its pivots, rank and Z bit for bit; C is gathered from A.
//
// The sketch.  Column panels of BSI_COLS = 64 columns of Y, one 16-column MFMA tile per wave, up to BSC_TILES = 4 of the ceil(l / 16) row
// tiles of the panel in the wave's accumulators, Re and Im apart (v_mfma_f64_16x16x4_f64 / v_mfma_f32_16x16x4_f32, Acc<R> of rc_gemm.hpp, the
// real and imaginary parts as separate real operands); l > 64 takes a second pass over the panels for row tiles 4 .. 7.  The panel's rows of A stream through LDS in chunks of BSI_ROWS = 32 rows beside the matching 32
// columns of Omega.  The images are separate re / im planes, each with the layout and pitches of the real kernel's image (rc_gemm.hpp):
// a fragment read is then a read of R from one plane, exactly the real kernel's access (pitch 34 along the reduction index, or a pitch of
// 16 modulo 32 along the other: free of bank conflicts), which interleaved elements would turn into reads at twice the stride; the
// staging stores pay for it with two stores of R per element.  Zeros fill past m, n and l, so the MFMA loop has no edge branch.
// Per element each of Re Y and Im Y is one accumulator chain from zero over the ascending rows of A, four rows per instruction, and
// within a step (the order of kernels_batched_residual_c.hip)
//     Re takes MFMA(Om_re, A_re) then MFMA(-Om_im, A_im);   Im takes MFMA(Om_re, A_im) then MFMA(Om_im, A_re)
// (the negation is a sign flip in a register: exact): a function of (l, m, n) and the two constants alone.  Conjugating a and omega
// negates the second product of Re's pair twice and every product of Im's chain once, and the MFMAs round a sum and its negation to
// opposite values, so Y comes out conjugated bit for bit (an Im cancelled to zero is +0 either way) and the stages above commute with
// it; with +0 imaginary parts Re's chain gains only zeros and carries the real kernel's values, and Im Y is zero.
//
// Registers: two waves per SIMD (256 registers), which is what the pivoted QR after the sketch needs: it is a chain of short dependent steps,
// and with one workgroup per CU nothing hides their latency (measured: 1.4 to 1.6 times the blocks per second of the one-wave variant that
// kept all eight row tiles).  Four row tiles are 2 x 4 x 8 accumulator registers in c64 and 8 + 8 staged complex elements
// (64 registers); a is read a second time when l > 64, Omega's image holds the 64 rows of one pass.  The chunk loop has no scratch access.

// dynamic LDS: [W: n x (l|1) complex, LDS plan only] tile[8 x 9] complex | A chunk re, im [BSI_A_ELEMS each] Omega chunk re, im
// [bsc_o_elems(l) each] vn1[n] vn2[n] red[8] real | jp[n]
constexpr int BSC_TILES = 4;  // row tiles of Y in a wave's accumulators at a time: l > 64 takes a second pass over the panel
__host__ __device__ constexpr int bsc_o_elems(int l) { return bsi_o_elems(l < 16 * BSC_TILES ? l : 16 * BSC_TILES); }  // one plane of Omega's image
template <typename R>
size_t bsc_lds_bytes(int l, int n, bool in_lds) {
    size_t c = (size_t)BIC_NB * (BIC_NB + 1);
    if (in_lds) c += (size_t)n * (size_t)(l | 1);
    return c * sizeof(cplx<R>) + ((size_t)2 * BSI_A_ELEMS + (size_t)2 * bsc_o_elems(l) + (size_t)2 * n + 8) * sizeof(R) + (size_t)n * sizeof(int);
}

template <typename R>
struct BscArgs {
    CV<R> a, omega, y, c, z;  // y.p == nullptr: the sketch is not written
    int64_t abs, obs, ybs, cbs, zbs;
    int64_t *col_ind, *ranks;
    cplx<R> *ws;
    double tol;
    int count, kk;
    bool w_lds;  // the working copy in LDS (else in the workgroup's workspace slot)
};

// W[c * ldw + i] = Y[i, c] = sum_r Om[i, r] A[r, c] for the TL row tiles of 16 rows from tile t0 on of the l x n sketch of one block (and Y to
// Yb when it is not null).
// AR / OR: the lanes of the staging loads run along the rows of a / of omega (the operand's smaller stride), else along its columns;
// each thread's elements of a chunk are then a fixed step apart in memory and in the LDS planes, whose offsets are compile-time constants.
// WM: where the sketch goes besides Yb.  BSC_W_COLS: W[c * ldw + i] as above; BSC_W_ROWS: W[i * ldw + c], the working copy of Y^T
// (k_batched_range_step_c's row basis); BSC_W_NONE: W is not written (its projection, whose l x m "sketch" only goes to Yb).
// yconj: Yb receives the conjugate, the sign of the imaginary part flipped at the store (that projection's p_conj); W never does.
enum { BSC_W_COLS = 0, BSC_W_ROWS = 1, BSC_W_NONE = 2 };
template <typename R, int TL, bool AR, bool OR, int WM = BSC_W_COLS>
__device__ __forceinline__ void bsc_sketch(const BscArgs<R> &g, const cplx<R> *__restrict__ A, const cplx<R> *__restrict__ Om, cplx<R> *Yb, cplx<R> *W, int ldw, R *As,
                                           R *Os, int oplane, int t0, int tid, int wv, int lane, bool yconj = false) {
    constexpr int PO = bsi_po(16 * TL);
    constexpr int A_PER = BSI_ROWS * BSI_COLS / BID_THREADS;    // 8 elements of A per thread and chunk
    constexpr int O_PER = BSI_ROWS * 16 * TL / BID_THREADS;     // 2 TL elements of Omega
    constexpr int A_SR = AR ? 1 : BSI_PA, A_SC = AR ? BSI_PK : 1;   // A's planes: As[r * A_SR + c * A_SC] (re), + BSI_A_ELEMS (im)
    constexpr int O_SI = OR ? 1 : BSI_PK, O_SR = OR ? PO : 1;       // Omega's planes: Os[i * O_SI + r * O_SR] (re), + oplane (im)
    const int m = (int)g.a.rows, n = (int)g.a.cols, ltot = (int)g.omega.rows;
    const int l = ltot - 16 * t0 < 16 * TL ? ltot - 16 * t0 : 16 * TL;  // rows of Omega in this pass, from row 16 t0
    const int64_t ars = g.a.rs, acs = g.a.cs, ors = g.omega.rs, ocs = g.omega.cs;
    Om += (int64_t)(16 * t0) * ors;
    // this thread's elements of a chunk: A[ar + AR_STEP e, ac + AC_STEP e], Om[oi + 16 (e / 2) or 8 e, orr + 16 (e % 2) or 0]
    const int ar = AR ? (tid & (BSI_ROWS - 1)) : (tid / BSI_COLS), ac = AR ? (tid / BSI_ROWS) : (tid & (BSI_COLS - 1));
    constexpr int AR_STEP = AR ? 0 : BID_THREADS / BSI_COLS, AC_STEP = AR ? BID_THREADS / BSI_ROWS : 0;
    const int oi = OR ? (tid & 15) : (tid / BSI_ROWS), orr = OR ? (tid >> 4) : (tid & (BSI_ROWS - 1));
    const int r16 = lane & 15, k4 = lane >> 4;
    R *as_st = As + ar * A_SR + ac * A_SC, *os_st = Os + oi * O_SI + orr * O_SR;
    const R *as_ld = As + k4 * A_SR + (wv * 16 + r16) * A_SC, *os_ld = Os + r16 * O_SI + k4 * O_SR;
    for (int c0 = 0; c0 < n; c0 += BSI_COLS) {
        typename Acc<R>::type are[TL], aim[TL];
#pragma unroll
        for (int i = 0; i < TL; ++i) { are[i] = typename Acc<R>::type{0, 0, 0, 0}; aim[i] = typename Acc<R>::type{0, 0, 0, 0}; }
        // the chunk at rows m0 .. m0 + 31 into this thread's staging registers
        cplx<R> av[A_PER], ov[O_PER];
        auto fetch = [&](int m0) {
            const cplx<R> *pa = A + (int64_t)(m0 + ar) * ars + (int64_t)(c0 + ac) * acs;
            const cplx<R> *po = Om + (int64_t)oi * ors + (int64_t)(m0 + orr) * ocs;
            // the steps between a thread's elements are uniform; hidden from the optimizer here, every address is the thread's one base plus a
            // scalar offset (otherwise each of the 8 + 2 TL addresses becomes a loop-carried 64-bit register pair of its own)
            int64_t sa = AR ? AC_STEP * acs : AR_STEP * ars, so_i = ors, so_r = ocs;
            asm volatile("" : "+s"(sa), "+s"(so_i), "+s"(so_r));
#pragma unroll
            for (int e = 0; e < A_PER; ++e) {
                const bool ok = m0 + ar + AR_STEP * e < m && c0 + ac + AC_STEP * e < n;
                av[e] = ok ? pa[e * sa] : czero<R>();
            }
#pragma unroll
            for (int e = 0; e < O_PER; ++e) {
                const int di = OR ? 16 * (e / 2) : 8 * e, dr = OR ? 16 * (e % 2) : 0;
                const bool ok = oi + di < l && m0 + orr + dr < m;
                ov[e] = ok ? po[di * so_i + dr * so_r] : czero<R>();
            }
        };
        for (int m0 = 0; m0 < m; m0 += BSI_ROWS) {
            fetch(m0);
#pragma unroll
            for (int e = 0; e < A_PER; ++e) {
                as_st[AR_STEP * e * A_SR + AC_STEP * e * A_SC] = av[e].re;
                as_st[AR_STEP * e * A_SR + AC_STEP * e * A_SC + BSI_A_ELEMS] = av[e].im;
            }
#pragma unroll
            for (int e = 0; e < O_PER; ++e) {
                const int di = OR ? 16 * (e / 2) : 8 * e, dr = OR ? 16 * (e % 2) : 0;
                os_st[di * O_SI + dr * O_SR] = ov[e].re;
                os_st[di * O_SI + dr * O_SR + oplane] = ov[e].im;
            }
            __syncthreads();
#pragma unroll
            for (int ks = 0; ks < BSI_ROWS / 4; ++ks) {
                const R bre = as_ld[ks * 4 * A_SR], bim = as_ld[ks * 4 * A_SR + BSI_A_ELEMS];
#pragma unroll
                for (int i = 0; i < TL; ++i) {
                    const R ore = os_ld[i * 16 * O_SI + ks * 4 * O_SR], oim = os_ld[i * 16 * O_SI + ks * 4 * O_SR + oplane];
                    are[i] = Acc<R>::mfma(ore, bre, are[i]);
                    are[i] = Acc<R>::mfma(-oim, bim, are[i]);
                    aim[i] = Acc<R>::mfma(ore, bim, aim[i]);
                    aim[i] = Acc<R>::mfma(oim, bre, aim[i]);
                }
            }
            __syncthreads();  // the chunk images are rewritten by the next chunk
        }
        const int col = c0 + wv * 16 + r16;
#pragma unroll
        for (int i = 0; i < TL; ++i)
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int row = (t0 + i) * 16 + Acc<R>::row(lane, reg);
                if (row < ltot && col < n) {
                    const cplx<R> v{are[i][reg], aim[i][reg]};
                    if constexpr (WM == BSC_W_COLS) W[(size_t)col * ldw + row] = v;
                    if constexpr (WM == BSC_W_ROWS) W[(size_t)row * ldw + col] = v;
                    if (Yb) Yb[row * g.y.rs + col * g.y.cs] = yconj ? cj(v) : v;
                }
            }
    }
    __syncthreads();
}

template <typename R, bool AR, bool OR>
__global__ __launch_bounds__(BID_THREADS, 2) void k_batched_sketch_id_c(BscArgs<R> g) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const int m = (int)g.a.rows, n = (int)g.a.cols, l = (int)g.omega.rows, kk = g.kk;
    const int ldw = g.w_lds ? (l | 1) : l;
    const int oplane = bsc_o_elems(l);
    cplx<R> *lds = reinterpret_cast<cplx<R> *>(smem_raw);
    cplx<R> *W = g.w_lds ? lds : g.ws + (size_t)blockIdx.x * (size_t)l * (size_t)n;
    cplx<R>(*tile)[BIC_NB + 1] = reinterpret_cast<cplx<R>(*)[BIC_NB + 1]>(lds + (g.w_lds ? (size_t)n * ldw : 0));
    R *As = reinterpret_cast<R *>(lds + (g.w_lds ? (size_t)n * ldw : 0) + BIC_NB * (BIC_NB + 1));
    R *Os = As + 2 * BSI_A_ELEMS;
    R *vn1 = Os + 2 * oplane;
    R *vn2 = vn1 + n;
    R *red = vn2 + n;
    int *jp = reinterpret_cast<int *>(red + 8);
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;

    for (int b = blockIdx.x; b < g.count; b += gridDim.x) {
        const cplx<R> *__restrict__ A = g.a.p + (int64_t)b * g.abs;
        const cplx<R> *__restrict__ Om = g.omega.p + (int64_t)b * g.obs;
        cplx<R> *Yb = g.y.p ? g.y.p + (int64_t)b * g.ybs : nullptr;
        // ---- the sketch into W (and y), at most BSC_TILES row tiles per pass over the panels, one instance per number of 16-row tiles of a pass ----
        for (int t0 = 0; 16 * t0 < l; t0 += BSC_TILES) {
            const int rest = ((l + 15) >> 4) - t0;
            switch (rest < BSC_TILES ? rest : BSC_TILES) {
                case 1: bsc_sketch<R, 1, AR, OR>(g, A, Om, Yb, W, ldw, As, Os, oplane, t0, tid, wv, lane); break;
                case 2: bsc_sketch<R, 2, AR, OR>(g, A, Om, Yb, W, ldw, As, Os, oplane, t0, tid, wv, lane); break;
                case 3: bsc_sketch<R, 3, AR, OR>(g, A, Om, Yb, W, ldw, As, Os, oplane, t0, tid, wv, lane); break;
                default: bsc_sketch<R, 4, AR, OR>(g, A, Om, Yb, W, ldw, As, Os, oplane, t0, tid, wv, lane); break;
            }
        }
        // ---- the column ID of Y: k_batched_id's stages on l rows --------------------------------------------------------------------
        bid_norms_pow2(W, ldw, l, n, vn1, vn2, jp, red + 4, wv, lane);
        const int r = bid_qrcp(W, ldw, l, n, kk, g.tol, jp, vn1, vn2, red, tid, wv, lane);
        for (int p = tid; p < n; p += BID_THREADS) g.col_ind[(int64_t)b * n + p] = jp[p];
        if (tid == 0) g.ranks[b] = r;
        // C[:, j] = A[:, jp[j]] (zero for j >= r), the lanes along a's smaller stride
        cplx<R> *Cb = g.c.p + (int64_t)b * g.cbs;
        if (g.a.rs <= g.a.cs) {
            for (int j = wv; j < kk; j += BID_WAVES) {
                const cplx<R> *src = A + (int64_t)jp[j] * g.a.cs;
                for (int i = lane; i < m; i += 64) Cb[i * g.c.rs + j * g.c.cs] = j < r ? src[i * g.a.rs] : czero<R>();
            }
        } else {
            const int total = m * kk;  // <= 65536 * 128
            for (int idx = tid; idx < total; idx += BID_THREADS) {
                const int i = idx / kk, j = idx - i * kk;
                Cb[i * g.c.rs + j * g.c.cs] = j < r ? A[i * g.a.rs + (int64_t)jp[j] * g.a.cs] : czero<R>();
            }
        }
        bid_z(W, ldw, n, r, kk, jp, tile, g.z.p + (int64_t)b * g.zbs, g.z.rs, g.z.cs, tid);
        __syncthreads();  // W, jp and the norms are rewritten by the next block
    }
}

// ---- batched range step of complex tall blocks (rc_sketch_range_step_complex_batched_c64 / _c32) -------------------------------------------
// k_batched_range_step's structure (kernels_batched_id.hip) with the stages above.  Per block: the sketch Y = Omega A (nothing conjugated)
// by bsc_sketch, k_batched_sketch_id_c's instances and passes, stored as the working copy of the plain transpose Y^T (n x l, column i =
// row i of Y); bid_norms_pow2 and the pivoted complex Householder QR of Y^T by bid_qrcp<cplx<R>, true> run to all l steps with the taus kept;
// the rank r, the first step whose real R_jj is exactly zero or not finite; Q (l x n), row c = (H_0 .. H_c e_c)^T for c < r (transposed,
// not conjugated: Q Q^H = I, and the QR of Y^H would give the same rows) and exactly zero from r on, written to q and, conjugated and n
// fastest, to the workgroup's slot; then the projection P^T = conj(Q) A^T, which is bsc_sketch once more on the transposed view of A with
// the slot's conj(Q) as the test matrix (the lanes of its staging loads along n) and P^T's only destination the transposed view of p.
// So an element of P = A Q^H is one accumulator chain pair (Re, Im) from zero over ascending column index of A, four columns per
// instruction in bsc_sketch's order, a zero row of Q is a zero column of P, and p_conj flips the sign of Im P at the store and nowhere else.
// A streams from HBM twice when l <= 64; above that each of the two products takes a second pass over A for row tiles 4 .. 7, as the
// sketched ID's does.  conj(Q) is re-read per 64-row panel of A from L2, as Omega is per column panel in the sketch.
// Conjugating a and omega conjugates Y (above), hence W, Q and the slot bit for bit, and P by the sketch's argument again; with +0
// imaginary parts every imaginary part below stays zero.
// dynamic LDS: [W: l x (n|1) complex, LDS plan only] taus[l] complex | A chunk re, im [BSI_A_ELEMS each] Omega chunk re, im
// [bsc_o_elems(l) each] vn1[l] vn2[l] red[8] real | jp[l] rk[4]
// slot: conj(Q) [l x n] [W: l x n, workspace plan only]
template <typename R>
size_t brsc_lds_bytes(int l, int n, bool in_lds) {
    size_t c = (size_t)l;
    if (in_lds) c += (size_t)l * (size_t)(n | 1);
    return c * sizeof(cplx<R>) + ((size_t)2 * BSI_A_ELEMS + (size_t)2 * bsc_o_elems(l) + (size_t)2 * l + 8) * sizeof(R) + (size_t)(l + 4) * sizeof(int);
}

template <typename R>
struct BrscArgs {
    CV<R> a, omega, y, q, p;  // y.p == nullptr: the sketch is not written
    int64_t abs, obs, ybs, qbs, pbs;
    int64_t *ranks;
    cplx<R> *ws;
    size_t slot;  // complex elements of one workgroup's slot
    int count;
    bool w_lds;   // the working copy of Y^T in LDS (else behind conj(Q) in the slot)
    bool p_conj;  // p receives conj(a q^H)
};

// Q[c, :] = (H_0 .. H_c e_c)^T for c < r, zero for r <= c < l, to Qb[c * qrs + i * qcs] and, conjugated, to Qs[c * n + i]: one wave per row
// of Q, its n entries in registers (entry lane + 64 e), the reflectors by bsc_reflect_back (v_j in W's column jp[j] below row j)
template <typename R, int NE>
__device__ __forceinline__ void brsc_form_q(const cplx<R> *W, int ldw, int n, int l, int r, const int *jp, const cplx<R> *taus, cplx<R> *Qs, cplx<R> *Qb, int64_t qrs,
                                            int64_t qcs, int wv, int lane) {
    for (int c = wv; c < l; c += BID_WAVES) {
        cplx<R> x[NE];
#pragma unroll
        for (int e = 0; e < NE; ++e) x[e] = (c < r && lane + 64 * e == c) ? cone<R>() : czero<R>();
        if (c < r) bsc_reflect_back<R, NE>(W, ldw, n, c + 1, jp, taus, x, lane);
#pragma unroll
        for (int e = 0; e < NE; ++e) {
            const int i = lane + 64 * e;
            if (i < n) {
                Qs[(size_t)c * n + i] = cj(x[e]);
                Qb[c * qrs + i * qcs] = x[e];
            }
        }
    }
}

// bsc_sketch's passes of at most BSC_TILES row tiles over the l rows of the test matrix, one instance per number of 16-row tiles of a pass
#define RC_BSC_PASSES(AR_, OR_, WM_, G_, A_, OM_, YB_, W_, LDW_, T_, YC_)                                                                   \
    for (int t0 = 0; 16 * t0 < l; t0 += BSC_TILES) {                                                                                        \
        const int rest = ((l + 15) >> 4) - t0;                                                                                              \
        switch (rest < BSC_TILES ? rest : BSC_TILES) {                                                                                      \
            case 1: bsc_sketch<R, 1, AR_, OR_, WM_>(G_, A_, OM_, YB_, W_, LDW_, As, Os, oplane, t0, T_, T_ >> 6, T_ & 63, YC_); break;      \
            case 2: bsc_sketch<R, 2, AR_, OR_, WM_>(G_, A_, OM_, YB_, W_, LDW_, As, Os, oplane, t0, T_, T_ >> 6, T_ & 63, YC_); break;      \
            case 3: bsc_sketch<R, 3, AR_, OR_, WM_>(G_, A_, OM_, YB_, W_, LDW_, As, Os, oplane, t0, T_, T_ >> 6, T_ & 63, YC_); break;      \
            default: bsc_sketch<R, 4, AR_, OR_, WM_>(G_, A_, OM_, YB_, W_, LDW_, As, Os, oplane, t0, T_, T_ >> 6, T_ & 63, YC_); break;     \
        }                                                                                                                                   \
    }

template <typename R, bool AR, bool OR>
__global__ __launch_bounds__(BID_THREADS, 2) void k_batched_range_step_c(BrscArgs<R> g) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const int m = (int)g.a.rows, n = (int)g.a.cols, l = (int)g.omega.rows;
    const int ldw = g.w_lds ? (n | 1) : n;
    const int oplane = bsc_o_elems(l);
    cplx<R> *lds = reinterpret_cast<cplx<R> *>(smem_raw);
    cplx<R> *Qs = g.ws + (size_t)blockIdx.x * g.slot;
    cplx<R> *W = g.w_lds ? lds : Qs + (size_t)l * (size_t)n;
    cplx<R> *taus = lds + (g.w_lds ? (size_t)l * ldw : 0);
    R *As = reinterpret_cast<R *>(taus + l);
    R *Os = As + 2 * BSI_A_ELEMS;
    R *vn1 = Os + 2 * oplane;
    R *vn2 = vn1 + l;
    R *red = vn2 + l;
    int *jp = reinterpret_cast<int *>(red + 8);
    int *rk = jp + l;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;

    for (int b = blockIdx.x; b < g.count; b += gridDim.x) {
        const cplx<R> *__restrict__ A = g.a.p + (int64_t)b * g.abs;
        const cplx<R> *__restrict__ Om = g.omega.p + (int64_t)b * g.obs;
        cplx<R> *Yb = g.y.p ? g.y.p + (int64_t)b * g.ybs : nullptr;
        // ---- the sketch, k_batched_sketch_id_c's, into the working copy of Y^T (and y) -----------------------------------------------------
        {
            BscArgs<R> s;
            s.a = g.a; s.omega = g.omega; s.y = g.y;
            // the thread index behind an empty asm: the sketch's per-thread staging offsets (8 instances of them with the projection's) are then
            // recomputed per block instead of being hoisted out of the block loop and spilled there
            int t = tid;
            asm volatile("" : "+v"(t));
            RC_BSC_PASSES(AR, OR, BSC_W_ROWS, s, A, Om, Yb, W, ldw, t, false)
        }
        // ---- the row basis: Y^T P = Q R to all l steps, the rank from R's real diagonal, Q formed from the first r reflectors ---------------
        bid_norms_pow2(W, ldw, n, l, vn1, vn2, jp, red + 4, wv, lane);
        if (tid == 0) *rk = l;
        bid_qrcp<cplx<R>, true>(W, ldw, n, l, l, 0.0, jp, vn1, vn2, red, tid, wv, lane, taus);
        if (tid < l) {
            const R d = W[(size_t)jp[tid] * ldw + tid].re;
            if (d == (R)0 || !isfinite(d)) atomicMin(rk, tid);
        }
        __syncthreads();
        const int r = *rk;
        if (tid == 0) g.ranks[b] = r;
        cplx<R> *Qb = g.q.p + (int64_t)b * g.qbs;
        if (n <= 128) brsc_form_q<R, 2>(W, ldw, n, l, r, jp, taus, Qs, Qb, g.q.rs, g.q.cs, wv, lane);
        else if (n <= 256) brsc_form_q<R, 4>(W, ldw, n, l, r, jp, taus, Qs, Qb, g.q.rs, g.q.cs, wv, lane);
        else brsc_form_q<R, 8>(W, ldw, n, l, r, jp, taus, Qs, Qb, g.q.rs, g.q.cs, wv, lane);
        __syncthreads();  // the slot's conj(Q) is read by every wave below
        // ---- the projection P^T = conj(Q) A^T: the sketch of a's transposed view with the slot's conj(Q), into p's transposed view -----------
        {
            BscArgs<R> s;
            s.a = CV<R>{g.a.p, n, m, g.a.cs, g.a.rs};
            s.omega = CV<R>{Qs, l, n, n, 1};
            s.y = CV<R>{g.p.p, l, m, g.p.cs, g.p.rs};
            cplx<R> *Pb = g.p.p + (int64_t)b * g.pbs;
            int t = tid;
            asm volatile("" : "+v"(t));
            RC_BSC_PASSES(!AR, false, BSC_W_NONE, s, A, Qs, Pb, nullptr, 0, t, g.p_conj)
        }
        __syncthreads();  // W, conj(Q), jp and the small arrays are rewritten by the next block
    }
}
#undef RC_BSC_PASSES

// ---- what the shared plans and launchers take from this family (batched_launchers.hpp) ------------------------------------------------------
template <typename R>
struct ComplexFamily {
    using RecompressArgs = BrcCArgs<R>;
    using SketchIdArgs = BscArgs<R>;
    using RangeStepArgs = BrscArgs<R>;
    static size_t svd_lds_bytes(int M, int N, BsvPlace p) { return bsc_lds_bytes<R>(M, N, p.ld, p.w, p.v, p.g); }
    static size_t svd_ws_elems(int M, int N, BsvPlace p) { return bsc_ws_elems(M, N, p.ld, p.w, p.v, p.g); }
    static auto svd_kernel(BsvPlace p) {
        return p.w   ? k_batched_svd_c<R, true, true, true>
               : p.v ? k_batched_svd_c<R, false, true, true>
               : p.g ? k_batched_svd_c<R, false, false, true>
                     : k_batched_svd_c<R, false, false, false>;
    }
    static size_t recompress_lds_bytes(int m, int n, int K, BrcPlace p) { return brcc_lds_bytes<R>(m, n, K, p.ld, p.l, p.r, p.v, p.g); }
    static size_t recompress_ws_elems(int form, int m, int n, int K, BrcPlace p) {
        return form == BRC_LARGE  ? brlc_ws_elems(m, n, K, p.ld, p.l, p.r, p.v, p.g)
               : form == BRC_TALL ? brtc_ws_elems(m, n, K, p.ld, p.l, p.r, p.v, p.g)
                                  : brcc_ws_elems(m, n, K, p.ld, p.l, p.r, p.v, p.g);
    }
    // m <= BRT_H under the tall call is the small instance, n <= BRT_H under the large call the tall call's: the same bits at the same rate
    template <int FORM>
    static auto recompress_kernel(int m, int n) {
        constexpr bool TALL = FORM != BRC_SMALL, LARGE = FORM == BRC_LARGE;
        return LARGE && n > BRT_H   ? k_batched_recompress_c<R, TALL, LARGE>
               : TALL && m > BRT_H ? k_batched_recompress_c<R, TALL>
                                   : k_batched_recompress_c<R, false>;
    }
    static size_t sketch_id_lds_bytes(int l, int n, bool w_lds) { return bsc_lds_bytes<R>(l, n, w_lds); }
    static auto sketch_id_kernel(bool a_rows, bool o_rows) {
        void (*const kerns[4])(BscArgs<R>) = {k_batched_sketch_id_c<R, false, false>, k_batched_sketch_id_c<R, false, true>, k_batched_sketch_id_c<R, true, false>,
                                              k_batched_sketch_id_c<R, true, true>};
        return kerns[(a_rows ? 2 : 0) + (o_rows ? 1 : 0)];
    }
    static size_t range_step_lds_bytes(int l, int n, bool w_lds) { return brsc_lds_bytes<R>(l, n, w_lds); }
    static auto range_step_kernel(bool a_rows, bool o_rows) {
        void (*const kerns[4])(BrscArgs<R>) = {k_batched_range_step_c<R, false, false>, k_batched_range_step_c<R, false, true>,
                                               k_batched_range_step_c<R, true, false>, k_batched_range_step_c<R, true, true>};
        return kerns[(a_rows ? 2 : 0) + (o_rows ? 1 : 0)];
    }
};

}  // namespace

template <> struct BatchedFamily<cplx<double>> : ComplexFamily<double> {};
template <> struct BatchedFamily<cplx<float>> : ComplexFamily<float> {};

// (the launchers: batched_launchers.hpp)
RC_INSTANTIATE_BATCHED_SKETCH(cplx<double>, cplx<float>)
RC_INSTANTIATE_BATCHED_ID_SVD(cplx<double>, cplx<float>)
RC_INSTANTIATE_BATCHED_RECOMPRESS(cplx<double>, cplx<float>)

}  // namespace rc
