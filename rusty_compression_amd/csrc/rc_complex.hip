// Complex scalars (c32 / c64) of the hot path: the `_c32` / `_c64` entry points of the C ABI.
//
// The reference instantiates every trait for f32, f64, c32, c64 through macros
// (/root/reference/src/qr.rs:408-416, src/pivoted_qr.rs:187-190, src/svd.rs:188-191, src/random_sampling.rs:123-126,
// :165-168, :277-280, src/types.rs:198-204); conjugation semantics: `conj_matmat` is A^H X (src/types.rs:128-132),
// Q^H everywhere the real code has Q^T.  LAPACK routines behind it: ?geqp3 with rwork (src/pivoted_qr.rs:161-172),
// ?ungqr, ?gesdd, ?trtrs on complex data.
//
// Design.  Complex data is interleaved (re, im) -- the layout of ndarray's Complex<T> / numpy complex -- and every
// operand is first brought into a column-major working copy (any strides, optional conjugate / transpose folded into
// that copy), so the kernels see one layout:
//   * products: "4M" on the real MFMA GEMM -- the operands are split into real and imaginary planes, four real GEMMs
//     (kernels_gemm.hip) form Re C and Im C, one kernel recombines with the complex alpha / beta;
//   * pivoted QR: ?geqp3 / ?laqp2 semantics with complex Householder reflectors (?larfg: beta real, tau complex;
//     applied as H^H = I - conj(tau) v v^H), LAPACK's norm down-dating, first-maximum pivoting; Q by ?ung2r;
//   * SVD: one-sided (Hestenes) Jacobi with complex rotations on the tall orientation, one launch per round of the
//     circle-method schedule (the pairs of a round are disjoint); singular values are real, descending;
//   * triangular solves: back substitution, one thread per right-hand side.
// These are correct, deterministic and column-parallel, but not tuned like the real-scalar kernels: complex is the
// breadth row of SURVEY.md 8(f), the measured hot path (BASELINE.json) is real.
#include "rc_common.hpp"
#include "rc_cplx.hpp"
#include "rc_device.hpp"

#include <algorithm>
#include <cmath>

using namespace rc;

namespace {

// the column-major working matrix (cplx<R>, CV<R> and view_of: rc_cplx.hpp); every temporary of this family has this layout, Omega too
template <typename E>
Mat<E> tmp_colmajor(rc_context *c, int64_t rows, int64_t cols) {
    const int64_t ld = std::max<int64_t>(rows, 1);
    return Mat<E>{c->alloc<E>((size_t)ld * std::max<int64_t>(cols, 1)), rows, cols, 1, ld};
}
template <typename E>
Mat<E> tmp_omega(rc_context *c, int64_t rows, int64_t cols) { return tmp_colmajor<E>(c, rows, cols); }

// ------------------------------------------------------------------------------------------------ elementwise kernels
template <typename R>
__global__ __launch_bounds__(256) void k_c_copy(CV<R> src, CV<R> dst, int conj) {  // dst = src or conj(src); any strides
    const int64_t total = dst.rows * dst.cols;
    const bool col_fast = dst.cs <= dst.rs;
    for (int64_t e = blockIdx.x * (int64_t)256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        int64_t i, j;
        if (col_fast) { i = e / dst.cols; j = e - i * dst.cols; }
        else { j = e / dst.rows; i = e - j * dst.rows; }
        cplx<R> v = src.at(i, j);
        if (conj) v.im = -v.im;
        dst.at(i, j) = v;
    }
}
template <typename R>
void copy_mat(rc_context *c, CV<R> src, CV<R> dst, bool conj = false) {
    RC_REQUIRE(src.rows == dst.rows && src.cols == dst.cols, RC_INVALID_ARGUMENT, "complex copy: shape mismatch");
    if (dst.empty()) return;
    hipLaunchKernelGGL(k_c_copy<R>, dim3((unsigned)std::min<int64_t>(cdiv(dst.rows * dst.cols, 256), 8192)), dim3(256), 0, c->stream, src, dst, conj ? 1 : 0);
}
template <typename R>
__global__ __launch_bounds__(256) void k_c_fill(CV<R> dst, int identity) {
    const int64_t total = dst.rows * dst.cols;
    for (int64_t e = blockIdx.x * (int64_t)256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int64_t j = e / dst.rows, i = e - j * dst.rows;
        dst.at(i, j) = cplx<R>{(identity && i == j) ? (R)1 : (R)0, (R)0};
    }
}
template <typename R>
void c_fill(rc_context *c, CV<R> dst, bool identity) {
    if (dst.empty()) return;
    hipLaunchKernelGGL(k_c_fill<R>, dim3((unsigned)std::min<int64_t>(cdiv(dst.rows * dst.cols, 256), 8192)), dim3(256), 0, c->stream, dst, identity ? 1 : 0);
}
template <typename R>
__global__ __launch_bounds__(256) void k_c_gather_cols(CV<R> src, const int64_t *idx, CV<R> dst, int *health) {  // dst[:, j] = src[:, idx[j]]
    const int64_t total = dst.rows * dst.cols;
    for (int64_t e = blockIdx.x * (int64_t)256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int64_t j = e / dst.rows, i = e - j * dst.rows;
        const int64_t s = idx[j];
        if ((uint64_t)s < (uint64_t)src.cols) {
            dst.at(i, j) = src.at(i, s);
        } else {  // (as k_gather_cols: no wild addresses; health bit 32)
            dst.at(i, j) = cplx<R>{0, 0};
            if (i == 0) atomicOr(health, 32);
        }
    }
}
template <typename R>
void gather_cols(rc_context *c, CV<R> src, const int64_t *idx, CV<R> dst) {
    if (dst.empty()) return;
    hipLaunchKernelGGL(k_c_gather_cols<R>, dim3((unsigned)std::min<int64_t>(cdiv(dst.rows * dst.cols, 256), 8192)), dim3(256), 0, c->stream, src, idx, dst, c->health_word());
}
template <typename R>
__global__ __launch_bounds__(256) void k_c_scale_rows(const R *s, CV<R> m) {  // m[i, :] *= s[i]
    const int64_t total = m.rows * m.cols;
    for (int64_t e = blockIdx.x * (int64_t)256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int64_t j = e / m.rows, i = e - j * m.rows;
        cplx<R> v = m.at(i, j);
        m.at(i, j) = s[i] * v;
    }
}
// planes for the 4M product: re / im as real column-major matrices with the same leading dimension
template <typename R>
__global__ __launch_bounds__(256) void k_c_split(CV<R> src, R *re, R *im, int64_t ld) {
    const int64_t total = src.rows * src.cols;
    for (int64_t e = blockIdx.x * (int64_t)256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int64_t j = e / src.rows, i = e - j * src.rows;
        const cplx<R> v = src.at(i, j);
        re[i + j * ld] = v.re;
        im[i + j * ld] = v.im;
    }
}
template <typename R>
__global__ __launch_bounds__(256) void k_c_combine(const R *re, const R *im, int64_t ld, cplx<R> alpha, cplx<R> beta, CV<R> dst) {
    const int64_t total = dst.rows * dst.cols;
    for (int64_t e = blockIdx.x * (int64_t)256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int64_t j = e / dst.rows, i = e - j * dst.rows;
        cplx<R> v = alpha * cplx<R>{re[i + j * ld], im[i + j * ld]};
        if (beta.re != (R)0 || beta.im != (R)0) v = v + beta * dst.at(i, j);
        dst.at(i, j) = v;
    }
}


// out[j] = ||a[:, j]||^2 (column-major a), one wave per column
template <typename R>
__global__ __launch_bounds__(256) void k_c_col_sumsq(CV<R> a, R *out) {
    const int lane = threadIdx.x & 63;
    for (int64_t j = blockIdx.x * 4 + (threadIdx.x >> 6); j < a.cols; j += (int64_t)gridDim.x * 4) {
        R acc = 0;
        for (int64_t i = lane; i < a.rows; i += 64) acc += abs2(a.at(i, j));
        acc = wave_sum_dpp(acc);
        if (lane == 0) out[j] = acc;
    }
}
// out2[0] = ||a - b||_F^2, out2[1] = ||b||_F^2 : one workgroup, fixed order (small matrices only on this path); both operands are read
// times 2^-e, e the device word of input_exponent(a, b) (as k_fro_partial, kernels_util.hip)
template <typename R>
__global__ __launch_bounds__(1024) void k_c_fro(CV<R> a, CV<R> b, R *out2, const int *e) {
    __shared__ R sh[32];
    const int down = -*e;
    R d2 = 0, b2 = 0;
    const int64_t total = a.rows * a.cols;
    for (int64_t e = threadIdx.x; e < total; e += 1024) {
        const int64_t j = e / a.rows, i = e - j * a.rows;
        cplx<R> x = a.at(i, j), y = b.at(i, j);
        x = {ldexp(x.re, down), ldexp(x.im, down)};
        y = {ldexp(y.re, down), ldexp(y.im, down)};
        d2 += abs2(x - y);
        b2 += abs2(y);
    }
    d2 = wave_sum_dpp(d2);
    b2 = wave_sum_dpp(b2);
    if ((threadIdx.x & 63) == 0) { sh[threadIdx.x >> 6] = d2; sh[16 + (threadIdx.x >> 6)] = b2; }
    __syncthreads();
    if (threadIdx.x == 0) {
        R s1 = 0, s2 = 0;
        for (int i = 0; i < 16; ++i) { s1 += sh[i]; s2 += sh[16 + i]; }
        out2[0] = s1;
        out2[1] = s2;
    }
}

// ------------------------------------------------------------------------------------------------ products (4M)
// C = alpha op(A) op(B) + beta C;  A, B, C: any strided views;  op: 0 none, 1 transpose, 2 conjugate transpose
template <typename R>
void c_gemm(rc_context *c, int opa, int opb, cplx<R> alpha, CV<R> a, CV<R> b, cplx<R> beta, CV<R> cm) {
    if (opa) a = a.t();
    if (opb) b = b.t();
    const R sa = opa == 2 ? (R)-1 : (R)1, sb = opb == 2 ? (R)-1 : (R)1;  // sign of the imaginary plane
    RC_REQUIRE(a.cols == b.rows && a.rows == cm.rows && b.cols == cm.cols, RC_INVALID_ARGUMENT, "complex gemm: shapes (%lld x %lld) * (%lld x %lld) -> (%lld x %lld)",
               (long long)a.rows, (long long)a.cols, (long long)b.rows, (long long)b.cols, (long long)cm.rows, (long long)cm.cols);
    if (cm.empty()) return;
    ArenaMark mark(c);
    const int64_t m = a.rows, k = a.cols, n = b.cols;
    const int64_t lda = even_ld(std::max<int64_t>(m, 1)), ldb = even_ld(std::max<int64_t>(k, 1)), ldc = even_ld(std::max<int64_t>(m, 1));
    R *ar = c->alloc<R>((size_t)lda * std::max<int64_t>(k, 1)), *ai = c->alloc<R>((size_t)lda * std::max<int64_t>(k, 1));
    R *br = c->alloc<R>((size_t)ldb * n), *bi = c->alloc<R>((size_t)ldb * n);
    R *cr = c->alloc<R>((size_t)ldc * n), *ci = c->alloc<R>((size_t)ldc * n);
    if (k == 0) {  // empty inner dimension: C = beta C
        fill_words(c, cr, (size_t)ldc * n * sizeof(R), 0u);
        fill_words(c, ci, (size_t)ldc * n * sizeof(R), 0u);
        hipLaunchKernelGGL(k_c_combine<R>, dim3((unsigned)std::min<int64_t>(cdiv(m * n, 256), 8192)), dim3(256), 0, c->stream, cr, ci, ldc, alpha, beta, cm);
        return;
    }
    if (k > 0) {
        hipLaunchKernelGGL(k_c_split<R>, dim3((unsigned)std::min<int64_t>(cdiv(m * k, 256), 8192)), dim3(256), 0, c->stream, a, ar, ai, lda);
        hipLaunchKernelGGL(k_c_split<R>, dim3((unsigned)std::min<int64_t>(cdiv(k * n, 256), 8192)), dim3(256), 0, c->stream, b, br, bi, ldb);
    }
    Mat<R> Ar = colmajor(ar, m, k, lda), Ai = colmajor(ai, m, k, lda), Br = colmajor(br, k, n, ldb), Bi = colmajor(bi, k, n, ldb);
    Mat<R> Cr = colmajor(cr, m, n, ldc), Ci = colmajor(ci, m, n, ldc);
    // Re C = Ar Br - (sa sb) Ai Bi ;  Im C = sb Ar Bi + sa Ai Br   (four products on the real MFMA GEMM)
    gemm<R>(c, (R)1, Ar, Br, (R)0, Cr);
    gemm<R>(c, -(sa * sb), Ai, Bi, (R)1, Cr);
    gemm<R>(c, sb, Ar, Bi, (R)0, Ci);
    gemm<R>(c, sa, Ai, Br, (R)1, Ci);
    hipLaunchKernelGGL(k_c_combine<R>, dim3((unsigned)std::min<int64_t>(cdiv(m * n, 256), 8192)), dim3(256), 0, c->stream, cr, ci, ldc, alpha, beta, cm);
}
template <typename R> cplx<R> one() { return cplx<R>{(R)1, (R)0}; }
template <typename R> cplx<R> zero() { return cplx<R>{(R)0, (R)0}; }

// ------------------------------------------------------------------------------------------------ pivoted QR
// step j: pivot (first maximum), swap by index, ?larfg on the pivot column; one workgroup
template <typename R>
__global__ __launch_bounds__(1024) void k_c_qr_pivot_reflect(CV<R> w, int64_t j, int pivot, int64_t *jpvt, R *vn1, R *vn2, cplx<R> *tau) {
    __shared__ R shv[16];
    __shared__ long long shi[16];
    __shared__ R shs[16];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int64_t n = w.cols, m = w.rows;
    if (pivot) {
        R best = (R)-1;
        long long bi = 0x7fffffffffffffffLL;
        for (int64_t p = j + tid; p < n; p += 1024) {
            const R v = fabs(vn1[p]);
            if (v > best) { best = v; bi = p; }
        }
        for (int off = 32; off > 0; off >>= 1) {
            const R ob = __shfl_xor(best, off, 64);
            const long long oi = __shfl_xor(bi, off, 64);
            if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
        }
        if (lane == 0) { shv[wv] = best; shi[wv] = bi; }
        __syncthreads();
        if (tid == 0) {
            for (int q = 1; q < 16; ++q)
                if (shv[q] > best || (shv[q] == best && shi[q] < bi)) { best = shv[q]; bi = shi[q]; }
            const int64_t pvt = (bi >= j && bi < n) ? (int64_t)bi : j;
            if (pvt != j) {
                const int64_t t = jpvt[pvt]; jpvt[pvt] = jpvt[j]; jpvt[j] = t;
                vn1[pvt] = vn1[j];
                vn2[pvt] = vn2[j];
            }
        }
        __syncthreads();
    }
    cplx<R> *col = w.p + jpvt[j] * w.cs;
    const cplx<R> alpha = col[j];
    R acc = 0;
    for (int64_t i = j + 1 + tid; i < m; i += 1024) acc += abs2(col[i]);
    acc = wave_sum_dpp(acc);
    if (lane == 0) shs[wv] = acc;
    __syncthreads();
    R ssq = 0;
    for (int q = 0; q < 16; ++q) ssq += shs[q];
    const R xnorm = sqrt(ssq);
    if (xnorm == (R)0 && alpha.im == (R)0) {  // ?larfg: H = I
        if (tid == 0) tau[j] = cplx<R>{0, 0};
        return;
    }
    const R beta = -copysign(sqrt(alpha.re * alpha.re + alpha.im * alpha.im + ssq), alpha.re);  // ?lapy3
    const cplx<R> scal = cdiv(cplx<R>{(R)1, (R)0}, cplx<R>{alpha.re - beta, alpha.im});
    for (int64_t i = j + 1 + tid; i < m; i += 1024) col[i] = col[i] * scal;
    if (tid == 0) {
        tau[j] = cplx<R>{(beta - alpha.re) / beta, -alpha.im / beta};
        col[j] = cplx<R>{beta, (R)0};
    }
}
// apply H_j^H = I - conj(tau) v v^H to every remaining column + LAPACK norm down-date; one workgroup per column
template <typename R>
__global__ __launch_bounds__(256) void k_c_qr_apply(CV<R> w, int64_t j, int pivot, const int64_t *jpvt, R *vn1, R *vn2, const cplx<R> *tau) {
    __shared__ R sh[8];
    const int64_t n = w.cols, m = w.rows;
    const int64_t p = j + 1 + blockIdx.x;
    if (p >= n) return;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const cplx<R> tj = tau[j];
    const cplx<R> *v = w.p + jpvt[j] * w.cs;
    cplx<R> *x = w.p + jpvt[p] * w.cs;
    if (tj.re != (R)0 || tj.im != (R)0) {
        cplx<R> dot{0, 0};  // v^H x
        for (int64_t i = j + tid; i < m; i += 256) {
            const cplx<R> vi = i == j ? cplx<R>{(R)1, (R)0} : v[i];
            dot = dot + cj(vi) * x[i];
        }
        R dr = wave_sum_dpp(dot.re), di = wave_sum_dpp(dot.im);
        __syncthreads();
        if (lane == 0) { sh[wv] = dr; sh[4 + wv] = di; }
        __syncthreads();
        dr = (sh[0] + sh[1]) + (sh[2] + sh[3]);
        di = (sh[4] + sh[5]) + (sh[6] + sh[7]);
        const cplx<R> f = cj(tj) * cplx<R>{dr, di};
        for (int64_t i = j + tid; i < m; i += 256) {
            const cplx<R> vi = i == j ? cplx<R>{(R)1, (R)0} : v[i];
            x[i] = x[i] - f * vi;
        }
    }
    if (!pivot) return;
    __syncthreads();
    const R vn = vn1[p];
    if (vn == (R)0) return;
    const R t = cabs(x[j]) / vn;
    R temp = (R)1 - t * t;
    temp = temp > (R)0 ? temp : (R)0;
    const R r = vn / vn2[p];
    if (temp * r * r <= num<R>::tol3z()) {
        R ss = 0;
        for (int64_t i = j + 1 + tid; i < m; i += 256) ss += abs2(x[i]);
        ss = wave_sum_dpp(ss);
        __syncthreads();
        if (lane == 0) sh[wv] = ss;
        __syncthreads();
        if (tid == 0) { const R nn = (j < m - 1) ? sqrt((sh[0] + sh[1]) + (sh[2] + sh[3])) : (R)0; vn1[p] = nn; vn2[p] = nn; }
    } else if (tid == 0) {
        vn1[p] = vn * sqrt(temp);
    }
}
template <typename R>
__global__ __launch_bounds__(256) void k_c_qr_init(CV<R> w, int64_t *jpvt, R *vn1, R *vn2) {
    const int lane = threadIdx.x & 63;
    for (int64_t j = blockIdx.x * 4 + (threadIdx.x >> 6); j < w.cols; j += (int64_t)gridDim.x * 4) {
        R acc = 0;
        for (int64_t i = lane; i < w.rows; i += 64) acc += abs2(w.at(i, j));
        acc = sqrt(wave_sum_dpp(acc));
        if (lane == 0) { vn1[j] = acc; vn2[j] = acc; jpvt[j] = j; }
    }
}
// w: column-major m x n, overwritten with the ?geqp3 output format (columns never moved: jpvt maps position -> column)
template <typename R>
void c_geqp3(rc_context *c, CV<R> w, int64_t kmax, int64_t *jpvt, cplx<R> *tau) {
    const int64_t m = w.rows, n = w.cols;
    if (m == 0 || n == 0) return;
    kmax = std::min(kmax, std::min(m, n));
    ProfScope ps(c, "op:geqp3<complex> %lldx%lld k=%lld", (long long)m, (long long)n, (long long)kmax);
    ArenaMark mark(c);
    R *vn1 = c->alloc<R>((size_t)n), *vn2 = c->alloc<R>((size_t)n);
    hipLaunchKernelGGL(k_c_qr_init<R>, dim3((unsigned)std::min<int64_t>(cdiv(n, 4), 8192)), dim3(256), 0, c->stream, w, jpvt, vn1, vn2);
    for (int64_t j = 0; j < kmax; ++j) {
        hipLaunchKernelGGL(k_c_qr_pivot_reflect<R>, dim3(1), dim3(1024), 0, c->stream, w, j, 1, jpvt, vn1, vn2, tau);
        if (n - j - 1 > 0) hipLaunchKernelGGL(k_c_qr_apply<R>, dim3((unsigned)(n - j - 1)), dim3(256), 0, c->stream, w, j, 1, jpvt, vn1, vn2, tau);
    }
}
// r(i, p) = (i <= p) ? w(i, jpvt[p]) : 0
template <typename R>
__global__ __launch_bounds__(256) void k_c_extract_r(CV<R> w, const int64_t *jpvt, CV<R> r) {
    const int64_t total = r.rows * r.cols;
    for (int64_t e = blockIdx.x * (int64_t)256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int64_t p = e / r.rows, i = e - p * r.rows;
        r.at(i, p) = i <= p ? w.p[jpvt[p] * w.cs + i] : cplx<R>{0, 0};
    }
}
// q(:, cq) = H_0 ... H_{k-1} e_cq (?ung2r), one workgroup per column, the column lives in q
template <typename R>
__global__ __launch_bounds__(256) void k_c_form_q(CV<R> w, const int64_t *jpvt, const cplx<R> *tau, int64_t k, CV<R> q) {
    __shared__ R sh[8];
    const int64_t m = w.rows, cq = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    cplx<R> *x = q.p + cq * q.cs;
    for (int64_t i = tid; i < m; i += 256) x[i] = cplx<R>{i == cq ? (R)1 : (R)0, (R)0};
    for (int64_t j = (cq < k - 1 ? cq : k - 1); j >= 0; --j) {
        const cplx<R> tj = tau[j];
        if (tj.re == (R)0 && tj.im == (R)0) continue;
        const cplx<R> *v = w.p + jpvt[j] * w.cs;
        // thread tid owns the rows i = tid (mod 256) for the whole kernel: x[i] is only ever touched by its owner (the loops used
        // to start at j + tid, which moved a row from thread to thread between steps with no barrier in between: a race between
        // waves, visible as ~1e-4 errors of the c32 factor at k = 200)
        const int64_t i0 = tid >= j ? tid : tid + ((j - tid + 255) / 256) * 256;
        cplx<R> dot{0, 0};
        for (int64_t i = i0; i < m; i += 256) {
            const cplx<R> vi = i == j ? cplx<R>{(R)1, (R)0} : v[i];
            dot = dot + cj(vi) * x[i];
        }
        R dr = wave_sum_dpp(dot.re), di = wave_sum_dpp(dot.im);
        __syncthreads();
        if (lane == 0) { sh[wv] = dr; sh[4 + wv] = di; }
        __syncthreads();
        const cplx<R> f = tj * cplx<R>{(sh[0] + sh[1]) + (sh[2] + sh[3]), (sh[4] + sh[5]) + (sh[6] + sh[7])};
        for (int64_t i = i0; i < m; i += 256) {
            const cplx<R> vi = i == j ? cplx<R>{(R)1, (R)0} : v[i];
            x[i] = x[i] - f * vi;
        }
    }
}
// T X = B in place, T upper triangular k x k, one thread per right-hand side column
template <typename R>
__global__ __launch_bounds__(256) void k_c_trsm_upper(CV<R> t, CV<R> b) {
    const int64_t col = blockIdx.x * (int64_t)256 + threadIdx.x;
    if (col >= b.cols) return;
    const int64_t k = t.rows;
    for (int64_t i = k - 1; i >= 0; --i) {
        cplx<R> acc = b.at(i, col);
        for (int64_t l = i + 1; l < k; ++l) acc = acc - t.at(i, l) * b.at(l, col);
        b.at(i, col) = cdiv(acc, t.at(i, i));
    }
}

// A P = Q R with k = q.cols = r.rows steps;  a: any view (not modified), q / r: any views (may be empty)
template <typename R>
void c_pivoted_qr(rc_context *c, CV<R> a, CV<R> q, CV<R> r, int64_t *ind, int64_t k) {
    const int64_t m = a.rows, n = a.cols;
    RC_REQUIRE(k <= std::min(m, n), RC_INVALID_ARGUMENT, "pivoted_qr: rank %lld exceeds min(m, n)", (long long)k);
    if (n == 0) return;
    ArenaMark mark(c);
    CV<R> w = tmp_colmajor<cplx<R>>(c, m, n);
    copy_mat(c, a, w);
    cplx<R> *tau = c->alloc<cplx<R>>((size_t)std::max<int64_t>(k, 1));
    c_geqp3(c, w, k, ind, tau);
    if (!r.empty()) {
        CV<R> rw = tmp_colmajor<cplx<R>>(c, r.rows, n);
        hipLaunchKernelGGL(k_c_extract_r<R>, dim3((unsigned)std::min<int64_t>(cdiv(r.rows * n, 256), 8192)), dim3(256), 0, c->stream, w, ind, rw);
        copy_mat(c, rw, r);
    }
    if (!q.empty()) {
        CV<R> qw = tmp_colmajor<cplx<R>>(c, m, q.cols);
        hipLaunchKernelGGL(k_c_form_q<R>, dim3((unsigned)q.cols), dim3(256), 0, c->stream, w, ind, tau, k, qw);
        copy_mat(c, qw, q);
    }
}

// LAPACK granularity (see lapack_geqp3 / lapack_orgqr in rc_api.hip): ?geqp3 with the columns in pivoted order, ?ungqr
template <typename R>
void c_lapack_geqp3(rc_context *c, CV<R> a, int64_t kmax, int64_t *jpvt, cplx<R> *tau) {
    const int64_t m = a.rows, n = a.cols;
    RC_REQUIRE(kmax >= 0 && kmax <= std::min(m, n), RC_INVALID_ARGUMENT, "geqp3: need 0 <= kmax <= min(m, n)");
    RC_REQUIRE(jpvt != nullptr && (kmax == 0 || tau != nullptr), RC_INVALID_ARGUMENT, "geqp3: null jpvt / tau");
    if (n == 0) return;
    if (kmax == 0 || m == 0) { iota_i64(c, jpvt, n); return; }
    ArenaMark mark(c);
    CV<R> w = tmp_colmajor<cplx<R>>(c, m, n);
    const int *e = input_exponent(c, a);  // input scale: factor 2^-e a; R takes 2^e back, the reflectors and tau carry none
    copy_mat_scaled(c, a, w, e);
    c_geqp3(c, w, kmax, jpvt, tau);
    gather_cols(c, w, jpvt, a);
    rescale(c, a, e, 1, kmax);
}
template <typename R>
void c_lapack_ungqr(rc_context *c, CV<R> a, const cplx<R> *tau, int64_t k, CV<R> q) {
    const int64_t m = a.rows;
    RC_REQUIRE(k >= 0 && k <= std::min(m, a.cols) && q.rows == m && q.cols == k, RC_INVALID_ARGUMENT,
               "orgqr: need k <= min(m, n) reflectors in a and q of m x k");
    if (k == 0 || m == 0) return;
    RC_REQUIRE(tau != nullptr, RC_INVALID_ARGUMENT, "orgqr: null tau");
    ArenaMark mark(c);
    int64_t *ident = c->alloc<int64_t>((size_t)k);
    iota_i64(c, ident, k);
    CV<R> w = tmp_colmajor<cplx<R>>(c, m, k), qw = tmp_colmajor<cplx<R>>(c, m, k);
    CV<R> ak = a; ak.cols = k;
    copy_mat(c, ak, w);
    hipLaunchKernelGGL(k_c_form_q<R>, dim3((unsigned)k), dim3(256), 0, c->stream, w, ident, tau, k, qw);
    copy_mat(c, qw, q);
}

// ------------------------------------------------------------------------------------------------ SVD (one-sided Jacobi)
__device__ inline void rr_pair_c(int N, int r, int pi, int &p, int &q) {  // circle method, round r, pair pi
    if (pi == 0) { p = N - 1; q = r; }
    else { p = (r + pi) % (N - 1); q = (r - pi + (N - 1)) % (N - 1); }
    if (p > q) { const int t = p; p = q; q = t; }
}
template <typename R>
__global__ __launch_bounds__(256) void k_c_jacobi_round(CV<R> g, CV<R> v, int r, int *state) {
    if (state[1]) return;
    const int n = (int)g.cols, N = (n + 1) & ~1;
    const int lane = threadIdx.x & 63;
    const int pi = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (pi >= N / 2) return;
    int p, q;
    rr_pair_c(N, r, pi, p, q);
    if (q >= n) return;
    const int64_t M = g.rows;
    cplx<R> *gp = g.p + (int64_t)p * g.cs, *gq = g.p + (int64_t)q * g.cs;
    R app = 0, aqq = 0;
    cplx<R> apq{0, 0};
    for (int64_t i = lane; i < M; i += 64) {
        const cplx<R> a = gp[i], b = gq[i];
        app += abs2(a);
        aqq += abs2(b);
        apq = apq + cj(a) * b;
    }
    app = wave_sum_dpp(app);
    aqq = wave_sum_dpp(aqq);
    apq.re = wave_sum_dpp(apq.re);
    apq.im = wave_sum_dpp(apq.im);
    const R habs = hypot(apq.re, apq.im);
    const R tol = sqrt((R)M) * num<R>::eps();
    if (habs == (R)0 || habs <= tol * sqrt(app) * sqrt(aqq)) return;
    // q~ = e^{-i phi} q makes p^H q~ = |apq| real: a real Jacobi rotation between p and q~.
    // The phase and the rotation parameters are evaluated in f64 for both precisions (as in the real kernels): in f32,
    // c^2 + s^2 - 1 and |phase|^2 - 1 have a systematic sign and the thousands of rotations a column undergoes inflate the
    // singular values by a few 1e-5 (the reference's c32 tests ask for 1e-5: src/svd.rs:291).
    const double hd = hypot((double)apq.re, (double)apq.im);
    const cplx<R> ph{(R)((double)apq.re / hd), (R)(-(double)apq.im / hd)};
    const double zeta = ((double)aqq - (double)app) / (2.0 * hd);
    const double td = copysign(1.0, zeta) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
    const double cd = 1.0 / sqrt(1.0 + td * td);
    const R cs = (R)cd, sn = (R)(cd * td);
    for (int64_t i = lane; i < M; i += 64) {
        const cplx<R> a = gp[i], b = ph * gq[i];
        gp[i] = cs * a - sn * b;
        gq[i] = sn * a + cs * b;
    }
    cplx<R> *vp = v.p + (int64_t)p * v.cs, *vq = v.p + (int64_t)q * v.cs;
    for (int64_t i = lane; i < n; i += 64) {
        const cplx<R> a = vp[i], b = ph * vq[i];
        vp[i] = cs * a - sn * b;
        vq[i] = sn * a + cs * b;
    }
    if (lane == 0) state[0] = 1;
}
__global__ void k_c_jacobi_sweep_end(int *state) {
    if (threadIdx.x != 0 || state[1]) return;
    state[2] += 1;
    if (state[0] == 0) state[1] = 1;
    state[0] = 0;
}
template <typename R>
__global__ __launch_bounds__(256) void k_c_jacobi_norms(CV<R> g, R *sig) {
    const int lane = threadIdx.x & 63;
    const int64_t j = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (j >= g.cols) return;
    R acc = 0;
    for (int64_t i = lane; i < g.rows; i += 64) acc += abs2(g.at(i, j));
    acc = wave_sum_dpp(acc);
    if (lane == 0) sig[j] = sqrt(acc);
}
template <typename R>
__global__ __launch_bounds__(256) void k_c_jacobi_rank(int n, const R *sig, int *order, R *s) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const R si = sig[i];
    int rank = 0;
    for (int j = 0; j < n; ++j) rank += (sig[j] > si || (sig[j] == si && j < i)) ? 1 : 0;
    order[i] = rank;
    s[rank] = si;
}
// uc(:, order[j]) = g(:, j) / sig[j], vc(:, order[j]) = v(:, j)
template <typename R>
__global__ __launch_bounds__(256) void k_c_jacobi_emit(CV<R> g, CV<R> v, const R *sig, const int *order, CV<R> uc, CV<R> vc) {
    const int lane = threadIdx.x & 63;
    const int64_t j = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (j >= g.cols) return;
    const int dst = order[j];
    const R sj = sig[j];
    const R inv = sj > (R)0 ? (R)1 / sj : (R)0;
    for (int64_t i = lane; i < g.rows; i += 64) uc.at(i, dst) = inv * g.at(i, j);
    for (int64_t i = lane; i < v.rows; i += 64) vc.at(i, dst) = v.at(i, j);
}
// ?gesdd returns orthonormal left vectors also for rank-deficient input; k_c_jacobi_emit leaves a ZERO column of uc for every zero
// singular value.  Complex twin of k_complete_left_basis (kernels_svd.hip), same basis choice: for each zero column, the unit vector
// with the largest component outside the span of the columns before it, orthogonalised twice against them (classical Gram-Schmidt
// with conjugated inner products, one re-orthogonalisation) and normalised.  uc: M x n column-major, M >= n (the square core of the
// QR-first branch or the tall uc of the direct one).  One workgroup; returns at once when the smallest singular value is positive
// (the values are sorted), which is every full-rank call.
template <typename R>
__global__ __launch_bounds__(1024) void k_c_complete_left_basis(CV<R> uc, const R *s) {
    extern __shared__ __attribute__((aligned(16))) char cb_raw[];
    cplx<R> *v = reinterpret_cast<cplx<R> *>(cb_raw);  // M
    cplx<R> *d = v + uc.rows;                             // n: projections
    __shared__ R red_v[16];
    __shared__ int red_i[16];
    __shared__ int sh_p;
    __shared__ R sh_nrm;
    const int M = (int)uc.rows, n = (int)uc.cols, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (!(s[n - 1] == (R)0)) return;
    int z = 0;  // number of positive singular values: columns z .. n-1 are the zero ones
    for (int j = 0; j < n; ++j) z += s[j] > (R)0 ? 1 : 0;
    for (int j = z; j < n; ++j) {
        // residual of every unit vector: 1 - sum_c |U(p, c)|^2 over the columns before j
        R best = (R)-1;
        int bp = 0;
        for (int p = tid; p < M; p += 1024) {
            R acc = 1;
            for (int c2 = 0; c2 < j; ++c2) acc -= abs2(uc.at(p, c2));
            if (acc > best) { best = acc; bp = p; }
        }
        const R mx = wave_max_dpp(best);
        const int cand = wave_min_dpp(best == mx ? bp : 0x7fffffff);
        if (lane == 0) { red_v[wv] = mx; red_i[wv] = cand; }
        __syncthreads();
        if (tid == 0) {
            R b = red_v[0];
            int bi = red_i[0];
            for (int w = 1; w < 16; ++w)
                if (red_v[w] > b || (red_v[w] == b && red_i[w] < bi)) { b = red_v[w]; bi = red_i[w]; }
            sh_p = bi;
        }
        __syncthreads();
        const int p = sh_p;
        for (int i = tid; i < M; i += 1024) v[i] = cplx<R>{i == p ? (R)1 : (R)0, (R)0};
        __syncthreads();
        for (int pass = 0; pass < 2; ++pass) {
            for (int c2 = tid; c2 < j; c2 += 1024) {  // d = U(:, :j)^H v
                cplx<R> acc{0, 0};
                for (int i = 0; i < M; ++i) acc = acc + cj(uc.at(i, c2)) * v[i];
                d[c2] = acc;
            }
            __syncthreads();
            for (int i = tid; i < M; i += 1024) {  // v -= U(:, :j) d
                cplx<R> acc = v[i];
                for (int c2 = 0; c2 < j; ++c2) acc = acc - uc.at(i, c2) * d[c2];
                v[i] = acc;
            }
            __syncthreads();
        }
        R part = 0;
        for (int i = tid; i < M; i += 1024) part += abs2(v[i]);
        part = wave_sum_dpp(part);
        if (lane == 0) red_v[wv] = part;
        __syncthreads();
        if (tid == 0) {
            R t = 0;
            for (int w = 0; w < 16; ++w) t += red_v[w];
            sh_nrm = sqrt(t);
        }
        __syncthreads();
        const R inv = (R)1 / sh_nrm;
        for (int i = tid; i < M; i += 1024) uc.at(i, j) = inv * v[i];
        __threadfence();
        __syncthreads();
    }
}
template <typename R>
void c_complete_left_basis(rc_context *c, CV<R> uc, const R *s) {
    if (uc.empty() || uc.rows < uc.cols || uc.rs != 1) return;
    const size_t lds = (size_t)(uc.rows + uc.cols) * sizeof(cplx<R>);
    if (lds > 64 * 1024) return;  // (cores beyond M + n = 4096 c64 keep the zero vectors, as the real kernel does)
    hipLaunchKernelGGL(k_c_complete_left_basis<R>, dim3(1), dim3(1024), lds, c->stream, uc, s);
}
// thin SVD of the TALL column-major g (M x n, M >= n, destroyed): g = uc diag(s) vc^H
template <typename R>
void c_jacobi_svd_tall(rc_context *c, CV<R> g, CV<R> uc, R *s, CV<R> vc) {
    const int n = (int)g.cols, N = (n + 1) & ~1;
    ProfScope ps(c, "op:jacobi_svd<complex> %lldx%d", (long long)g.rows, n);
    ArenaMark mark(c);
    int *state = c->alloc<int>(4);
    R *sig = c->alloc<R>((size_t)n);
    int *order = c->alloc<int>((size_t)n);
    CV<R> v = tmp_colmajor<cplx<R>>(c, n, n);
    fill_words(c, state, 4 * sizeof(int), 0u);
    c_fill(c, v, true);
    RC_REQUIRE(!c->capturing, RC_RUNTIME_ERROR, "complex SVD reads its convergence flag back: not capturable");
    const unsigned grid = (unsigned)((N / 2 + 3) / 4);
    bool converged = false;
    for (int sweep = 0; sweep < 60 && n > 1; ++sweep) {
        for (int r = 0; r < N - 1; ++r) hipLaunchKernelGGL(k_c_jacobi_round<R>, dim3(grid), dim3(256), 0, c->stream, g, v, r, state);
        hipLaunchKernelGGL(k_c_jacobi_sweep_end, dim3(1), dim3(64), 0, c->stream, state);
        int h[4] = {0, 0, 0, 0};
        RC_HIP(hipMemcpyAsync(h, state, sizeof(h), hipMemcpyDeviceToHost, c->stream));
        RC_HIP(hipStreamSynchronize(c->stream));
        if (h[1]) { converged = true; break; }
    }
    RC_REQUIRE(converged || n <= 1, RC_LINALG_ERROR, "complex Jacobi SVD did not converge in 60 sweeps");
    hipLaunchKernelGGL(k_c_jacobi_norms<R>, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, c->stream, g, sig);
    hipLaunchKernelGGL(k_c_jacobi_rank<R>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, n, sig, order, s);
    hipLaunchKernelGGL(k_c_jacobi_emit<R>, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, c->stream, g, v, sig, order, uc, vc);
    c_complete_left_basis(c, uc, s);  // (?gesdd: the left vectors stay orthonormal when singular values are zero; no-op otherwise)
}
template <typename R>
void c_colinv(rc_context *c, CV<R> in, const int64_t *ind, CV<R> out);
// ComputeSVD::compute_svd (src/compute_svd.rs:18-27): a (m x n) = u diag(s) vt, u: m x r, vt: r x n, r = min(m, n)
template <typename R>
void c_compute_svd(rc_context *c, CV<R> a, CV<R> u, R *s, CV<R> vt) {
    const int64_t m = a.rows, n = a.cols, r = std::min(m, n);
    RC_REQUIRE(u.rows == m && u.cols == r && vt.rows == r && vt.cols == n, RC_INVALID_ARGUMENT, "compute_svd: output shapes");
    if (r == 0) return;
    ArenaMark mark(c);
    // Round 3: a clearly rectangular input goes through a QR factorization first (as ?gesdd does): the one-launch-per-round Jacobi
    // then works on the r x r triangle instead of on M-row columns (128 x 2048 c64: 23 -> see tools/bench_complex.py)
    const bool qr_first = std::max(m, n) >= 2 * r && r >= 2;
    if (m >= n) {
        if (qr_first) {
            CV<R> q = tmp_colmajor<cplx<R>>(c, m, n), rr = tmp_colmajor<cplx<R>>(c, n, n), rp = tmp_colmajor<cplx<R>>(c, n, n), ur = tmp_colmajor<cplx<R>>(c, n, n), vc = tmp_colmajor<cplx<R>>(c, n, n);
            int64_t *ind = c->alloc<int64_t>((size_t)n);
            c_pivoted_qr(c, a, q, rr, ind, n);   // a P = q rr
            c_colinv(c, rr, ind, rp);            // rr P^H: a = q (rr P^H)
            c_jacobi_svd_tall(c, rp, ur, s, vc);
            c_gemm<R>(c, 0, 0, one<R>(), q, ur, zero<R>(), u);
            copy_mat(c, vc.t(), vt, true);
        } else {
            CV<R> g = tmp_colmajor<cplx<R>>(c, m, n), uc = tmp_colmajor<cplx<R>>(c, m, n), vc = tmp_colmajor<cplx<R>>(c, n, n);
            copy_mat(c, a, g);
            c_jacobi_svd_tall(c, g, uc, s, vc);
            copy_mat(c, uc, u);
            copy_mat(c, vc.t(), vt, true);  // vt = vc^H
        }
    } else {
        // a^H = U' S V'^H  =>  a = V' S U'^H
        if (qr_first) {
            CV<R> ah = tmp_colmajor<cplx<R>>(c, n, m), q = tmp_colmajor<cplx<R>>(c, n, m), rr = tmp_colmajor<cplx<R>>(c, m, m), rp = tmp_colmajor<cplx<R>>(c, m, m), ur = tmp_colmajor<cplx<R>>(c, m, m), vc = tmp_colmajor<cplx<R>>(c, m, m);
            int64_t *ind = c->alloc<int64_t>((size_t)m);
            copy_mat(c, a.t(), ah, true);
            c_pivoted_qr(c, ah, q, rr, ind, m);  // a^H P = q rr
            c_colinv(c, rr, ind, rp);
            c_jacobi_svd_tall(c, rp, ur, s, vc); // rr P^H = ur S vc^H  =>  a^H = (q ur) S vc^H  =>  a = vc S (q ur)^H
            CV<R> qu = tmp_colmajor<cplx<R>>(c, n, m);
            c_gemm<R>(c, 0, 0, one<R>(), q, ur, zero<R>(), qu);
            copy_mat(c, vc, u);
            copy_mat(c, qu.t(), vt, true);
        } else {
            CV<R> g = tmp_colmajor<cplx<R>>(c, n, m), uc = tmp_colmajor<cplx<R>>(c, n, m), vc = tmp_colmajor<cplx<R>>(c, m, m);
            copy_mat(c, a.t(), g, true);
            c_jacobi_svd_tall(c, g, uc, s, vc);
            copy_mat(c, vc, u);
            copy_mat(c, uc.t(), vt, true);
        }
    }
}

// ------------------------------------------------------------------------------------------------ compositions
// out = in with columns gathered by the inverse permutation: out[:, i] = in[:, inv[i]]
template <typename R>
void c_colinv(rc_context *c, CV<R> in, const int64_t *ind, CV<R> out) {
    int64_t *inv = c->alloc<int64_t>((size_t)std::max<int64_t>(in.cols, 1));
    invert_perm(c, ind, in.cols, inv);
    gather_cols(c, in, inv, out);
}
// QRTraits::column_id (src/qr.rs:270-309)
template <typename R>
void c_qr_column_id(rc_context *c, CV<R> q, CV<R> r, const int64_t *ind, CV<R> cm, CV<R> z) {
    const int64_t m = q.rows, k = q.cols, n = r.cols;
    RC_REQUIRE(r.rows == k && cm.rows == m && cm.cols == k && z.rows == k && z.cols == n && k <= n, RC_INVALID_ARGUMENT, "column_id: shapes");
    if (n == 0) return;
    ArenaMark mark(c);
    CV<R> zt = tmp_colmajor<cplx<R>>(c, k, n);
    if (k == n) {
        c_gemm(c, 0, 0, one<R>(), q, r, zero<R>(), cm);
        c_fill(c, zt, true);
    } else {
        c_fill(c, zt.sub(0, k, 0, k), true);
        copy_mat(c, r.sub(0, k, k, n - k), zt.sub(0, k, k, n - k));
        CV<R> r11 = tmp_colmajor<cplx<R>>(c, k, k);
        copy_mat(c, r.sub(0, k, 0, k), r11);
        hipLaunchKernelGGL(k_c_trsm_upper<R>, dim3((unsigned)cdiv(n - k, 256)), dim3(256), 0, c->stream, r11, zt.sub(0, k, k, n - k));
        c_gemm(c, 0, 0, one<R>(), q, r11, zero<R>(), cm);
    }
    CV<R> zo = tmp_colmajor<cplx<R>>(c, k, n);
    c_colinv(c, zt, ind, zo);
    copy_mat(c, zo, z);
}
// LQTraits::row_id (src/qr.rs:363-403) = the adjoint of the column ID of (Q^H, L^H)
template <typename R>
void c_lq_row_id(rc_context *c, CV<R> l, CV<R> q, const int64_t *ind, CV<R> x, CV<R> rrows) {
    const int64_t m = l.rows, k = l.cols, n = q.cols;
    ArenaMark mark(c);
    CV<R> qh = tmp_colmajor<cplx<R>>(c, n, k), lh = tmp_colmajor<cplx<R>>(c, k, m), cp = tmp_colmajor<cplx<R>>(c, n, k), zp = tmp_colmajor<cplx<R>>(c, k, m);
    copy_mat(c, q.t(), qh, true);
    copy_mat(c, l.t(), lh, true);
    c_qr_column_id(c, qh, lh, ind, cp, zp);
    copy_mat(c, zp.t(), x, true);      // X = Z'^H   (m x k)
    copy_mat(c, cp.t(), rrows, true);  // R = C'^H   (k x n)
}
// P A = L Q: pivoted QR of A^H, conjugate-transposed back (src/pivoted_qr.rs:32-41)
template <typename R>
void c_pivoted_lq(rc_context *c, CV<R> a, CV<R> l, CV<R> q, int64_t *ind, int64_t k) {
    const int64_t m = a.rows, n = a.cols;
    ArenaMark mark(c);
    CV<R> ah = tmp_colmajor<cplx<R>>(c, n, m), qp = tmp_colmajor<cplx<R>>(c, n, k), rp = tmp_colmajor<cplx<R>>(c, k, m);
    copy_mat(c, a.t(), ah, true);
    c_pivoted_qr(c, ah, qp, rp, ind, k);
    copy_mat(c, rp.t(), l, true);
    copy_mat(c, qp.t(), q, true);
}
// ---- the input scale of rc_pivoted_qr_c*, rc_pivoted_lq_c*, rc_compute_svd_c* and the two-sided IDs: the call
// runs on 2^-e a, e the exponent of a's largest component (a device word), and R, L and s take 2^e back.  The functions above stay as
// they are for the range finders, rc_rsvd_id_c* and the column IDs by rank, which promise no input-scale domain yet.
template <typename R>
CV<R> c_normalised(rc_context *c, CV<R> a, const int *e) {
    CV<R> an = tmp_colmajor<cplx<R>>(c, a.rows, a.cols);
    copy_mat_scaled(c, a, an, e);
    return an;
}
template <typename R>
void c_pivoted_qr_scaled(rc_context *c, CV<R> a, CV<R> q, CV<R> r, int64_t *ind, int64_t k) {
    ArenaMark mark(c);
    const int *e = input_exponent(c, a);
    c_pivoted_qr(c, c_normalised(c, a, e), q, r, ind, k);
    rescale(c, r, e, 1);
}
template <typename R>
void c_pivoted_lq_scaled(rc_context *c, CV<R> a, CV<R> l, CV<R> q, int64_t *ind, int64_t k) {
    ArenaMark mark(c);
    const int *e = input_exponent(c, a);
    c_pivoted_lq(c, c_normalised(c, a, e), l, q, ind, k);
    rescale(c, l, e, 1);
}
template <typename R>
void c_compute_svd_scaled(rc_context *c, CV<R> a, CV<R> u, R *s, CV<R> vt) {
    ArenaMark mark(c);
    const int *e = input_exponent(c, a);
    c_compute_svd(c, c_normalised(c, a, e), u, s, vt);
    rescale(c, Mat<R>(s, std::min(a.rows, a.cols), 1, 1, 1), e, 1);
}
template <typename R>
void fill_gaussian(rc_context *c, CV<R> out, uint64_t seed, uint64_t offset) {
    // element (i, j): re = normal number 2 (i cols + j), im = the next one (src/random_matrix.rs:136-143), row-major order
    if (out.empty()) return;
    ArenaMark mark(c);
    cplx<R> *tmp = c->alloc<cplx<R>>((size_t)out.rows * out.cols);
    fill_gaussian<R>(c, Mat<R>(reinterpret_cast<R *>(tmp), out.rows, 2 * out.cols, 2 * out.cols, 1), seed, 2 * offset);
    copy_mat(c, CV<R>{tmp, out.rows, out.cols, out.cols, 1}, out);
}
template <typename R>
void max_col_norm_dev(rc_context *c, CV<R> y, R *out_dev) {
    ArenaMark mark(c);
    CV<R> w = tmp_colmajor<cplx<R>>(c, y.rows, y.cols);
    copy_mat(c, y, w);
    R *ss = c->alloc<R>((size_t)std::max<int64_t>(y.cols, 1));
    hipLaunchKernelGGL(k_c_col_sumsq<R>, dim3((unsigned)std::min<int64_t>(cdiv(std::max<int64_t>(y.cols, 1), 4), 8192)), dim3(256), 0, c->stream, w, ss);
    max_sqrt<R>(c, ss, y.cols, out_dev);
}

// ---- the complex family's spelling of the primitives rc_dense_shared.hpp is written in (OpView, the range finders, qr_from_range,
// rank_by_tolerance, apply_perm_matrix and their entry points stand there, once for real and complex) ----
template <typename R>
void product(rc_context *c, int alpha, bool adj_a, CV<R> a, CV<R> b, int beta, CV<R> cm) {
    c_gemm<R>(c, adj_a ? 2 : 0, 0, cplx<R>{(R)alpha, (R)0}, a, b, cplx<R>{(R)beta, (R)0}, cm);
}
template <typename R>
void qrcp(rc_context *c, CV<R> w, int64_t k, CV<R> q, CV<R> r, int64_t *ind) { c_pivoted_qr<R>(c, w, q, r, ind, k); }

}  // namespace

#include "rc_dense_shared.hpp"

namespace {

// SVDTraits::compute_from_range_estimate (src/svd.rs:171-183)
template <typename R>
void svd_from_range(rc_context *c, CV<R> range, const OpView<cplx<R>> &a, CV<R> u, R *s, CV<R> vt) {
    const int64_t rr = range.cols, n = a.cols, r = std::min(rr, n);
    RC_REQUIRE(range.rows == a.rows && u.rows == a.rows && u.cols == r && vt.rows == r && vt.cols == n, RC_INVALID_ARGUMENT, "svd_from_range_estimate: shape mismatch");
    CV<R> b = tmp_colmajor<cplx<R>>(c, rr, n), ub = tmp_colmajor<cplx<R>>(c, rr, r);
    a.project(c, range, b);
    c_compute_svd<R>(c, b, ub, s, vt);
    product(c, 1, false, range, ub, 0, u);
}

static rc_status c_svd_rank_fwd(rc_context *ctx, const double *s, int64_t len, double tol, int64_t *rank) { return rc_svd_rank_by_tolerance_f64(ctx, s, len, tol, rank); }
static rc_status c_svd_rank_fwd(rc_context *ctx, const float *s, int64_t len, double tol, int64_t *rank) { return rc_svd_rank_by_tolerance_f32(ctx, s, len, tol, rank); }

// the cfg3 pipeline for complex scalars (call sequence of rsvd_id in rc_api.hip): range -> B = Q^H A once -> SVD(B), QRCP(B), column ID
template <typename R>
void c_rsvd_id(rc_context *c, CV<R> a, int64_t k, int64_t p, CV<R> omega, uint64_t seed, const rc_rsvd_id_out &o) {
    const int64_t m = a.rows, n = a.cols;
    RC_REQUIRE(k >= 1 && k + p <= m && k <= n, RC_INVALID_ARGUMENT, "rsvd_id: need 1 <= k, k + p <= m, k <= n");
    ArenaMark mark(c);
    CV<R> range = view_of<R>(o.range_q);
    if (range.p == nullptr) range = tmp_colmajor<cplx<R>>(c, m, k);
    RC_REQUIRE(range.rows == m && range.cols == k, RC_INVALID_ARGUMENT, "rsvd_id: range_q must be m x k");
    sample_range_by_rank(c, OpView<cplx<R>>::of(a), k, p, omega, seed, range);
    CV<R> b = tmp_colmajor<cplx<R>>(c, k, n);
    c_gemm<R>(c, 2, 0, one<R>(), range, a, zero<R>(), b);
    const bool want_id = o.id_c.data || o.id_z.data || o.qr_q.data || o.qr_r.data || o.qr_ind;
    const bool want_svd = o.u.data || o.s || o.vt.data;
    if (want_svd) RC_REQUIRE(o.u.data && o.s && o.vt.data, RC_INVALID_ARGUMENT, "rsvd_id: u, s, vt must be given together");
    if (want_id) {
        CV<R> qb = tmp_colmajor<cplx<R>>(c, k, k);
        CV<R> r = o.qr_r.data ? view_of<R>(o.qr_r) : tmp_colmajor<cplx<R>>(c, k, n);
        int64_t *ind = o.qr_ind ? o.qr_ind : c->alloc<int64_t>((size_t)n);
        c_pivoted_qr<R>(c, b, qb, r, ind, k);  // works on its own copy of b
        CV<R> q = o.qr_q.data ? view_of<R>(o.qr_q) : tmp_colmajor<cplx<R>>(c, m, k);
        c_gemm<R>(c, 0, 0, one<R>(), range, qb, zero<R>(), q);
        if (o.id_c.data || o.id_z.data) {
            RC_REQUIRE(o.id_c.data && o.id_z.data, RC_INVALID_ARGUMENT, "rsvd_id: id_c and id_z must be given together");
            c_qr_column_id<R>(c, q, r, ind, view_of<R>(o.id_c), view_of<R>(o.id_z));
        }
    }
    if (want_svd) {
        CV<R> ub = tmp_colmajor<cplx<R>>(c, k, k);
        c_compute_svd<R>(c, b, ub, static_cast<R *>(o.s), view_of<R>(o.vt));
        c_gemm<R>(c, 0, 0, one<R>(), range, ub, zero<R>(), view_of<R>(o.u));
    }
}

// rank-k column IDs of `count` same-shaped complex matrices into the packed buffer (layout of rc_batch_packed_bytes with
// elem_size = sizeof(complex)); matrix i runs on context i % nctx, every context is waited for at the end
template <typename R>
void c_batch_column_id(rc_context *const *ctxs, int nctx, const rc_matrix *mats, int count, int64_t k, void *packed) {
    RC_REQUIRE(count >= 0 && k >= 1, RC_INVALID_ARGUMENT, "batch_column_id: k >= 1");
    if (count == 0) return;
    RC_REQUIRE(mats != nullptr && packed != nullptr, RC_INVALID_ARGUMENT, "batch_column_id: null argument");
    const int64_t m = mats[0].rows, n = mats[0].cols;
    RC_REQUIRE(k <= std::min(m, n), RC_INVALID_ARGUMENT, "batch_column_id: rank exceeds min(m, n)");
    // everything is checked before the first launch (no option selects between complex factorizations: the device is all the lanes must share)
    for (int i = 0; i < count; ++i)
        RC_REQUIRE(mats[i].rows == m && mats[i].cols == n && mats[i].data, RC_INVALID_ARGUMENT, "batch_column_id: all matrices must have the shape of the first");
    for (int l = 0; l < nctx; ++l) {
        RC_REQUIRE(ctxs[l] != nullptr, RC_INVALID_ARGUMENT, "batch_column_id: bad context");
        RC_REQUIRE(ctxs[l]->device == ctxs[0]->device, RC_INVALID_ARGUMENT, "batch_column_id: context %d is on device %d, context 0 on device %d", l, ctxs[l]->device,
                   ctxs[0]->device);
    }
    for (int i = 0; i < count; ++i) {
        rc_context *c = ctxs[i % nctx];
        const PackedSlot<cplx<R>> s = packed_slot<cplx<R>>(packed, i, m, n, k);  // (the permutation is written straight into the slot)
        CV<R> A = view_of<R>(mats[i]);
        c->reset_arena();
        ArenaMark mark(c);
        CV<R> q = tmp_colmajor<cplx<R>>(c, m, k), r = tmp_colmajor<cplx<R>>(c, k, n);
        c_pivoted_qr<R>(c, A, q, r, s.ind, k);
        c_qr_column_id<R>(c, q, r, s.ind, s.cm, s.z);
    }
    for (int l = 0; l < std::min(nctx, count); ++l) RC_HIP(hipStreamSynchronize(ctxs[l]->stream));
}

}  // namespace

// ================================================================================================ extern "C"
extern "C" {

#define RC_DEFINE_COMPLEX(SUF, R, CT)                                                                                                     \
    rc_status rc_random_gaussian_##SUF(rc_context *ctx, rc_matrix out, uint64_t seed, uint64_t offset) {                                  \
        return guarded(ctx, [&] { fill_gaussian<R>(ctx, view_of<R>(out), seed, offset); });                                               \
    }                                                                                                                                     \
    rc_status rc_matmat_##SUF(rc_context *ctx, rc_matrix a, rc_matrix x, rc_matrix y) {                                                   \
        return guarded(ctx, [&] { c_gemm<R>(ctx, 0, 0, one<R>(), view_of<R>(a), view_of<R>(x), zero<R>(), view_of<R>(y)); });             \
    }                                                                                                                                     \
    rc_status rc_conj_matmat_##SUF(rc_context *ctx, rc_matrix a, rc_matrix x, rc_matrix y) {                                              \
        return guarded(ctx, [&] { c_gemm<R>(ctx, 2, 0, one<R>(), view_of<R>(a), view_of<R>(x), zero<R>(), view_of<R>(y)); });             \
    }                                                                                                                                     \
    rc_status rc_gemm_##SUF(rc_context *ctx, int32_t trans_a, int32_t trans_b, CT alpha, rc_matrix a, rc_matrix b, CT beta, rc_matrix c) { \
        return guarded(ctx, [&] {                                                                                                         \
            RC_REQUIRE(trans_a >= 0 && trans_a <= 2 && trans_b >= 0 && trans_b <= 2, RC_INVALID_ARGUMENT, "gemm: op must be 0, 1 or 2");  \
            c_gemm<R>(ctx, trans_a, trans_b, cplx<R>{alpha.re, alpha.im}, view_of<R>(a), view_of<R>(b), cplx<R>{beta.re, beta.im}, view_of<R>(c)); \
        });                                                                                                                               \
    }                                                                                                                                     \
    rc_status rc_rel_diff_fro_##SUF(rc_context *ctx, rc_matrix first, rc_matrix second, R *out) {                                         \
        return guarded(ctx, [&] {                                                                                                         \
            CV<R> A = view_of<R>(first), B = view_of<R>(second);                                                                          \
            RC_REQUIRE(A.rows == B.rows && A.cols == B.cols, RC_INVALID_ARGUMENT, "rel_diff_fro: shape mismatch");                        \
            R *d = ctx->alloc<R>(2);                                                                                                      \
            hipLaunchKernelGGL(k_c_fro<R>, dim3(1), dim3(1024), 0, ctx->stream, A, B, d, input_exponent(ctx, A, B));                      \
            R h[2];                                                                                                                       \
            read_back(ctx, d, h, 2);                                                                                                      \
            *out = std::sqrt(h[0]) / std::sqrt(h[1]);                                                                                     \
        });                                                                                                                               \
    }                                                                                                                                     \
    rc_status rc_pivoted_qr_##SUF(rc_context *ctx, rc_matrix a, rc_matrix q, rc_matrix r, int64_t *ind) {                                 \
        return guarded(ctx, [&] {                                                                                                         \
            CV<R> A = view_of<R>(a), Q = view_of<R>(q), Rr = view_of<R>(r);                                                               \
            RC_REQUIRE(Q.rows == A.rows && Rr.cols == A.cols && Rr.rows == Q.cols, RC_INVALID_ARGUMENT, "pivoted_qr: output shapes");     \
            c_pivoted_qr_scaled<R>(ctx, A, Q, Rr, ind, Q.cols);                                                                           \
        });                                                                                                                               \
    }                                                                                                                                     \
    rc_status rc_geqp3_##SUF(rc_context *ctx, rc_matrix a, int64_t kmax, int64_t *jpvt, CT *tau) {                                        \
        return guarded(ctx, [&] { c_lapack_geqp3<R>(ctx, view_of<R>(a), kmax, jpvt, reinterpret_cast<cplx<R> *>(tau)); });               \
    }                                                                                                                                     \
    rc_status rc_orgqr_##SUF(rc_context *ctx, rc_matrix a, const CT *tau, int64_t k, rc_matrix q) {                                       \
        return guarded(ctx, [&] { c_lapack_ungqr<R>(ctx, view_of<R>(a), reinterpret_cast<const cplx<R> *>(tau), k, view_of<R>(q)); });   \
    }                                                                                                                                     \
    rc_status rc_trsm_upper_##SUF(rc_context *ctx, rc_matrix t, rc_matrix b) {                                                            \
        return guarded(ctx, [&] {                                                                                                         \
            CV<R> tt = view_of<R>(t), bb = view_of<R>(b);                                                                                 \
            RC_REQUIRE(tt.rows == tt.cols && tt.rows == bb.rows, RC_INVALID_ARGUMENT, "trsm_upper: t must be k x k, b k x nrhs");        \
            if (bb.empty()) return;                                                                                                       \
            hipLaunchKernelGGL(k_c_trsm_upper<R>, dim3((unsigned)cdiv(bb.cols, 256)), dim3(256), 0, ctx->stream, tt, bb);                \
        });                                                                                                                               \
    }                                                                                                                                     \
    rc_status rc_pivoted_lq_##SUF(rc_context *ctx, rc_matrix a, rc_matrix l, rc_matrix q, int64_t *ind) {                                 \
        return guarded(ctx, [&] {                                                                                                         \
            CV<R> A = view_of<R>(a), L = view_of<R>(l), Q = view_of<R>(q);                                                                \
            RC_REQUIRE(L.rows == A.rows && Q.cols == A.cols && Q.rows == L.cols, RC_INVALID_ARGUMENT, "pivoted_lq: output shapes");       \
            c_pivoted_lq_scaled<R>(ctx, A, L, Q, ind, L.cols);                                                                            \
        });                                                                                                                               \
    }                                                                                                                                     \
    rc_status rc_compute_svd_##SUF(rc_context *ctx, rc_matrix a, rc_matrix u, R *s, rc_matrix vt) {                                       \
        return guarded(ctx, [&] { c_compute_svd_scaled<R>(ctx, view_of<R>(a), view_of<R>(u), s, view_of<R>(vt)); });                      \
    }                                                                                                                                     \
    rc_status rc_qr_to_mat_##SUF(rc_context *ctx, rc_matrix q, rc_matrix r, const int64_t *ind, rc_matrix out) {                          \
        return guarded(ctx, [&] {                                                                                                         \
            CV<R> Rr = view_of<R>(r);                                                                                                     \
            CV<R> rp = tmp_colmajor<cplx<R>>(ctx, Rr.rows, Rr.cols);                                                                      \
            c_colinv<R>(ctx, Rr, ind, rp);                                                                                                \
            c_gemm<R>(ctx, 0, 0, one<R>(), view_of<R>(q), rp, zero<R>(), view_of<R>(out));                                                \
        });                                                                                                                               \
    }                                                                                                                                     \
    rc_status rc_lq_to_mat_##SUF(rc_context *ctx, rc_matrix l, rc_matrix q, const int64_t *ind, rc_matrix out) {                          \
        return guarded(ctx, [&] {                                                                                                         \
            CV<R> L = view_of<R>(l);                                                                                                      \
            CV<R> lp = tmp_colmajor<cplx<R>>(ctx, L.rows, L.cols);                                                                        \
            c_colinv<R>(ctx, L.t(), ind, lp.t());                                                                                         \
            c_gemm<R>(ctx, 0, 0, one<R>(), lp, view_of<R>(q), zero<R>(), view_of<R>(out));                                                \
        });                                                                                                                               \
    }                                                                                                                                     \
    rc_status rc_qr_column_id_##SUF(rc_context *ctx, rc_matrix q, rc_matrix r, const int64_t *ind, rc_matrix c, rc_matrix z) {            \
        return guarded(ctx, [&] { c_qr_column_id<R>(ctx, view_of<R>(q), view_of<R>(r), ind, view_of<R>(c), view_of<R>(z)); });            \
    }                                                                                                                                     \
    rc_status rc_lq_row_id_##SUF(rc_context *ctx, rc_matrix l, rc_matrix q, const int64_t *ind, rc_matrix x, rc_matrix rr) {              \
        return guarded(ctx, [&] { c_lq_row_id<R>(ctx, view_of<R>(l), view_of<R>(q), ind, view_of<R>(x), view_of<R>(rr)); });              \
    }                                                                                                                                     \
    rc_status rc_svd_to_mat_##SUF(rc_context *ctx, rc_matrix u, const R *s, rc_matrix vt, rc_matrix out) {                                \
        return guarded(ctx, [&] {                                                                                                         \
            CV<R> VT = view_of<R>(vt);                                                                                                    \
            CV<R> sv = tmp_colmajor<cplx<R>>(ctx, VT.rows, VT.cols);                                                                      \
            copy_mat<R>(ctx, VT, sv);                                                                                                     \
            if (!sv.empty()) hipLaunchKernelGGL(k_c_scale_rows<R>, dim3((unsigned)std::min<int64_t>(cdiv(sv.rows * sv.cols, 256), 8192)), dim3(256), 0, ctx->stream, s, sv); \
            c_gemm<R>(ctx, 0, 0, one<R>(), view_of<R>(u), sv, zero<R>(), view_of<R>(out));                                                \
        });                                                                                                                               \
    }                                                                                                                                     \
    rc_status rc_svd_to_qr_##SUF(rc_context *ctx, rc_matrix u, const R *s, rc_matrix vt, rc_matrix q, rc_matrix r, int64_t *ind) {        \
        return guarded(ctx, [&] {                                                                                                         \
            CV<R> VT = view_of<R>(vt), Q = view_of<R>(q);                                                                                 \
            const int64_t k = Q.cols;                                                                                                     \
            RC_REQUIRE(k <= std::min(VT.rows, VT.cols), RC_INVALID_ARGUMENT, "svd_to_qr: rank exceeds min(r, n)");                        \
            CV<R> w = tmp_colmajor<cplx<R>>(ctx, VT.rows, VT.cols), qb = tmp_colmajor<cplx<R>>(ctx, VT.rows, k);                          \
            copy_mat<R>(ctx, VT, w);                                                                                                      \
            if (!w.empty()) hipLaunchKernelGGL(k_c_scale_rows<R>, dim3((unsigned)std::min<int64_t>(cdiv(w.rows * w.cols, 256), 8192)), dim3(256), 0, ctx->stream, s, w); \
            c_pivoted_qr<R>(ctx, w, qb, view_of<R>(r), ind, k);                                                                           \
            c_gemm<R>(ctx, 0, 0, one<R>(), view_of<R>(u), qb, zero<R>(), Q);                                                              \
        });                                                                                                                               \
    }                                                                                                                                     \
    rc_status rc_column_id_two_sided_##SUF(rc_context *ctx, rc_matrix c, rc_matrix c_out, rc_matrix x, int64_t *row_ind) {                \
        return guarded(ctx, [&] {                                                                                                         \
            CV<R> C = view_of<R>(c);                                                                                                      \
            const int64_t m = C.rows, k = C.cols, kk = std::min(m, k);                                                                    \
            CV<R> l = tmp_colmajor<cplx<R>>(ctx, m, kk), ql = tmp_colmajor<cplx<R>>(ctx, kk, k);                                          \
            c_pivoted_lq_scaled<R>(ctx, C, l, ql, row_ind, kk); /* LQ::compute_from, qr.rs:354-362 */                                     \
            c_lq_row_id<R>(ctx, l, ql, row_ind, view_of<R>(c_out), view_of<R>(x));                                                        \
        });                                                                                                                               \
    }                                                                                                                                     \
    rc_status rc_row_id_two_sided_##SUF(rc_context *ctx, rc_matrix r, rc_matrix x, rc_matrix r_out, int64_t *col_ind) {                   \
        return guarded(ctx, [&] {                                                                                                         \
            CV<R> Rr = view_of<R>(r);                                                                                                     \
            const int64_t k = Rr.rows, n = Rr.cols, kk = std::min(k, n);                                                                  \
            CV<R> q = tmp_colmajor<cplx<R>>(ctx, k, kk), rr = tmp_colmajor<cplx<R>>(ctx, kk, n);                                          \
            c_pivoted_qr_scaled<R>(ctx, Rr, q, rr, col_ind, kk);                                                                          \
            c_qr_column_id<R>(ctx, q, rr, col_ind, view_of<R>(x), view_of<R>(r_out));                                                     \
        });                                                                                                                               \
    }                                                                                                                                     \
    rc_status rc_column_id_rank_##SUF(rc_context *ctx, rc_matrix a, int64_t k, rc_matrix c, rc_matrix z, int64_t *col_ind) {              \
        return guarded(ctx, [&] {                                                                                                         \
            CV<R> A = view_of<R>(a);                                                                                                      \
            const int64_t kk = std::min(k, std::min(A.rows, A.cols));                                                                     \
            CV<R> q = tmp_colmajor<cplx<R>>(ctx, A.rows, kk), r = tmp_colmajor<cplx<R>>(ctx, kk, A.cols);                                 \
            c_pivoted_qr<R>(ctx, A, q, r, col_ind, kk);                                                                                   \
            c_qr_column_id<R>(ctx, q, r, col_ind, view_of<R>(c), view_of<R>(z));                                                          \
        });                                                                                                                               \
    }                                                                                                                                     \
    /* singular values are real for every scalar type (src/svd.rs:86-101) */                                                              \
    rc_status rc_svd_rank_by_tolerance_##SUF(rc_context *ctx, const R *s, int64_t len, double tol, int64_t *rank) {                        \
        return c_svd_rank_fwd(ctx, s, len, tol, rank);                                                                                    \
    }                                                                                                                                     \
    /* the fused rSVD + ID call (same members, same "null = skipped" rule as rc_rsvd_id_f64); B = Q^H A is formed once */                \
    rc_status rc_rsvd_id_##SUF(rc_context *ctx, rc_matrix a, int64_t k, int64_t p, rc_matrix omega, uint64_t seed, const rc_rsvd_id_out *out) { \
        if (!out) return RC_INVALID_ARGUMENT;                                                                                             \
        return guarded(ctx, [&] { c_rsvd_id<R>(ctx, view_of<R>(a), k, p, view_of<R>(omega), seed, *out); });                              \
    }                                                                                                                                     \
    /* cfg5's batch for complex matrices: the same packed layout, one rank-k column ID per matrix, round-robin over the contexts */      \
    rc_status rc_batch_column_id_##SUF(rc_context *const *ctxs, int32_t nctx, const rc_matrix *mats, int32_t count, int64_t k, void *packed) { \
        if (!ctxs || nctx < 1 || !ctxs[0]) return RC_INVALID_ARGUMENT;                                                                    \
        return guarded(ctxs[0], [&] { c_batch_column_id<R>(ctxs, nctx, mats, count, k, packed); });                                       \
    }

RC_DEFINE_COMPLEX(c64, double, rc_complex64)
RC_DEFINE_COMPLEX(c32, float, rc_complex32)
RC_DEFINE_DENSE_SHARED(c64, cplx<double>, double)
RC_DEFINE_DENSE_SHARED(c32, cplx<float>, float)

}  // extern "C"
