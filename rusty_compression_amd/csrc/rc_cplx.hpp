// The complex element of every complex kernel (rc_complex.hip, kernels_batched_id_c.hip, batched_apply.hpp and the two kernels built
// on it, kernels_batched_residual_c.hip) and the strided complex view of an rc_matrix.  Complex data is interleaved (re, im) -- the
// layout of ndarray's Complex<T> / numpy complex -- and aligned as its real type, so a view may start at any element of a caller's array.
#pragma once
#include "rc_common.hpp"

namespace rc {

namespace {

template <typename R>
struct cplx {
    R re, im;
};
template <typename R> __host__ __device__ __forceinline__ cplx<R> mk(R a, R b) { return cplx<R>{a, b}; }
template <typename R> __host__ __device__ __forceinline__ cplx<R> czero() { return {(R)0, (R)0}; }
template <typename R> __host__ __device__ __forceinline__ cplx<R> cone() { return {(R)1, (R)0}; }
template <typename R> __host__ __device__ __forceinline__ cplx<R> operator+(cplx<R> a, cplx<R> b) { return {a.re + b.re, a.im + b.im}; }
template <typename R> __host__ __device__ __forceinline__ cplx<R> operator-(cplx<R> a, cplx<R> b) { return {a.re - b.re, a.im - b.im}; }
template <typename R> __host__ __device__ __forceinline__ cplx<R> operator*(cplx<R> a, cplx<R> b) { return {a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re}; }
template <typename R> __host__ __device__ __forceinline__ cplx<R> operator*(R s, cplx<R> a) { return {s * a.re, s * a.im}; }
template <typename R> __host__ __device__ __forceinline__ cplx<R> cj(cplx<R> a) { return {a.re, -a.im}; }
template <typename R> __host__ __device__ __forceinline__ R abs2(cplx<R> a) { return a.re * a.re + a.im * a.im; }
template <typename R> __device__ __forceinline__ R cabs(cplx<R> a) { return hypot(a.re, a.im); }
template <typename R> __device__ __forceinline__ cplx<R> cdiv(cplx<R> a, cplx<R> b) {  // Smith's algorithm (?ladiv)
    if (fabs(b.re) >= fabs(b.im)) {
        const R r = b.im / b.re, d = b.re + b.im * r;
        return {(a.re + a.im * r) / d, (a.im - a.re * r) / d};
    }
    const R r = b.re / b.im, d = b.im + b.re * r;
    return {(a.re * r + a.im) / d, (a.im * r - a.re) / d};
}
// acc += a b as four FMAs: re by a.re b.re then -a.im b.im, im by a.re b.im then a.im b.re
template <typename R> __device__ __forceinline__ void cfma(cplx<R> a, cplx<R> b, cplx<R> &acc) {
    acc.re = fma(a.re, b.re, acc.re);
    acc.re = fma(-a.im, b.im, acc.re);
    acc.im = fma(a.re, b.im, acc.im);
    acc.im = fma(a.im, b.re, acc.im);
}

// strided complex view (mirror of rc_matrix, strides in complex elements)
template <typename R>
struct CV {
    cplx<R> *p;
    int64_t rows, cols, rs, cs;
    __host__ __device__ cplx<R> &at(int64_t i, int64_t j) const { return p[i * rs + j * cs]; }
    CV sub(int64_t r0, int64_t nr, int64_t c0, int64_t nc) const { return CV{p + r0 * rs + c0 * cs, nr, nc, rs, cs}; }
    CV t() const { return CV{p, cols, rows, cs, rs}; }
    bool empty() const { return rows == 0 || cols == 0; }
};
template <typename R>
CV<R> view_of(const rc_matrix &m) { return CV<R>{static_cast<cplx<R> *>(m.data), m.rows, m.cols, m.row_stride, m.col_stride}; }

}  // namespace

}  // namespace rc
