// The complex element of every complex kernel (rc_complex.hip, kernels_batched_id_c.hip, batched_stages.hpp, batched_apply.hpp and the
// two kernels built on it, kernels_batched_residual_c.hip), which rc_batched.hpp declares for the launchers' signatures, and the strided complex
// view of an rc_matrix.  Complex data is interleaved (re, im) -- the
// layout of ndarray's Complex<T> / numpy complex -- and aligned as its real type, so a view may start at any element of a caller's array.
#pragma once
#include "rc_common.hpp"
#include "rc_device.hpp"

namespace rc {

// one type in every translation unit (rc_batched.hpp declares it), so that Mat<cplx<R>> crosses them; its operations stay internal to each
template <typename R>
struct cplx {
    R re, im;
};

namespace {

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

// The complex side of the element operations the shared batched stages are written in (batched_stages.hpp, where the real side and the
// primary elem<E> stand): zero and one, division (Smith's), the larger pow2_key of the two parts, scaling by a real, and the back
// substitution's acc -= a b in the complex kernels' spelling.  abs2 and cj above are shared as they are; the real type is real_t<E>
// (rc_batched.hpp).
template <typename E> struct elem;
template <typename R>
struct elem<cplx<R>> {
    static __host__ __device__ __forceinline__ cplx<R> zero() { return czero<R>(); }
    static __host__ __device__ __forceinline__ cplx<R> one() { return cone<R>(); }
};
template <typename R> __device__ __forceinline__ cplx<R> ediv(cplx<R> a, cplx<R> b) { return cdiv(a, b); }
template <typename R> __device__ __forceinline__ R pow2_key_max(cplx<R> v) { return max(pow2_key(v.re), pow2_key(v.im)); }
template <typename R> __device__ __forceinline__ cplx<R> escale(cplx<R> v, R s) { return {v.re * s, v.im * s}; }
template <typename R> __device__ __forceinline__ void submul(cplx<R> &acc, cplx<R> a, cplx<R> b) { acc = acc - a * b; }

// strided complex view: Mat over the complex element
template <typename R>
using CV = Mat<cplx<R>>;
template <typename R>
CV<R> view_of(const rc_matrix &m) { return CV<R>(static_cast<cplx<R> *>(m.data), m.rows, m.cols, m.row_stride, m.col_stride); }

}  // namespace

}  // namespace rc
