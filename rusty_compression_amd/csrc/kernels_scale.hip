// Input-scale normalisation of the dense entry points: the exponent e of the largest finite magnitude of a
// matrix, left in device memory; the working copy written times 2^-e; R, L and s multiplied by 2^e where they are delivered.  Every
// factor is an exact power of two, so the kernels below the entry points see the same bits for 2^t A as for A.  gfx950 only.
#include "rc_batched.hpp"
#include "rc_cplx.hpp"

namespace rc {

namespace {

// the magnitude's bit pattern: ordered as the magnitudes on finite values, inf and NaN above every finite one
__device__ __forceinline__ unsigned long long mag_bits(double v) { return (unsigned long long)__double_as_longlong(v) & 0x7fffffffffffffffull; }
__device__ __forceinline__ unsigned long long mag_bits(float v) { return (unsigned long long)(__float_as_uint(v) & 0x7fffffffu); }
template <typename R> __device__ __forceinline__ unsigned long long mag_bits(cplx<R> v) { return max(mag_bits(v.re), mag_bits(v.im)); }

__device__ __forceinline__ double pow2_times(double v, int e) { return ldexp(v, e); }
__device__ __forceinline__ float pow2_times(float v, int e) { return ldexpf(v, e); }
template <typename R> __device__ __forceinline__ cplx<R> pow2_times(cplx<R> v, int e) { return {pow2_times(v.re, e), pow2_times(v.im, e)}; }

// partial[block] = the largest mag_bits of the block's share of a (deterministic two-stage maximum, as fro_diff's sums)
template <typename E>
__global__ __launch_bounds__(256) void k_mag_partial(Mat<E> a, unsigned long long *partial) {
    __shared__ unsigned long long sh[256];
    const bool col_fast = (a.cs <= a.rs);
    const int64_t total = a.rows * a.cols;
    unsigned long long mx = 0;
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
        int64_t i, j;
        if (col_fast) { i = e / a.cols; j = e - i * a.cols; }
        else { j = e / a.rows; i = e - j * a.rows; }
        mx = max(mx, mag_bits(a.at(i, j)));
    }
    sh[threadIdx.x] = mx;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) sh[threadIdx.x] = max(sh[threadIdx.x], sh[threadIdx.x + s]);
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[blockIdx.x] = sh[0];
}
// e = ilogb of the largest magnitude, clamped to the normal exponents; 0 for a zero matrix and for one with an inf or a NaN (the rule
// of block_pow2_exponent, rc_device.hpp)
template <typename R>
__global__ __launch_bounds__(256) void k_mag_exponent(const unsigned long long *partial, int n, int *e_out) {
    __shared__ unsigned long long sh[256];
    unsigned long long mx = 0;
    for (int i = threadIdx.x; i < n; i += 256) mx = max(mx, partial[i]);
    sh[threadIdx.x] = mx;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) sh[threadIdx.x] = max(sh[threadIdx.x], sh[threadIdx.x + s]);
        __syncthreads();
    }
    if (threadIdx.x != 0) return;
    R v;
    if (sizeof(R) == 8) v = (R)__longlong_as_double((long long)sh[0]);
    else v = (R)__uint_as_float((unsigned)sh[0]);
    int e = 0;
    if (v != (R)0 && v < (R)INFINITY) {
        constexpr int lim = sizeof(R) == 8 ? 1022 : 126;
        e = ilogb(v);
        e = e < -lim ? -lim : (e > lim ? lim : e);
    }
    *e_out = e;
}

// k_copy_tiled (kernels_util.hip) with the stored value times 2^-e
template <typename E>
__global__ __launch_bounds__(256) void k_copy_tiled_scaled(Mat<E> src, Mat<E> dst, const int *e) {
    __shared__ E tile[32][33];
    const int down = -*e;
    const int64_t tr = (int64_t)blockIdx.y * 32, tc = (int64_t)blockIdx.x * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
    const bool src_col_fast = (src.cs <= src.rs);
    for (int y = ty; y < 32; y += 8) {
        int64_t i = src_col_fast ? tr + y : tr + tx;
        int64_t j = src_col_fast ? tc + tx : tc + y;
        if (i < src.rows && j < src.cols) {
            if (src_col_fast) tile[y][tx] = src.at(i, j);
            else tile[tx][y] = src.at(i, j);
        }
    }
    __syncthreads();
    const bool dst_col_fast = (dst.cs <= dst.rs);
    for (int y = ty; y < 32; y += 8) {
        int64_t i = dst_col_fast ? tr + y : tr + tx;
        int64_t j = dst_col_fast ? tc + tx : tc + y;
        if (i < dst.rows && j < dst.cols) dst.at(i, j) = pow2_times(dst_col_fast ? tile[y][tx] : tile[tx][y], down);
    }
}

// x(i, j) *= 2^(sign e), except below the diagonal of the first refl_k columns (the reflectors of a ?geqp3 result carry no scale)
template <typename E>
__global__ __launch_bounds__(256) void k_rescale(Mat<E> x, const int *e, int sign, int64_t refl_k) {
    const int by = sign * *e;
    if (by == 0) return;
    const bool col_fast = (x.cs <= x.rs);
    const int64_t total = x.rows * x.cols;
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        int64_t i, j;
        if (col_fast) { i = t / x.cols; j = t - i * x.cols; }
        else { j = t / x.rows; i = t - j * x.rows; }
        if (j < refl_k && i > j) continue;
        x.at(i, j) = pow2_times(x.at(i, j), by);
    }
}

template <typename E>
int mag_grid(Mat<E> a) { return (int)std::max<int64_t>(1, std::min<int64_t>(rc::cdiv(a.rows * a.cols, 256 * 8), 1024)); }

}  // namespace

template <typename E>
int *input_exponent(rc_context *c, Mat<E> a, Mat<E> b) {
    using R = real_t<E>;
    int *e = c->alloc<int>(1);
    ArenaMark mark(c);  // (e stays: it was taken before the mark)
    const int ga = mag_grid(a), gb = b.p ? mag_grid(b) : 0;
    unsigned long long *partial = c->alloc<unsigned long long>((size_t)(ga + gb));
    hipLaunchKernelGGL(k_mag_partial<E>, dim3(ga), dim3(256), 0, c->stream, a, partial);
    if (gb) hipLaunchKernelGGL(k_mag_partial<E>, dim3(gb), dim3(256), 0, c->stream, b, partial + ga);
    hipLaunchKernelGGL(k_mag_exponent<R>, dim3(1), dim3(256), 0, c->stream, partial, ga + gb, e);
    return e;
}

template <typename E>
void copy_mat_scaled(rc_context *c, Mat<E> src, Mat<E> dst, const int *e) {
    RC_REQUIRE(src.rows == dst.rows && src.cols == dst.cols, RC_INVALID_ARGUMENT, "copy_mat_scaled: shape mismatch (%lld x %lld) vs (%lld x %lld)",
               (long long)src.rows, (long long)src.cols, (long long)dst.rows, (long long)dst.cols);
    if (src.empty()) return;
    dim3 grid((unsigned)rc::cdiv(src.cols, 32), (unsigned)rc::cdiv(src.rows, 32));
    hipLaunchKernelGGL(k_copy_tiled_scaled<E>, grid, dim3(256), 0, c->stream, src, dst, e);
}

template <typename E>
void rescale(rc_context *c, Mat<E> x, const int *e, int sign, int64_t refl_k) {
    if (x.empty()) return;
    int grid = (int)std::min<int64_t>(rc::cdiv(x.rows * x.cols, 256), 8192);
    hipLaunchKernelGGL(k_rescale<E>, dim3(grid), dim3(256), 0, c->stream, x, e, sign, refl_k);
}

#define RC_INST(E)                                                                    \
    template int *input_exponent<E>(rc_context *, Mat<E>, Mat<E>);                    \
    template void copy_mat_scaled<E>(rc_context *, Mat<E>, Mat<E>, const int *);      \
    template void rescale<E>(rc_context *, Mat<E>, const int *, int, int64_t);
RC_INST(double)
RC_INST(float)
RC_INST(cplx<double>)
RC_INST(cplx<float>)
#undef RC_INST

}  // namespace rc
