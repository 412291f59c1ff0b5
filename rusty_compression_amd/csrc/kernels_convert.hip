// Strided batched conversion between the compute type and the storage type of the mixed calls (rc_demote_batched_f64 / _c64: f64 -> f32,
// c64 -> c32; rc_promote_batched_f32 / _c32: the way back): what a host needs to keep the factors of rc_lowrank_apply_mixed_batched_* and
// rc_block_operator_apply_mixed_* in half the bytes.
//
// Elementwise, any row, column and batch strides on either side.  Demotion is static_cast<float>: IEEE round-to-nearest-even, subnormal
// results and the overflow of a finite value to +-inf included (the bits of NumPy's astype(float32)); promotion is exact.  A complex
// element converts componentwise.
//
// MI355X mapping.  The path is a copy: blockIdx.y walks the blocks, blockIdx.x the elements of one block in a grid-stride loop (32-bit
// indices when the block allows) with the lanes along whichever index of the source view has the smaller stride, so the wide side of a demotion is read in full lines.  The
// overflow count of a block (finite source elements whose image is not finite) is an integer: lanes count their own, a wave adds its lanes
// by shuffles and issues at most one atomic add, onto a word the launcher zeroed on the stream, so the value does not depend on the order.
#include <algorithm>

#include "rc_cplx.hpp"

namespace rc {

namespace {

constexpr int CV_THREADS = 256;

__device__ __forceinline__ float cv_to(float, double v) { return static_cast<float>(v); }
__device__ __forceinline__ double cv_to(double, float v) { return static_cast<double>(v); }
template <typename D, typename R>
__device__ __forceinline__ cplx<D> cv_to(cplx<D>, cplx<R> v) { return {cv_to(D(), v.re), cv_to(D(), v.im)}; }
template <typename R>
__device__ __forceinline__ bool cv_finite(R v) { return __builtin_isfinite(v); }
template <typename R>
__device__ __forceinline__ bool cv_finite(cplx<R> v) { return __builtin_isfinite(v.re) && __builtin_isfinite(v.im); }

template <typename Src, typename Dst>
struct CvArgs {
    const Src *src;
    Dst *dst;
    int64_t srs, scs, sbs, drs, dcs, dbs;
    int64_t rows, cols;
    int count;
    unsigned long long *overflow;  // nullptr: not counted
};

template <typename Src, typename Dst, bool COUNT>
__global__ __launch_bounds__(CV_THREADS) void k_convert_batched(CvArgs<Src, Dst> a) {
    const int64_t total = a.rows * a.cols;
    const bool cols_fast = a.scs <= a.srs;
    const int64_t fast = cols_fast ? a.cols : a.rows;
    for (int blk = blockIdx.y; blk < a.count; blk += gridDim.y) {
        const Src *sp = a.src + (int64_t)blk * a.sbs;
        Dst *dp = a.dst + (int64_t)blk * a.dbs;
        int bad = 0;
        // the element index in 32 bits whenever the block has fewer than 2^31 elements (every factor batch): one 32-bit division per
        // element instead of a 64-bit one
        auto walk = [&](auto first, auto step, auto count_, auto fast_) {
            for (auto idx = first; idx < count_; idx += step) {
                const auto f = idx % fast_, o = idx / fast_;
                const int64_t i = cols_fast ? o : f, j = cols_fast ? f : o;
                const Src v = sp[i * a.srs + j * a.scs];
                const Dst w = cv_to(Dst(), v);
                dp[i * a.drs + j * a.dcs] = w;
                if constexpr (COUNT) bad += (cv_finite(v) && !cv_finite(w)) ? 1 : 0;
            }
        };
        if (total < ((int64_t)1 << 31) - (int64_t)gridDim.x * CV_THREADS)
            walk((uint32_t)(blockIdx.x * CV_THREADS + threadIdx.x), (uint32_t)(gridDim.x * CV_THREADS), (uint32_t)total, (uint32_t)fast);
        else
            walk((int64_t)blockIdx.x * CV_THREADS + threadIdx.x, (int64_t)gridDim.x * CV_THREADS, total, fast);
        if constexpr (COUNT) {
            if (a.overflow) {
#pragma unroll
                for (int off = 32; off >= 1; off >>= 1) bad += __shfl_xor(bad, off, 64);
                if ((threadIdx.x & 63) == 0 && bad) atomicAdd(a.overflow + blk, (unsigned long long)bad);
            }
        }
    }
}

template <typename Src, typename Dst, bool COUNT>
void convert_launch(rc_context *c, const char *label, const rc_matrix &src, int64_t sbs, int32_t count, const rc_matrix &dst, int64_t dbs, int64_t *overflow) {
    if (overflow) RC_HIP(hipMemsetAsync(overflow, 0, (size_t)count * sizeof(int64_t), c->stream));
    CvArgs<Src, Dst> a;
    a.src = static_cast<const Src *>(src.data); a.dst = static_cast<Dst *>(dst.data);
    a.srs = src.row_stride; a.scs = src.col_stride; a.sbs = sbs;
    a.drs = dst.row_stride; a.dcs = dst.col_stride; a.dbs = dbs;
    a.rows = src.rows; a.cols = src.cols; a.count = count;
    a.overflow = reinterpret_cast<unsigned long long *>(overflow);
    // 8 elements per thread along x, at most 4096 workgroups; along y as many blocks side by side as bring the grid to about 4096
    // workgroups (small factor blocks are a handful of workgroups each), at least 64, never more than count
    const int64_t total = src.rows * src.cols;
    const int64_t gx = std::min<int64_t>((total + CV_THREADS * 8 - 1) / (CV_THREADS * 8), 4096);
    const int gy = (int)std::min<int64_t>(count, std::max<int64_t>(64, 4096 / gx));
    ProfScope ps(c, "op:%s %lldx%lld count=%d grid=%lldx%d", label, (long long)src.rows, (long long)src.cols, (int)count, (long long)gx, gy);
    hipLaunchKernelGGL((k_convert_batched<Src, Dst, COUNT>), dim3((unsigned)gx, (unsigned)gy), dim3(CV_THREADS), 0, c->stream, a);
    RC_HIP(hipGetLastError());
}

}  // namespace

void batched_demote(rc_context *c, bool complex_data, const rc_matrix &src, int64_t sbs, int32_t count, const rc_matrix &dst, int64_t dbs, int64_t *overflow) {
    if (complex_data) convert_launch<cplx<double>, cplx<float>, true>(c, "demote_batched<complex>", src, sbs, count, dst, dbs, overflow);
    else convert_launch<double, float, true>(c, "demote_batched", src, sbs, count, dst, dbs, overflow);
}

void batched_promote(rc_context *c, bool complex_data, const rc_matrix &src, int64_t sbs, int32_t count, const rc_matrix &dst, int64_t dbs) {
    if (complex_data) convert_launch<cplx<float>, cplx<double>, false>(c, "promote_batched<complex>", src, sbs, count, dst, dbs, nullptr);
    else convert_launch<float, double, false>(c, "promote_batched", src, sbs, count, dst, dbs, nullptr);
}

}  // namespace rc
