// The batched recompression of complex factor pairs with both factors tall through the C++ mirror include/rusty_compression.hpp:
// recompress_large_batched's c64 / c32 overloads on a stack of Gaussian factor pairs left (m x K), right (K x n) of blocks large on both
// sides, checked on the host against the blocks themselves: the new ranks are K, U diag(s) Vt (Vt = V^H, nothing else conjugated) multiplied
// out on the host reproduces left right, U and Vt have orthonormal columns / rows, and the singular values come back in the real type.  For
// blocks of at most 512 columns the result is compared with recompress_tall_batched's bit for bit.  Prints one "name value" line per check
// and exits non-zero when one fails; the CPU suite only compiles and links it.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <type_traits>
#include <unistd.h>

#include "rusty_compression.hpp"

using namespace rusty_compression;
using zd = std::complex<double>;

static int failures = 0;
static void expect(const char *name, double value, double bound) {
    std::printf("%s %.3e (bound %.1e)%s\n", name, value, bound, value <= bound ? "" : "  FAILED");
    if (!(value <= bound)) ++failures;
}

// relative Frobenius distance of two host arrays
template <typename T>
static double rel(const std::vector<T> &x, const std::vector<T> &ref) {
    double num = 0, den = 0;
    for (std::size_t i = 0; i < ref.size(); ++i) {
        num += std::norm(zd(x[i]) - zd(ref[i]));
        den += std::norm(zd(ref[i]));
    }
    return std::sqrt(num / den);
}

// out (rows x cols) = x (rows x inner) diag(d) y (inner x cols), C order, per block of a stack of `count`, nothing conjugated; d (count x
// dstride, real) or empty
template <typename T, typename Real>
static std::vector<T> stacked_product(const std::vector<T> &x, const std::vector<Real> &d, int64_t dstride, const std::vector<T> &y, int32_t count,
                                      int64_t rows, int64_t inner, int64_t cols) {
    std::vector<T> out((std::size_t)(count * rows * cols));
    for (int32_t i = 0; i < count; ++i)
        for (int64_t a = 0; a < rows; ++a)
            for (int64_t b = 0; b < cols; ++b) {
                zd acc = 0;
                for (int64_t j = 0; j < inner; ++j)
                    acc += zd(x[(std::size_t)((i * rows + a) * inner + j)]) * (d.empty() ? 1.0 : (double)d[(std::size_t)(i * dstride + j)]) *
                           zd(y[(std::size_t)((i * inner + j) * cols + b)]);
                out[(std::size_t)((i * rows + a) * cols + b)] = T(acc);
            }
    return out;
}

// max |x^H x - I| over the blocks of a stack of rows x cols matrices (transposed: x x^H of cols x rows blocks stored as rows of length `rows`)
template <typename T>
static double gram_defect(const std::vector<T> &x, int32_t count, int64_t rows, int64_t cols, bool transposed) {
    double worst = 0;
    for (int32_t i = 0; i < count; ++i)
        for (int64_t a = 0; a < cols; ++a)
            for (int64_t b = 0; b <= a; ++b) {
                zd acc = 0;
                for (int64_t j = 0; j < rows; ++j) {
                    const std::size_t base = (std::size_t)i * (std::size_t)(rows * cols);
                    const zd xa = transposed ? zd(x[base + (std::size_t)(a * rows + j)]) : zd(x[base + (std::size_t)(j * cols + a)]);
                    const zd xb = transposed ? zd(x[base + (std::size_t)(b * rows + j)]) : zd(x[base + (std::size_t)(j * cols + b)]);
                    acc += std::conj(xa) * xb;
                }
                worst = std::fmax(worst, std::abs(acc - (a == b ? 1.0 : 0.0)));
            }
    return worst;
}

// how many of two host arrays differ (0: the same bits)
template <typename T>
static double differing(const std::vector<T> &x, const std::vector<T> &y) {
    return x.size() == y.size() && std::memcmp(x.data(), y.data(), x.size() * sizeof(T)) == 0 ? 0.0 : 1.0;
}

template <typename T>
static void check(const char *tag, int32_t count, int64_t m, int64_t n, int64_t K, double bound, uint64_t seed) {
    using Real = typename Scalar<T>::real;
    Context ctx(0);
    const auto left = random_gaussian<T>(ctx, count * m, K, seed), right = random_gaussian<T>(ctx, count * K, n, seed + 1);
    const auto ha = stacked_product(left.to_host(), std::vector<Real>(), 0, right.to_host(), count, m, K, n);
    std::printf("%s:\n", tag);
    const auto svd = recompress_large_batched(left, nullptr, nullptr, right, nullptr, count, K);
    static_assert(std::is_same<decltype(svd.s), DeviceBuffer<Real>>::value, "singular values in the real type");
    double bad = 0;
    for (int64_t v : svd.ranks.to_host()) bad += v != K;
    expect("  ranks", bad, 0);
    expect("  u diag(s) vt (host product)", rel(stacked_product(svd.u.to_host(), svd.s.to_host(), K, svd.vt.to_host(), count, m, K, n), ha), bound);
    expect("  u^H u - I", gram_defect(svd.u.to_host(), count, m, K, false), bound);
    expect("  vt vt^H - I", gram_defect(svd.vt.to_host(), count, n, K, true), bound);
    if (n <= 512) {
        const auto ref = recompress_tall_batched<T>(left, nullptr, nullptr, right, nullptr, count, K);
        expect("  bits of recompress_tall_batched", differing(svd.u.to_host(), ref.u.to_host()) + differing(svd.s.to_host(), ref.s.to_host()) +
                                                        differing(svd.vt.to_host(), ref.vt.to_host()), 0);
    }
}

int main() {
    int rc = 0;
    try {
        check<c64>("recompress_large_batched<c64>", 2, 1300, 1100, 12, 1e-12, 81);
        check<c64>("recompress_large_batched<c64>, short left factor", 2, 40, 1500, 9, 1e-12, 82);
        check<c64>("recompress_large_batched<c64>, one stage on the right", 3, 900, 300, 12, 1e-12, 83);
        check<c32>("recompress_large_batched<c32>", 2, 700, 1300, 12, 1e-4, 84);
    } catch (const std::exception &e) {
        std::printf("exception: %s\n", e.what());
        rc = 2;
    }
    if (rc == 0) {
        std::printf(failures ? "FAILED %d\n" : "ALL OK\n", failures);
        rc = failures ? 1 : 0;
    }
    // every context has been destroyed; leave without running the HIP runtime's exit-time teardown (as mirror_examples.cpp)
    std::fflush(stdout);
    _exit(rc);
}
