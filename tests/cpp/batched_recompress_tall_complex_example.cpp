// The batched recompression of tall complex factor pairs through the C++ mirror include/rusty_compression.hpp: recompress_tall_batched on
// the output of the sketched column_id_rank_batched for c64 and c32 (the randomized SVD of a stack of tall exactly low-rank complex blocks
// in two launches), checked on the host against the blocks themselves: the new ranks are the exact ranks, U diag(s) Vt (Vt = V^H, nothing
// else conjugated), multiplied out on the host, reproduces A, and the singular values come back in the real type.  For blocks of at most
// 512 rows the result is compared with recompress_batched's bit for bit.  Prints one "name value" line per check and exits non-zero when
// one fails; the CPU suite only compiles and links it.
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

// how many bytes of two host arrays differ (0: the same bits)
template <typename T>
static double differing(const std::vector<T> &x, const std::vector<T> &y) {
    return x.size() == y.size() && std::memcmp(x.data(), y.data(), x.size() * sizeof(T)) == 0 ? 0.0 : 1.0;
}

template <typename T>
static void check(const char *tag, int32_t count, int64_t m, int64_t n, double bound, double tol, uint64_t seed) {
    using Real = typename Scalar<T>::real;
    Context ctx(0);
    const int64_t r = 5, k = 12, l = 20;
    const auto hx = random_gaussian<T>(ctx, count * m, r, seed).to_host(), hy = random_gaussian<T>(ctx, count * r, n, seed + 1).to_host();
    const auto ha = stacked_product(hx, std::vector<Real>(), 0, hy, count, m, r, n);
    const auto a = DeviceMatrix<T>::from_host(ctx, ha.data(), count * m, n);
    const auto omega = random_gaussian<T>(ctx, l, m, seed + 2);
    std::printf("%s:\n", tag);
    const auto id = column_id_rank_batched<T>(a, omega, count, k, tol);
    const auto svd = recompress_tall_batched(id, k, tol);
    static_assert(std::is_same<decltype(svd.s), DeviceBuffer<Real>>::value, "singular values in the real type");
    double bad = 0;
    for (int64_t v : svd.ranks.to_host()) bad += v != r;
    expect("  ranks", bad, 0);
    expect("  u diag(s) vt (host product)", rel(stacked_product(svd.u.to_host(), svd.s.to_host(), k, svd.vt.to_host(), count, m, k, n), ha), bound);
    if (m <= 512) {
        const auto ref = recompress_batched(id, k, tol);
        expect("  bits of recompress_batched", differing(svd.u.to_host(), ref.u.to_host()) + differing(svd.s.to_host(), ref.s.to_host()) +
                                                   differing(svd.vt.to_host(), ref.vt.to_host()), 0);
    }
}

int main() {
    int rc = 0;
    try {
        check<c64>("recompress_tall_batched<c64>", 3, 3000, 40, 1e-10, 1e-9, 81);
        check<c64>("recompress_tall_batched<c64>, one stage", 4, 400, 30, 1e-10, 1e-9, 82);
        check<c32>("recompress_tall_batched<c32>", 3, 1300, 40, 1e-3, 1e-4, 83);
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
