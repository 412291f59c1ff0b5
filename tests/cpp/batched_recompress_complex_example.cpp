// The batched recompression of complex factors through the C++ mirror include/rusty_compression.hpp: recompress_batched on raw factors
// (left, mid, the real s, right), on the outputs of column_id_rank_batched and two_sided_id_rank_batched (an ID turned into an SVD) and
// on two batched SVDs (rounded addition) for c64 and c32, on stacks of small exactly low-rank complex blocks, checked on the host
// against the blocks themselves: U diag(s) Vt (Vt = V^H, nothing else conjugated), rebuilt by to_mat_batched, reproduces A (or A + B),
// the new ranks are the exact ranks, and the singular values come back in the real type.  Prints one "name value" line per check and
// exits non-zero when one fails; the CPU suite only compiles and links it.
#include <cmath>
#include <cstdio>
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

// how many of the ranks differ from `want`
static double wrong_ranks(const DeviceIndex &ranks, int64_t want) {
    double bad = 0;
    for (int64_t r : ranks.to_host()) bad += r != want;
    return bad;
}

// the stacked products x_i y_i of count blocks (x: count * m x r, y: count * r x n), nothing conjugated
template <typename T>
static std::vector<T> stacked_product(const std::vector<T> &hx, const std::vector<T> &hy, int32_t count, int64_t m, int64_t n, int64_t r) {
    std::vector<T> h((std::size_t)(count * m * n));
    for (int32_t i = 0; i < count; ++i)
        for (int64_t a = 0; a < m; ++a)
            for (int64_t b = 0; b < n; ++b) {
                zd acc = 0;
                for (int64_t j = 0; j < r; ++j) acc += zd(hx[(std::size_t)((i * m + a) * r + j)]) * zd(hy[(std::size_t)((i * r + j) * n + b)]);
                h[(std::size_t)((i * m + a) * n + b)] = T(acc);
            }
    return h;
}

template <typename T>
static void check(const char *tag, int32_t count, int64_t m, int64_t n, double bound, double tol, uint64_t seed) {
    using Real = typename Scalar<T>::real;
    Context ctx(0);
    const int64_t r = 5, k = 12;
    const auto x = random_gaussian<T>(ctx, count * m, r, seed), y = random_gaussian<T>(ctx, count * r, n, seed + 1);
    const auto x2 = random_gaussian<T>(ctx, count * m, r, seed + 7), y2 = random_gaussian<T>(ctx, count * r, n, seed + 8);
    const auto ha = stacked_product(x.to_host(), y.to_host(), count, m, n, r), hb = stacked_product(x2.to_host(), y2.to_host(), count, m, n, r);
    const auto a = DeviceMatrix<T>::from_host(ctx, ha.data(), count * m, n), b = DeviceMatrix<T>::from_host(ctx, hb.data(), count * m, n);
    std::vector<T> hsum(ha.size());
    for (std::size_t i = 0; i < ha.size(); ++i) hsum[i] = ha[i] + hb[i];
    std::printf("%s:\n", tag);
    // the raw factors x_i diag(1) y_i with a real scale vector of ones
    std::vector<Real> ones((std::size_t)(count * r), (Real)1);
    DeviceBuffer<Real> s(ctx, ones.size());
    s.from_host(ones.data());
    const auto raw = recompress_batched<T>(x, nullptr, &s, y, nullptr, count, k, tol);
    static_assert(std::is_same<decltype(raw.s), DeviceBuffer<Real>>::value, "singular values in the real type");
    expect("  raw factors -> svd", rel(to_mat_batched(raw).to_host(), ha), bound);
    expect("  raw factors -> svd ranks", wrong_ranks(raw.ranks, r), 0);
    const auto cid = recompress_batched(column_id_rank_batched<T>(a, count, k, tol), k, tol);
    expect("  column_id -> svd", rel(to_mat_batched(cid).to_host(), ha), bound);
    expect("  column_id -> svd ranks", wrong_ranks(cid.ranks, r), 0);
    const auto ts = recompress_batched(two_sided_id_rank_batched<T>(a, count, k, tol), k, tol);
    expect("  two_sided_id -> svd", rel(to_mat_batched(ts).to_host(), ha), bound);
    expect("  two_sided_id -> svd ranks", wrong_ranks(ts.ranks, r), 0);
    const auto sum = recompress_batched(svd_rank_batched<T>(a, count, k, tol), svd_rank_batched<T>(b, count, k, tol), 2 * k, tol);
    expect("  svd + svd", rel(to_mat_batched(sum).to_host(), hsum), bound);
    expect("  svd + svd ranks", wrong_ranks(sum.ranks, 2 * r), 0);
}

int main() {
    int rc = 0;
    try {
        check<c64>("recompress_batched<c64>", 5, 40, 30, 1e-10, 1e-9, 61);
        check<c32>("recompress_batched<c32>", 4, 30, 40, 1e-3, 1e-4, 62);
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
