// The batched recompression through the C++ mirror include/rusty_compression.hpp: recompress_batched on the outputs of
// column_id_rank_batched and two_sided_id_rank_batched (an ID turned into an SVD) and on two batched SVDs (rounded addition) for a
// stack of small exactly low-rank matrices, checked on the host against the matrices themselves: U diag(s) Vt, rebuilt by
// to_mat_batched, reproduces A (or A + B), and the new ranks are the exact ranks.  Prints one "name value" line per check and exits
// non-zero when one fails; the CPU suite only compiles and links it.
#include <cmath>
#include <cstdio>
#include <unistd.h>

#include "rusty_compression.hpp"

using namespace rusty_compression;

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
        num += (double)(x[i] - ref[i]) * (double)(x[i] - ref[i]);
        den += (double)ref[i] * (double)ref[i];
    }
    return std::sqrt(num / den);
}

// how many of the ranks differ from `want`
static double wrong_ranks(const DeviceIndex &ranks, int64_t want) {
    double bad = 0;
    for (int64_t r : ranks.to_host()) bad += r != want;
    return bad;
}

// count stacked m x n blocks of exact rank r: block i is x_i y_i with Gaussian x_i (m x r) and y_i (r x n)
template <typename T>
static DeviceMatrix<T> low_rank_stack(const Context &ctx, int32_t count, int64_t m, int64_t n, int64_t r, uint64_t seed) {
    const auto hx = random_gaussian<T>(ctx, count * m, r, seed).to_host(), hy = random_gaussian<T>(ctx, count * r, n, seed + 1).to_host();
    std::vector<T> h((std::size_t)(count * m * n));
    for (int32_t i = 0; i < count; ++i)
        for (int64_t a = 0; a < m; ++a)
            for (int64_t b = 0; b < n; ++b) {
                T acc = 0;
                for (int64_t j = 0; j < r; ++j) acc += hx[(std::size_t)((i * m + a) * r + j)] * hy[(std::size_t)((i * r + j) * n + b)];
                h[(std::size_t)((i * m + a) * n + b)] = acc;
            }
    return DeviceMatrix<T>::from_host(ctx, h.data(), count * m, n);
}

template <typename T>
static void check(const char *tag, int32_t count, int64_t m, int64_t n, double bound, double tol, uint64_t seed) {
    Context ctx(0);
    const int64_t r = 5, k = 12;
    const auto a = low_rank_stack<T>(ctx, count, m, n, r, seed), b = low_rank_stack<T>(ctx, count, m, n, r, seed + 7);
    const auto ha = a.to_host(), hb = b.to_host();
    std::vector<T> hsum(ha.size());
    for (std::size_t i = 0; i < ha.size(); ++i) hsum[i] = ha[i] + hb[i];
    std::printf("%s:\n", tag);
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
        check<double>("recompress_batched<double>", 5, 40, 30, 1e-10, 1e-9, 51);
        check<float>("recompress_batched<float>", 4, 30, 40, 1e-3, 1e-4, 52);
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
