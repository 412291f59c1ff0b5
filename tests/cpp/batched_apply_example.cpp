// The batched apply / to_mat through the C++ mirror include/rusty_compression.hpp: apply_batched and to_mat_batched on the outputs of
// column_id_rank_batched, two_sided_id_rank_batched and svd_rank_batched for a stack of small Gaussian matrices at full rank, checked
// on the host against the matrices themselves (to_mat reproduces A, apply reproduces A b).  Prints one "name value" line per check
// and exits non-zero when one fails; the CPU suite only compiles and links it.
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
        num += std::norm(x[i] - ref[i]);
        den += std::norm(ref[i]);
    }
    return std::sqrt(num / den);
}

template <typename T>
static void check(const char *tag, int32_t count, int64_t m, int64_t n, int64_t nrhs, double bound, uint64_t seed) {
    Context ctx(0);
    const int64_t k = m < n ? m : n;  // full rank: the factors reproduce A to the rounding level
    auto a = random_gaussian<T>(ctx, count * m, n, seed);        // block i is rows i m .. (i + 1) m - 1
    auto b = random_gaussian<T>(ctx, count * n, nrhs, seed + 1);  // block i is rows i n .. (i + 1) n - 1
    const auto ha = a.to_host(), hb = b.to_host();
    std::vector<T> hab((std::size_t)(count * m * nrhs));
    for (int32_t i = 0; i < count; ++i)
        for (int64_t r = 0; r < m; ++r)
            for (int64_t c = 0; c < nrhs; ++c) {
                T acc = 0;
                for (int64_t j = 0; j < n; ++j) acc += ha[(std::size_t)((i * m + r) * n + j)] * hb[(std::size_t)((i * n + j) * nrhs + c)];
                hab[(std::size_t)((i * m + r) * nrhs + c)] = acc;
            }
    std::printf("%s:\n", tag);
    const auto cid = column_id_rank_batched<T>(a, count, k);
    expect("  column_id to_mat", rel(to_mat_batched(cid).to_host(), ha), bound);
    expect("  column_id apply", rel(apply_batched(cid, b).to_host(), hab), bound);
    const auto ts = two_sided_id_rank_batched<T>(a, count, k);
    expect("  two_sided_id to_mat", rel(to_mat_batched(ts).to_host(), ha), bound);
    expect("  two_sided_id apply", rel(apply_batched(ts, b).to_host(), hab), bound);
    const auto svd = svd_rank_batched<T>(a, count, k);
    expect("  svd to_mat", rel(to_mat_batched(svd).to_host(), ha), bound);
    expect("  svd apply", rel(apply_batched(svd, b).to_host(), hab), bound);
}

int main() {
    int rc = 0;
    try {
        check<double>("apply_batched<double>", 5, 40, 24, 3, 1e-10, 41);
        check<float>("apply_batched<float>", 5, 24, 40, 1, 1e-3, 42);
        check<c64>("apply_batched<c64>", 3, 30, 20, 9, 1e-10, 43);
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
