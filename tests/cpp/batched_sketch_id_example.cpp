// The batched sketched column ID through the C++ mirror include/rusty_compression.hpp: the column_id_rank_batched overload that takes a
// test matrix omega, on a stack of tall exactly low-rank blocks with a Gaussian omega.  Checked on the host against the blocks
// themselves: the ranks are the exact ranks, C Z reproduces A (by to_mat_batched where the batched apply accepts the block, m <= 512,
// and by a host product for taller blocks), recompress_batched takes the result, and the sketch handed back is omega A.  Prints one
// "name value" line per check and exits non-zero when one fails; the CPU suite only compiles and links it.
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

// out (rows x cols) = x (rows x inner) y (inner x cols), C order, per block of a stack of `count`
template <typename T>
static std::vector<T> stacked_product(const std::vector<T> &x, const std::vector<T> &y, int32_t count, int64_t rows, int64_t inner, int64_t cols,
                                      bool shared_x = false) {
    std::vector<T> out((std::size_t)(count * rows * cols));
    for (int32_t i = 0; i < count; ++i)
        for (int64_t a = 0; a < rows; ++a)
            for (int64_t b = 0; b < cols; ++b) {
                double acc = 0;
                for (int64_t j = 0; j < inner; ++j)
                    acc += (double)x[(std::size_t)(((shared_x ? 0 : i) * rows + a) * inner + j)] * (double)y[(std::size_t)((i * inner + j) * cols + b)];
                out[(std::size_t)((i * rows + a) * cols + b)] = (T)acc;
            }
    return out;
}

template <typename T>
static void check(const char *tag, int32_t count, int64_t m, int64_t n, double bound, double tol, uint64_t seed) {
    Context ctx(0);
    const int64_t r = 5, k = 12, l = 20;
    const auto hx = random_gaussian<T>(ctx, count * m, r, seed).to_host(), hy = random_gaussian<T>(ctx, count * r, n, seed + 1).to_host();
    const auto ha = stacked_product(hx, hy, count, m, r, n);
    const auto a = DeviceMatrix<T>::from_host(ctx, ha.data(), count * m, n);
    const auto omega = random_gaussian<T>(ctx, l, m, seed + 2);
    std::printf("%s:\n", tag);
    DeviceMatrix<T> sketch;
    const auto id = column_id_rank_batched<T>(a, omega, count, k, tol, &sketch);
    double bad = 0;
    for (int64_t v : id.ranks.to_host()) bad += v != r;
    expect("  ranks", bad, 0);
    expect("  sketch = omega a", rel(sketch.to_host(), stacked_product(omega.to_host(), ha, count, l, m, n, true)), bound);
    expect("  c z (host product)", rel(stacked_product(id.c.to_host(), id.z.to_host(), count, m, k, n), ha), bound);
    if (m <= 512) {
        expect("  to_mat_batched", rel(to_mat_batched(id).to_host(), ha), bound);
        const auto svd = recompress_batched(id, k, tol);
        expect("  recompress_batched", rel(to_mat_batched(svd).to_host(), ha), bound);
    }
}

int main() {
    int rc = 0;
    try {
        check<double>("sketched column_id_rank_batched<double>", 4, 400, 30, 1e-10, 1e-9, 61);
        check<double>("sketched column_id_rank_batched<double>, tall", 2, 3000, 40, 1e-10, 1e-9, 62);
        check<float>("sketched column_id_rank_batched<float>", 3, 300, 40, 1e-3, 1e-4, 63);
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
