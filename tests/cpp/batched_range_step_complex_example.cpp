// The complex batched range step and the power-iterated sketched column ID through the C++ mirror include/rusty_compression.hpp:
// range_step_batched<c64 / c32> on a stack of tall complex blocks with a shared complex Gaussian omega, and column_id_rank_power_batched on
// exactly low-rank blocks.  Checked on the host against the blocks themselves: the kept rows of q satisfy q q^H = I and the rest are zero,
// p = a q^H, conj_p hands back exactly conj(p), the sketch handed back is omega a (nothing conjugated), (a q^H) q reproduces a low-rank a,
// and the power-iterated ID finds the exact ranks and reproduces a; with no iterations it is the one-pass call bit for bit.  Prints one
// "name value" line per check and exits non-zero when one fails; the CPU suite only compiles and links it.
#include <cmath>
#include <complex>
#include <cstdio>
#include <unistd.h>

#include "rusty_compression.hpp"

using namespace rusty_compression;
using z128 = std::complex<double>;

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
        num += std::norm((z128)x[i] - (z128)ref[i]);
        den += std::norm((z128)ref[i]);
    }
    return std::sqrt(num / den);
}

// out (rows x cols) = x (rows x inner) y (inner x cols), C order, per block of a stack of `count`; hy: y's block is cols x inner and y^H is used
template <typename T>
static std::vector<T> stacked_product(const std::vector<T> &x, const std::vector<T> &y, int32_t count, int64_t rows, int64_t inner, int64_t cols,
                                      bool shared_x = false, bool hy = false) {
    std::vector<T> out((std::size_t)(count * rows * cols));
    for (int32_t i = 0; i < count; ++i)
        for (int64_t a = 0; a < rows; ++a)
            for (int64_t b = 0; b < cols; ++b) {
                z128 acc = 0;
                for (int64_t j = 0; j < inner; ++j)
                    acc += (z128)x[(std::size_t)(((shared_x ? 0 : i) * rows + a) * inner + j)] *
                           (hy ? std::conj((z128)y[(std::size_t)((i * cols + b) * inner + j)]) : (z128)y[(std::size_t)((i * inner + j) * cols + b)]);
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
    const auto step = range_step_batched<T>(a, omega, count, &sketch);
    const auto hq = step.q.to_host(), hp = step.p.to_host();
    const auto ranks = step.ranks.to_host();
    double bad = 0, orth = 0, tail = 0;
    for (int32_t i = 0; i < count; ++i) {
        const int64_t ri = ranks[(std::size_t)i];
        bad += ri < r || ri > l;
        for (int64_t x = 0; x < l; ++x)
            for (int64_t y = 0; y < l; ++y) {
                z128 dot = 0;
                for (int64_t j = 0; j < n; ++j) dot += (z128)hq[(std::size_t)((i * l + x) * n + j)] * std::conj((z128)hq[(std::size_t)((i * l + y) * n + j)]);
                if (x < ri && y < ri) orth = std::fmax(orth, std::abs(dot - (x == y ? 1.0 : 0.0)));
                else tail = std::fmax(tail, std::abs(dot));
            }
    }
    expect("  ranks in [r, l]", bad, 0);
    expect("  q q^H = I on the kept rows", orth, bound);
    expect("  rows of q past the rank are zero", tail, 0);
    expect("  sketch = omega a", rel(sketch.to_host(), stacked_product(omega.to_host(), ha, count, l, m, n, true)), bound);
    expect("  p = a q^H", rel(hp, stacked_product(ha, hq, count, m, n, l, false, true)), bound);
    expect("  p q = a", rel(stacked_product(hp, hq, count, m, l, n), ha), bound);
    const auto hpc = range_step_batched<T>(a, omega, count, nullptr, true).p.to_host();
    double differ = 0;
    for (std::size_t i = 0; i < hp.size(); ++i) differ += !(hpc[i].real() == hp[i].real() && hpc[i].imag() == -hp[i].imag());
    expect("  conj_p gives conj(p) exactly", differ, 0);

    const auto id0 = column_id_rank_power_batched<T>(a, omega, count, k, tol, 0), one = column_id_rank_batched<T>(a, omega, count, k, tol);
    expect("  no iterations = the one-pass call", (double)(id0.z.to_host() != one.z.to_host()) + (double)(id0.col_ind.to_host() != one.col_ind.to_host()), 0);
    for (int iterations = 1; iterations <= 2; ++iterations) {
        const auto id = column_id_rank_power_batched<T>(a, omega, count, k, tol, iterations);
        bad = 0;
        for (int64_t v : id.ranks.to_host()) bad += v != r;
        std::printf("  iterations = %d\n", iterations);
        expect("    ranks", bad, 0);
        expect("    c z (host product)", rel(stacked_product(id.c.to_host(), id.z.to_host(), count, m, k, n), ha), bound);
    }
}

int main() {
    int rc = 0;
    try {
        check<c64>("range_step_batched<c64>", 4, 400, 30, 1e-10, 1e-9, 81);
        check<c64>("range_step_batched<c64>, tall", 2, 3000, 40, 1e-10, 1e-9, 82);
        check<c32>("range_step_batched<c32>", 3, 300, 40, 1e-3, 1e-4, 83);
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
