// The batched complex truncated SVD through the C++ mirror include/rusty_compression.hpp: svd_rank_batched<c64> (tall) and <c32>
// (wide) on a stack of small Gaussian matrices, checked on the host against its contract (real descending singular values,
// orthonormal kept columns of U, the phase rule, U S Vt reproducing A at full rank).  Prints one "name value" line per check and
// exits non-zero when one fails; the CPU suite only compiles and links it.
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

template <typename T>
static void check(const char *tag, int32_t count, int64_t m, int64_t n, double eps, uint64_t seed) {
    using Real = typename Scalar<T>::real;
    Context ctx(0);
    const int64_t p = m < n ? m : n, k = p;  // full rank: U S Vt reproduces A to the rounding level
    auto a = random_gaussian<T>(ctx, count * m, n, seed);  // matrix i is rows i m .. (i + 1) m - 1
    auto svd = svd_rank_batched<T>(a, count, k);
    auto ha = a.to_host();
    auto hu = svd.u.to_host(), hvt = svd.vt.to_host();
    auto hs = svd.s.to_host();
    auto hr = svd.ranks.to_host();
    double order = 0, orth = 0, phase = 0, num = 0, den = 0;
    for (int32_t b = 0; b < count; ++b) {
        const T *ab = ha.data() + b * m * n, *ub = hu.data() + b * m * k, *vb = hvt.data() + b * k * n;
        const Real *sb = hs.data() + b * p;
        if (hr[b] != k) { std::printf("%s rank %lld != %lld FAILED\n", tag, (long long)hr[b], (long long)k); ++failures; }
        for (int64_t j = 1; j < p; ++j) order = std::max(order, (double)(sb[j] - sb[j - 1]));
        for (int64_t c = 0; c < k; ++c) {
            int64_t imax = 0;
            for (int64_t i = 0; i < m; ++i)
                if (std::norm(ub[i * k + c]) > std::norm(ub[imax * k + c])) imax = i;
            const T top = ub[imax * k + c];
            if (top.imag() != 0 || !(top.real() > 0)) phase = 1;  // the phase rule: the largest entry is exactly real and positive
            for (int64_t c2 = 0; c2 < k; ++c2) {
                std::complex<double> d = 0;
                for (int64_t i = 0; i < m; ++i) d += std::conj(std::complex<double>(ub[i * k + c])) * std::complex<double>(ub[i * k + c2]);
                orth = std::max(orth, std::abs(d - std::complex<double>(c == c2 ? 1.0 : 0.0)));
            }
        }
        for (int64_t i = 0; i < m; ++i)
            for (int64_t j = 0; j < n; ++j) {
                std::complex<double> s = 0;
                for (int64_t l = 0; l < k; ++l) s += std::complex<double>(ub[i * k + l]) * (double)sb[l] * std::complex<double>(vb[l * n + j]);
                num += std::norm(std::complex<double>(ab[i * n + j]) - s);
                den += std::norm(std::complex<double>(ab[i * n + j]));
            }
    }
    std::printf("%s:\n", tag);
    expect("  s_ascending_steps", order, 0.0);
    expect("  u_orthonormal", orth, 100 * eps);
    expect("  largest_entry_not_real_positive", phase, 0.0);
    expect("  u_s_vt_reconstruction", std::sqrt(num / den), 100 * eps);
}

int main() {
    int rc = 0;
    try {
        check<c64>("svd_rank_batched<c64>", 5, 40, 24, 1.1e-16, 41);
        check<c32>("svd_rank_batched<c32>", 5, 24, 40, 6e-8, 42);
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
