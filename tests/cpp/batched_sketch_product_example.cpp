// The batched sketch product and the randomized SVD of wide blocks through the C++ mirror include/rusty_compression.hpp:
// sketch_product_batched on a stack of Gaussian blocks against the host product; for blocks of at most 512 columns its bits against the
// sketch that range_step_batched writes; range_step_large_batched (q orthonormal on full-rank blocks; p = a q^T and a = p q on blocks of
// rank r < l) and svd_rank_large_batched at rank r on those blocks, which the chain reproduces to rounding.  Prints one "name value" line per check and exits non-zero when
// one fails; the CPU suite only compiles and links it.
#include <cmath>
#include <cstdio>
#include <cstring>
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

// out (rows x cols) = x (rows x inner) y (inner x cols), C order, per block of a stack of `count`; x shared by the blocks when xshared,
// y read as the transpose of a stack of cols x inner blocks when ytrans; d (count x inner) scales the inner index when not empty
template <typename T>
static std::vector<T> stacked_product(const std::vector<T> &x, bool xshared, const std::vector<T> &d, const std::vector<T> &y, bool ytrans, int32_t count,
                                      int64_t rows, int64_t inner, int64_t cols) {
    std::vector<T> out((std::size_t)(count * rows * cols));
    for (int32_t i = 0; i < count; ++i)
        for (int64_t a = 0; a < rows; ++a)
            for (int64_t b = 0; b < cols; ++b) {
                double acc = 0;
                for (int64_t j = 0; j < inner; ++j) {
                    const double xv = (double)x[(std::size_t)(((xshared ? 0 : i) * rows + a) * inner + j)];
                    const double yv = ytrans ? (double)y[(std::size_t)((i * cols + b) * inner + j)] : (double)y[(std::size_t)((i * inner + j) * cols + b)];
                    acc += xv * (d.empty() ? 1.0 : (double)d[(std::size_t)(i * inner + j)]) * yv;
                }
                out[(std::size_t)((i * rows + a) * cols + b)] = (T)acc;
            }
    return out;
}

// max |q q^T - I| over the blocks of a stack of l x n matrices
template <typename T>
static double row_gram_defect(const std::vector<T> &q, int32_t count, int64_t l, int64_t n) {
    double worst = 0;
    for (int32_t i = 0; i < count; ++i)
        for (int64_t a = 0; a < l; ++a)
            for (int64_t b = 0; b <= a; ++b) {
                double acc = 0;
                for (int64_t j = 0; j < n; ++j) acc += (double)q[(std::size_t)((i * l + a) * n + j)] * (double)q[(std::size_t)((i * l + b) * n + j)];
                worst = std::fmax(worst, std::fabs(acc - (a == b ? 1.0 : 0.0)));
            }
    return worst;
}

template <typename T>
static double differing(const std::vector<T> &x, const std::vector<T> &y) {
    return x.size() == y.size() && std::memcmp(x.data(), y.data(), x.size() * sizeof(T)) == 0 ? 0.0 : 1.0;
}

template <typename T>
static void check(const char *tag, int32_t count, int64_t m, int64_t n, int64_t l, int64_t r, double bound, uint64_t seed) {
    Context ctx(0);
    std::printf("%s:\n", tag);
    // blocks of exact rank r: a_i = b_i c_i, multiplied out on the host
    const auto hb = random_gaussian<T>(ctx, count * m, r, seed).to_host(), hc = random_gaussian<T>(ctx, count * r, n, seed + 1).to_host();
    const auto ha = stacked_product(hb, false, std::vector<T>(), hc, false, count, m, r, n);
    const auto a = DeviceMatrix<T>::from_host(ctx, ha.data(), count * m, n);
    const auto omega = random_gaussian<T>(ctx, l, m, seed + 2);
    const auto y = sketch_product_batched(a, omega, count);
    expect("  omega a (host product)", rel(y.to_host(), stacked_product(omega.to_host(), true, std::vector<T>(), ha, false, count, l, m, n)), bound);
    if (n <= 512) {
        DeviceMatrix<T> sketch(ctx, 1, 1);
        range_step_batched(a, omega, count, &sketch);
        ctx.synchronize();
        expect("  bits of range_step_batched's sketch", differing(y.to_host(), sketch.to_host()), 0);
    }
    // on full-rank blocks the step keeps all l rows of q, orthonormal
    const auto full = random_gaussian<T>(ctx, count * m, n, seed + 3);
    const auto fstep = range_step_large_batched(full, omega, count);
    double bad = 0;
    for (int64_t v : fstep.ranks.to_host()) bad += v != l;
    expect("  ranks of the step (full-rank blocks)", bad, 0);
    expect("  q q^T - I", row_gram_defect(fstep.q.to_host(), count, l, n), bound);
    // on the blocks of rank r < l (the sketch has l - r singular values at rounding level): p = a q^T and a = p q
    const auto step = range_step_large_batched(a, omega, count);
    const auto hq = step.q.to_host(), hp = step.p.to_host();
    expect("  p = a q^T (host product)", rel(hp, stacked_product(ha, false, std::vector<T>(), hq, true, count, m, n, l)), bound);
    expect("  p q (the blocks)", rel(stacked_product(hp, false, std::vector<T>(), hq, false, count, m, l, n), ha), bound);
    for (int steps = 1; steps <= 2; ++steps) {
        const auto svd = svd_rank_large_batched(a, omega, count, r, 0.0, steps);
        bad = 0;
        for (int64_t v : svd.ranks.to_host()) bad += v != r;
        expect("  ranks of the SVD", bad, 0);
        // s is count x l; the first r columns of u and rows of vt carry the block
        const auto hs = svd.s.to_host();
        std::vector<T> sr((std::size_t)(count * r));
        for (int32_t i = 0; i < count; ++i)
            for (int64_t j = 0; j < r; ++j) sr[(std::size_t)(i * r + j)] = hs[(std::size_t)(i * l + j)];
        expect("  u diag(s) vt (the blocks)", rel(stacked_product(svd.u.to_host(), false, sr, svd.vt.to_host(), false, count, m, r, n), ha), bound);
    }
}

int main() {
    int rc = 0;
    try {
        check<double>("sketch product and large SVD<double>, wide", 2, 300, 700, 24, 9, 1e-11, 91);
        check<double>("sketch product and large SVD<double>, delegating (n <= 512)", 2, 700, 300, 24, 9, 1e-11, 92);
        check<float>("sketch product and large SVD<float>, wide", 2, 260, 600, 20, 7, 2e-3, 93);
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
