// The batched sketched column ID of complex tall blocks through the C++ mirror include/rusty_compression.hpp, for c64 and c32: the
// column_id_rank_batched overload that takes a test matrix omega, on stacks of 1500 x 64 and of 400 x 64 exactly low-rank complex blocks
// with a complex Gaussian omega, then residual_batched on its result and, where the recompression accepts the factors (m <= 512),
// recompress_batched.  Checked on the host in complex double: the ranks are the
// exact ranks, the sketch handed back is omega a (nothing conjugated), residual_batched's err is the Frobenius norm of a - c z formed from
// the factors the call returned (to the complex residual example's bounds, 1e-10 and 1e-4) and small against a, and the recompressed u diag(s) vt
// reproduces a.  Prints one "name value" line per check and exits non-zero when one fails; the CPU suite only compiles and links it.
#include <cmath>
#include <cstdio>
#include <unistd.h>

#include "rusty_compression.hpp"

using namespace rusty_compression;
using zd = std::complex<double>;

static int failures = 0;
static void expect(const char *name, double value, double bound) {
    std::printf("%s %.3e (bound %.1e)%s\n", name, value, bound, value <= bound ? "" : "  FAILED");
    if (!(value <= bound)) ++failures;
}

// out (rows x cols) = x (rows x inner) y (inner x cols) in complex double, C order, per block of a stack of `count`
template <typename X, typename Y>
static std::vector<zd> stacked_product(const std::vector<X> &x, const std::vector<Y> &y, int32_t count, int64_t rows, int64_t inner, int64_t cols,
                                       bool shared_x = false) {
    std::vector<zd> out((std::size_t)(count * rows * cols));
    for (int32_t i = 0; i < count; ++i)
        for (int64_t a = 0; a < rows; ++a)
            for (int64_t b = 0; b < cols; ++b) {
                zd acc = 0;
                for (int64_t j = 0; j < inner; ++j)
                    acc += zd(x[(std::size_t)(((shared_x ? 0 : i) * rows + a) * inner + j)]) * zd(y[(std::size_t)((i * inner + j) * cols + b)]);
                out[(std::size_t)((i * rows + a) * cols + b)] = acc;
            }
    return out;
}

// relative Frobenius distance of a device result from a host stack
template <typename T>
static double rel(const std::vector<T> &x, const std::vector<zd> &ref) {
    double num = 0, den = 0;
    for (std::size_t i = 0; i < ref.size(); ++i) {
        num += std::norm(zd(x[i]) - ref[i]);
        den += std::norm(ref[i]);
    }
    return std::sqrt(num / den);
}

template <typename T>
static void check(const char *tag, int32_t count, int64_t m, double bound, double res_bound, double tol, uint64_t seed) {
    using Real = typename Scalar<T>::real;
    Context ctx(0);
    const int64_t n = 64, r = 5, k = 12, l = 20;
    const auto hx = random_gaussian<T>(ctx, count * m, r, seed).to_host(), hy = random_gaussian<T>(ctx, count * r, n, seed + 1).to_host();
    const auto had = stacked_product(hx, hy, count, m, r, n);
    std::vector<T> ha(had.size());
    for (std::size_t i = 0; i < had.size(); ++i) ha[i] = T((Real)had[i].real(), (Real)had[i].imag());
    const std::vector<zd> ref(ha.begin(), ha.end());  // the blocks as the device holds them
    const auto a = DeviceMatrix<T>::from_host(ctx, ha.data(), count * m, n);
    const auto omega = random_gaussian<T>(ctx, l, m, seed + 2);
    std::printf("%s:\n", tag);
    DeviceMatrix<T> sketch;
    const auto id = column_id_rank_batched<T>(a, omega, count, k, tol, &sketch);
    const auto ranks = id.ranks.to_host();
    double bad = 0;
    for (int64_t v : ranks) bad += v != r;
    expect("  ranks", bad, 0);
    expect("  sketch = omega a", rel(sketch.to_host(), stacked_product(omega.to_host(), ha, count, l, m, n, true)), bound);
    const auto cz = stacked_product(id.c.to_host(), id.z.to_host(), count, m, k, n);
    const auto res = residual_batched(id, a);
    const auto err = res.err.to_host(), nrm = res.nrm.to_host();
    double gap = 0, worst = 0;
    for (int32_t b = 0; b < count; ++b) {
        double e2 = 0, a2 = 0;
        for (int64_t i = 0; i < m * n; ++i) {
            e2 += std::norm(ref[(std::size_t)(b * m * n + i)] - cz[(std::size_t)(b * m * n + i)]);
            a2 += std::norm(ref[(std::size_t)(b * m * n + i)]);
        }
        // err against the host's ||a - c z||_F, relative to ||a||_F (an exactly low-rank block leaves only rounding in both)
        gap = std::fmax(gap, std::fabs((double)err[(std::size_t)b] - std::sqrt(e2)) / std::sqrt(a2));
        worst = std::fmax(worst, (double)err[(std::size_t)b] / (double)nrm[(std::size_t)b]);
        gap = std::fmax(gap, std::fabs((double)nrm[(std::size_t)b] - std::sqrt(a2)) / std::sqrt(a2));
    }
    expect("  residual_batched: err, nrm against the host", gap, res_bound);
    expect("  residual_batched: err / nrm", worst, bound);
    if (m > 512) return;  // the recompression holds a factor in one workgroup: m <= 512
    const auto svd = recompress_batched(id, k, tol);
    bad = 0;
    for (int64_t v : svd.ranks.to_host()) bad += v != r;
    expect("  recompress_batched: ranks", bad, 0);
    const auto rs = residual_batched(svd, a);
    const auto serr = rs.err.to_host(), snrm = rs.nrm.to_host();
    worst = 0;
    for (int32_t b = 0; b < count; ++b) worst = std::fmax(worst, (double)serr[(std::size_t)b] / (double)snrm[(std::size_t)b]);
    expect("  recompress_batched: err / nrm", worst, bound);
}

int main() {
    int rc = 0;
    try {
        check<c64>("sketched column_id_rank_batched<c64>, tall", 3, 1500, 1e-10, 1e-10, 1e-9, 91);
        check<c64>("sketched column_id_rank_batched<c64>", 3, 400, 1e-10, 1e-10, 1e-9, 92);
        check<c32>("sketched column_id_rank_batched<c32>, tall", 3, 1500, 1e-3, 1e-4, 1e-4, 93);
        check<c32>("sketched column_id_rank_batched<c32>", 3, 400, 1e-3, 1e-4, 1e-4, 94);
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
