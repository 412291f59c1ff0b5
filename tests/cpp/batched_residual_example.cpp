// The batched residual norms through the C++ mirror include/rusty_compression.hpp: residual_batched of a batched column ID (plain and
// sketched, the latter on blocks taller than the batched apply accepts), a batched two-sided ID and a batched SVD, on stacks of exactly
// low-rank blocks plus a perturbation, with the residual blocks requested from the first.  Checked on
// the host against the factors the calls returned: err is the Frobenius norm of a - left mid diag(s) right formed in double, nrm that of a,
// and e the residual itself.  Prints one "name value" line per check and exits non-zero when one fails; the CPU suite only compiles and
// links it.
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

// the residual blocks a - left[:, :r] mid[:r, :r] diag(s[:r]) right[:r, :] of a stack in double, C order (mid, s empty: absent)
template <typename T>
static std::vector<double> host_residual(const std::vector<T> &a, const std::vector<T> &left, const std::vector<T> &mid, const std::vector<T> &s,
                                         int64_t s_stride, const std::vector<T> &right, const std::vector<int64_t> &ranks, int32_t count, int64_t m,
                                         int64_t n, int64_t k) {
    std::vector<double> e((std::size_t)(count * m * n));
    std::vector<double> w((std::size_t)(k * n)), w2((std::size_t)(k * n));
    for (int32_t b = 0; b < count; ++b) {
        const int64_t r = ranks[(std::size_t)b];
        for (int64_t l = 0; l < r; ++l)
            for (int64_t j = 0; j < n; ++j)
                w[(std::size_t)(l * n + j)] = (s.empty() ? 1.0 : (double)s[(std::size_t)(b * s_stride + l)]) * (double)right[(std::size_t)((b * k + l) * n + j)];
        if (!mid.empty()) {
            for (int64_t l = 0; l < r; ++l)
                for (int64_t j = 0; j < n; ++j) {
                    double acc = 0;
                    for (int64_t p = 0; p < r; ++p) acc += (double)mid[(std::size_t)((b * k + l) * k + p)] * w[(std::size_t)(p * n + j)];
                    w2[(std::size_t)(l * n + j)] = acc;
                }
            w.swap(w2);
        }
        for (int64_t i = 0; i < m; ++i)
            for (int64_t j = 0; j < n; ++j) {
                double acc = 0;
                for (int64_t l = 0; l < r; ++l) acc += (double)left[(std::size_t)((b * m + i) * k + l)] * w[(std::size_t)(l * n + j)];
                e[(std::size_t)((b * m + i) * n + j)] = (double)a[(std::size_t)((b * m + i) * n + j)] - acc;
            }
    }
    return e;
}

// the largest relative distance of the device norms from the Frobenius norms of the blocks of a host stack
template <typename T>
static double norm_gap(const std::vector<T> &dev, const std::vector<double> &stack, int32_t count, int64_t per) {
    double worst = 0;
    for (int32_t b = 0; b < count; ++b) {
        double acc = 0;
        for (int64_t i = 0; i < per; ++i) acc += stack[(std::size_t)(b * per + i)] * stack[(std::size_t)(b * per + i)];
        const double ref = std::sqrt(acc);
        worst = std::fmax(worst, std::fabs((double)dev[(std::size_t)b] - ref) / (ref > 0 ? ref : 1.0));
    }
    return worst;
}

template <typename T>
static void check(const char *tag, int32_t count, int64_t m, int64_t n, double bound, uint64_t seed) {
    Context ctx(0);
    const int64_t r = 6, k = 10;
    const auto hx = random_gaussian<T>(ctx, count * m, r, seed).to_host(), hy = random_gaussian<T>(ctx, count * r, n, seed + 1).to_host();
    auto ha = random_gaussian<T>(ctx, count * m, n, seed + 2).to_host();
    for (int32_t b = 0; b < count; ++b)
        for (int64_t i = 0; i < m; ++i)
            for (int64_t j = 0; j < n; ++j) {
                double acc = 1e-1 * (double)ha[(std::size_t)((b * m + i) * n + j)];
                for (int64_t l = 0; l < r; ++l) acc += (double)hx[(std::size_t)((b * m + i) * r + l)] * (double)hy[(std::size_t)((b * r + l) * n + j)];
                ha[(std::size_t)((b * m + i) * n + j)] = (T)acc;
            }
    const std::vector<double> had(ha.begin(), ha.end());
    const auto a = DeviceMatrix<T>::from_host(ctx, ha.data(), count * m, n);
    const std::vector<T> none;
    std::printf("%s:\n", tag);
    {
        const auto omega = random_gaussian<T>(ctx, k + 8, m, seed + 3);
        const auto id = column_id_rank_batched<T>(a, omega, count, k, 0.0);
        const auto res = residual_batched(id, a, true);
        const auto e = host_residual(ha, id.c.to_host(), none, none, 0, id.z.to_host(), id.ranks.to_host(), count, m, n, id.c.ncols());
        expect("  sketched column ID: err", norm_gap(res.err.to_host(), e, count, m * n), bound);
        expect("  sketched column ID: nrm", norm_gap(res.nrm.to_host(), had, count, m * n), bound);
        const auto he = res.e.to_host();
        double num = 0, den = 0;
        for (std::size_t i = 0; i < e.size(); ++i) {
            num += ((double)he[i] - e[i]) * ((double)he[i] - e[i]);
            den += had[i] * had[i];
        }
        expect("  sketched column ID: e", res.has_e ? std::sqrt(num / den) : 1.0, bound);
    }
    if (m <= 512) {
        const auto id = column_id_rank_batched<T>(a, count, k, 0.0);
        const auto res = residual_batched(id, a);
        expect("  column ID: err", norm_gap(res.err.to_host(), host_residual(ha, id.c.to_host(), none, none, 0, id.z.to_host(), id.ranks.to_host(), count, m, n, k), count, m * n), bound);
        const auto ts = two_sided_id_rank_batched<T>(a, count, k, 0.0);
        const auto rts = residual_batched(ts, a);
        expect("  two-sided ID: err", norm_gap(rts.err.to_host(), host_residual(ha, ts.c.to_host(), ts.x.to_host(), none, 0, ts.r.to_host(), ts.ranks.to_host(), count, m, n, k), count, m * n), bound);
    }
    if (m <= 512 && n <= 128) {
        const auto svd = svd_rank_batched<T>(a, count, k, 0.0);
        const auto res = residual_batched(svd, a);
        const int64_t p = m < n ? m : n;
        expect("  SVD: err", norm_gap(res.err.to_host(), host_residual(ha, svd.u.to_host(), none, svd.s.to_host(), p, svd.vt.to_host(), svd.ranks.to_host(), count, m, n, k), count, m * n), bound);
        expect("  SVD: has no e", res.has_e ? 1.0 : 0.0, 0.0);
    }
}

int main() {
    int rc = 0;
    try {
        check<double>("residual_batched<double>", 4, 200, 60, 1e-10, 71);
        check<double>("residual_batched<double>, tall", 2, 3000, 40, 1e-10, 72);
        check<float>("residual_batched<float>", 3, 300, 70, 1e-4, 73);
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
