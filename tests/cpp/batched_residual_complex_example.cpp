// The batched residual norms of complex factors through the C++ mirror include/rusty_compression.hpp: residual_batched of a batched
// column ID, a batched two-sided ID and a batched SVD for c64 and c32, on stacks of exactly low-rank complex blocks plus a perturbation,
// with the residual blocks requested from the first.  Checked on the host against the factors the calls returned: err is the Frobenius
// norm of a - left mid diag(s) right formed in complex double (nothing conjugated), nrm that of a, and e the residual itself.  Prints one
// "name value" line per check and exits non-zero when one fails; the CPU suite only compiles and links it.
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

// the residual blocks a - left[:, :r] mid[:r, :r] diag(s[:r]) right[:r, :] of a stack in complex double, C order (mid, s empty: absent)
template <typename T>
static std::vector<zd> host_residual(const std::vector<T> &a, const std::vector<T> &left, const std::vector<T> &mid,
                                     const std::vector<typename Scalar<T>::real> &s, int64_t s_stride, const std::vector<T> &right,
                                     const std::vector<int64_t> &ranks, int32_t count, int64_t m, int64_t n, int64_t k) {
    std::vector<zd> e((std::size_t)(count * m * n));
    std::vector<zd> w((std::size_t)(k * n)), w2((std::size_t)(k * n));
    for (int32_t b = 0; b < count; ++b) {
        const int64_t r = ranks[(std::size_t)b];
        for (int64_t l = 0; l < r; ++l)
            for (int64_t j = 0; j < n; ++j)
                w[(std::size_t)(l * n + j)] = (s.empty() ? 1.0 : (double)s[(std::size_t)(b * s_stride + l)]) * zd(right[(std::size_t)((b * k + l) * n + j)]);
        if (!mid.empty()) {
            for (int64_t l = 0; l < r; ++l)
                for (int64_t j = 0; j < n; ++j) {
                    zd acc = 0;
                    for (int64_t p = 0; p < r; ++p) acc += zd(mid[(std::size_t)((b * k + l) * k + p)]) * w[(std::size_t)(p * n + j)];
                    w2[(std::size_t)(l * n + j)] = acc;
                }
            w.swap(w2);
        }
        for (int64_t i = 0; i < m; ++i)
            for (int64_t j = 0; j < n; ++j) {
                zd acc = 0;
                for (int64_t l = 0; l < r; ++l) acc += zd(left[(std::size_t)((b * m + i) * k + l)]) * w[(std::size_t)(l * n + j)];
                e[(std::size_t)((b * m + i) * n + j)] = zd(a[(std::size_t)((b * m + i) * n + j)]) - acc;
            }
    }
    return e;
}

// the largest relative distance of the device norms from the Frobenius norms of the blocks of a host stack
template <typename R>
static double norm_gap(const std::vector<R> &dev, const std::vector<zd> &stack, int32_t count, int64_t per) {
    double worst = 0;
    for (int32_t b = 0; b < count; ++b) {
        double acc = 0;
        for (int64_t i = 0; i < per; ++i) acc += std::norm(stack[(std::size_t)(b * per + i)]);
        const double ref = std::sqrt(acc);
        worst = std::fmax(worst, std::fabs((double)dev[(std::size_t)b] - ref) / (ref > 0 ? ref : 1.0));
    }
    return worst;
}

template <typename T>
static void check(const char *tag, int32_t count, int64_t m, int64_t n, double bound, uint64_t seed) {
    using Real = typename Scalar<T>::real;
    Context ctx(0);
    const int64_t r = 6, k = 10;
    const auto hx = random_gaussian<T>(ctx, count * m, r, seed).to_host(), hy = random_gaussian<T>(ctx, count * r, n, seed + 1).to_host();
    auto ha = random_gaussian<T>(ctx, count * m, n, seed + 2).to_host();
    for (int32_t b = 0; b < count; ++b)
        for (int64_t i = 0; i < m; ++i)
            for (int64_t j = 0; j < n; ++j) {
                zd acc = 1e-1 * zd(ha[(std::size_t)((b * m + i) * n + j)]);
                for (int64_t l = 0; l < r; ++l) acc += zd(hx[(std::size_t)((b * m + i) * r + l)]) * zd(hy[(std::size_t)((b * r + l) * n + j)]);
                ha[(std::size_t)((b * m + i) * n + j)] = T((Real)acc.real(), (Real)acc.imag());
            }
    const std::vector<zd> had(ha.begin(), ha.end());
    const auto a = DeviceMatrix<T>::from_host(ctx, ha.data(), count * m, n);
    const std::vector<T> none;
    const std::vector<Real> no_s;
    std::printf("%s:\n", tag);
    {
        const auto id = column_id_rank_batched<T>(a, count, k, 0.0);
        const auto res = residual_batched(id, a, true);
        const auto e = host_residual(ha, id.c.to_host(), none, no_s, 0, id.z.to_host(), id.ranks.to_host(), count, m, n, k);
        expect("  column ID: err", norm_gap(res.err.to_host(), e, count, m * n), bound);
        expect("  column ID: nrm", norm_gap(res.nrm.to_host(), had, count, m * n), bound);
        const auto he = res.e.to_host();
        double num = 0, den = 0;
        for (std::size_t i = 0; i < e.size(); ++i) {
            num += std::norm(zd(he[i]) - e[i]);
            den += std::norm(had[i]);
        }
        expect("  column ID: e", res.has_e ? std::sqrt(num / den) : 1.0, bound);
    }
    {
        const auto ts = two_sided_id_rank_batched<T>(a, count, k, 0.0);
        const auto rts = residual_batched(ts, a);
        expect("  two-sided ID: err", norm_gap(rts.err.to_host(), host_residual(ha, ts.c.to_host(), ts.x.to_host(), no_s, 0, ts.r.to_host(), ts.ranks.to_host(), count, m, n, k), count, m * n), bound);
    }
    {
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
        check<c64>("residual_batched<c64>", 4, 200, 60, 1e-10, 81);
        check<c32>("residual_batched<c32>", 3, 300, 70, 1e-4, 82);
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
