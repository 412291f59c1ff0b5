// The batched complex IDs through the C++ mirror include/rusty_compression.hpp: column_id_rank_batched<c64> and
// two_sided_id_rank_batched<c32> on a stack of small Gaussian matrices, checked on the host against the exact part of their contract
// (C gathered from A, Z's identity block, c's identity rows, X gathered from A, the reconstruction C Z and c X r).  Prints one
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

// max |A[:, ind[j]] - C[:, j]| over j < k (exact: 0), max |Z[:, ind[:k]] - I| (exact: 0), ||A - C Z|| / ||A|| of one matrix
template <typename T>
static void check_column_id(const char *tag, const T *a, const T *c, const T *z, const int64_t *ind, int64_t m, int64_t n, int64_t k, double recon) {
    double gather = 0, ident = 0, num = 0, den = 0;
    for (int64_t j = 0; j < k; ++j)
        for (int64_t i = 0; i < m; ++i) gather = std::max(gather, (double)std::abs(a[i * n + ind[j]] - c[i * k + j]));
    for (int64_t i = 0; i < k; ++i)
        for (int64_t j = 0; j < k; ++j) ident = std::max(ident, (double)std::abs(z[i * n + ind[j]] - T(i == j ? 1 : 0)));
    for (int64_t i = 0; i < m; ++i)
        for (int64_t j = 0; j < n; ++j) {
            T s = 0;
            for (int64_t l = 0; l < k; ++l) s += c[i * k + l] * z[l * n + j];
            num += std::norm(a[i * n + j] - s);
            den += std::norm(a[i * n + j]);
        }
    std::printf("%s:\n", tag);
    expect("  c_gathered_from_a", gather, 0.0);
    expect("  z_identity_block", ident, 0.0);
    expect("  c_z_reconstruction", std::sqrt(num / den), recon);
}

int main() {
    int rc = 0;
    try {
        Context ctx(0);
        const int32_t count = 5;
        const int64_t m = 40, n = 24, k = 24;  // full rank: C Z reproduces A to the rounding level
        {
            auto a = random_gaussian<c64>(ctx, count * m, n, 21);  // matrix i is rows i m .. (i + 1) m - 1
            auto id = column_id_rank_batched<c64>(a, count, k);
            auto ha = a.to_host();
            auto hc = id.c.to_host(), hz = id.z.to_host();
            auto hind = id.col_ind.to_host(), hr = id.ranks.to_host();
            for (int32_t b = 0; b < count; ++b) {
                if (hr[b] != k) { std::printf("c64 rank %lld != %lld FAILED\n", (long long)hr[b], (long long)k); ++failures; }
                check_column_id("column_id_rank_batched<c64>", ha.data() + b * m * n, hc.data() + b * m * k, hz.data() + b * k * n, hind.data() + b * n, m,
                                n, k, 1e-12);
            }
        }
        {
            const int64_t r = 12;  // two-sided ID at rank 12 < min(m, n)
            auto a = random_gaussian<c32>(ctx, count * m, n, 22);
            auto ts = two_sided_id_rank_batched<c32>(a, count, r);
            auto ha = a.to_host();
            auto hc = ts.c.to_host(), hx = ts.x.to_host();
            auto hrow = ts.row_ind.to_host(), hcol = ts.col_ind.to_host();
            double ident = 0, gather = 0;
            for (int32_t b = 0; b < count; ++b) {
                const c32 *ab = ha.data() + b * m * n, *cb = hc.data() + b * m * r, *xb = hx.data() + b * r * r;
                const int64_t *rows = hrow.data() + b * m, *cols = hcol.data() + b * n;
                for (int64_t i = 0; i < r; ++i)
                    for (int64_t j = 0; j < r; ++j) {
                        ident = std::max(ident, (double)std::abs(cb[rows[i] * r + j] - c32(i == j ? 1.0f : 0.0f)));
                        gather = std::max(gather, (double)std::abs(xb[i * r + j] - ab[rows[i] * n + cols[j]]));
                    }
            }
            std::printf("two_sided_id_rank_batched<c32>:\n");
            expect("  c_identity_rows", ident, 0.0);
            expect("  x_gathered_from_a", gather, 0.0);
        }
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
