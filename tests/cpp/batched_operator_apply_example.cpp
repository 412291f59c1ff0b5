// The block-sparse operator through the C++ mirror include/rusty_compression.hpp: a Gaussian matrix is cut into a grid of m x n tiles, the
// tiles are compressed at full rank by column_id_rank_batched / svd_rank_batched (so the factors reproduce them to the rounding level), one
// tile is kept dense, and BlockOperator applies the whole matrix and its conjugate transpose in one launch each (rc_block_operator_apply_*);
// the results are checked on the host against the dense products.  The operator is also handed to sample_range_by_rank through the callback
// table.  Prints one "name value" line per check and exits non-zero when one fails; the CPU suite only compiles and links it.
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
static double rel(const std::vector<T> &x, const std::vector<T> &ref) {
    double num = 0, den = 0;
    for (std::size_t i = 0; i < ref.size(); ++i) {
        num += std::norm(x[i] - ref[i]);
        den += std::norm(ref[i]);
    }
    return std::sqrt(num / den);
}

static double conj_of(double v) { return v; }
static float conj_of(float v) { return v; }
template <typename R> static std::complex<R> conj_of(std::complex<R> v) { return std::conj(v); }

template <typename T>
static void check(const char *tag, int64_t br, int64_t bc, int64_t m, int64_t n, int64_t nrhs, bool svd, double bound, uint64_t seed) {
    Context ctx(0);
    const int32_t count = (int32_t)(br * bc);
    const int64_t M = br * m, N = bc * n, k = m < n ? m : n;
    // the tiles stacked: tile i = (bi, bj) in rows i m .. (i + 1) m - 1 of `tiles`; the last one is applied as a dense block
    auto tiles = random_gaussian<T>(ctx, count * m, n, seed);
    auto x = random_gaussian<T>(ctx, N, nrhs, seed + 1), z = random_gaussian<T>(ctx, M, nrhs, seed + 2);
    const auto ht = tiles.to_host(), hx = x.to_host(), hz = z.to_host();
    std::vector<int64_t> rows, cols, ids;
    for (int64_t bi = 0; bi < br; ++bi)
        for (int64_t bj = 0; bj < bc; ++bj) {
            const int64_t i = bi * bc + bj;
            rows.push_back(bi * m);
            cols.push_back(bj * n);
            ids.push_back(i == count - 1 ? count : i);  // id count = dense block 0
        }
    auto dense = DeviceMatrix<T>::from_host(ctx, ht.data() + (std::size_t)((count - 1) * m * n), m, n);
    std::vector<T> ax((std::size_t)(M * nrhs)), ahz((std::size_t)(N * nrhs));
    for (int64_t i = 0; i < M; ++i)
        for (int64_t j = 0; j < N; ++j) {
            const T a = ht[(std::size_t)((((i / m) * bc + j / n) * m + i % m) * n + j % n)];
            for (int64_t c = 0; c < nrhs; ++c) {
                ax[(std::size_t)(i * nrhs + c)] += a * hx[(std::size_t)(j * nrhs + c)];
                ahz[(std::size_t)(j * nrhs + c)] += conj_of(a) * hz[(std::size_t)(i * nrhs + c)];
            }
        }
    std::printf("%s:\n", tag);
    if (svd) {
        const auto f = svd_rank_batched<T>(tiles, count, k);
        BlockOperator<T> op(ctx, M, N, rows, cols, ids, count, &f.u, nullptr, &f.s, &f.vt, &f.ranks, 1, &dense);
        expect("  svd blocks  A x", rel(op.apply(x).to_host(), ax), bound);
        expect("  svd blocks  A^H z", rel(op.conj_apply(z).to_host(), ahz), bound);
    } else {
        const auto f = column_id_rank_batched<T>(tiles, count, k);
        BlockOperator<T> op(ctx, M, N, rows, cols, ids, count, &f.c, nullptr, nullptr, &f.z, &f.ranks, 1, &dense);
        expect("  column_id blocks  A x", rel(op.apply(x).to_host(), ax), bound);
        expect("  column_id blocks  A^H z", rel(op.conj_apply(z).to_host(), ahz), bound);
        const auto q = sample_range_by_rank<T>(ctx, op, 8, 4, seed + 3);  // the operator behind the callback table
        expect("  range finder columns", std::fabs((double)q.ncols() - 8.0), 0.0);  // min(k, nrows, k + p) columns
    }
    ctx.synchronize();
}

int main() {
    int rc = 0;
    try {
        check<double>("BlockOperator<double>", 3, 2, 40, 24, 3, false, 1e-10, 51);
        check<float>("BlockOperator<float>", 2, 3, 24, 40, 1, true, 1e-3, 52);
        check<c64>("BlockOperator<c64>", 2, 2, 30, 20, 9, true, 1e-10, 53);
        check<c32>("BlockOperator<c32>", 2, 2, 20, 30, 5, false, 1e-3, 54);
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
