// Mixed-precision storage through the C++ mirror include/rusty_compression.hpp: the factors of a batched column ID are demoted to
// f32 / c32 (demote_batched), applied and rebuilt by lowrank_apply_batched_mixed, and compared with the full-precision
// lowrank_apply_batched on the promoted factors (promote_batched), which the contract makes the same bits; the distance to the
// full-precision apply on the original factors is the storage rounding.  A MixedBlockOperator on the same factors is compared with the
// BlockOperator on the promoted ones.  Prints one "name value" line per check and exits non-zero when one fails; the CPU suite only
// compiles and links it.
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
static void check(const char *tag, int64_t br, int64_t bc, int64_t m, int64_t n, int64_t nrhs, uint64_t seed) {
    using S = typename Mixed<T>::storage;
    Context ctx(0);
    const int32_t count = (int32_t)(br * bc);
    const int64_t k = m < n ? m : n;
    auto a = random_gaussian<T>(ctx, count * m, n, seed);         // block i is rows i m .. (i + 1) m - 1
    auto b = random_gaussian<T>(ctx, count * n, nrhs, seed + 1);  // block i is rows i n .. (i + 1) n - 1
    std::printf("%s:\n", tag);
    const auto id = column_id_rank_batched<T>(a, count, k);
    DeviceIndex overflow(ctx, (std::size_t)count);
    const DeviceMatrix<S> c_low = demote_batched<T>(id.c, count, &overflow), z_low = demote_batched<T>(id.z, count);
    const DeviceMatrix<T> c_up = promote_batched<T>(c_low, count), z_up = promote_batched<T>(z_low, count);
    int64_t lost = 0;
    for (int64_t v : overflow.to_host()) lost += v;
    expect("  overflowed elements", (double)lost, 0.0);
    const auto y_mixed = lowrank_apply_batched_mixed<T>(c_low, nullptr, nullptr, z_low, &id.ranks, count, &b).to_host();
    const auto y_up = lowrank_apply_batched<T>(c_up, nullptr, nullptr, z_up, &id.ranks, count, &b).to_host();
    const auto y_full = apply_batched(id, b).to_host();
    expect("  apply: mixed against promoted factors", rel(y_mixed, y_up), 0.0);
    expect("  apply: storage rounding", rel(y_mixed, y_full), 1e-5);
    const auto r_mixed = lowrank_apply_batched_mixed<T>(c_low, nullptr, nullptr, z_low, &id.ranks, count, nullptr).to_host();
    expect("  to_mat: mixed against promoted factors", rel(r_mixed, lowrank_apply_batched<T>(c_up, nullptr, nullptr, z_up, &id.ranks, count, nullptr).to_host()), 0.0);
    expect("  to_mat: storage rounding", rel(r_mixed, a.to_host()), 1e-5);
    // the same factors as the tiles of a br x bc block matrix
    std::vector<int64_t> rows, cols, ids;
    for (int64_t bi = 0; bi < br; ++bi)
        for (int64_t bj = 0; bj < bc; ++bj) {
            rows.push_back(bi * m);
            cols.push_back(bj * n);
            ids.push_back(bi * bc + bj);
        }
    auto x = random_gaussian<T>(ctx, bc * n, nrhs, seed + 2), z = random_gaussian<T>(ctx, br * m, nrhs, seed + 3);
    MixedBlockOperator<T> mixed(ctx, br * m, bc * n, rows, cols, ids, count, &c_low, nullptr, nullptr, &z_low, &id.ranks);
    BlockOperator<T> full(ctx, br * m, bc * n, rows, cols, ids, count, &c_up, nullptr, nullptr, &z_up, &id.ranks);
    expect("  operator A x: mixed against promoted factors", rel(mixed.apply(x).to_host(), full.apply(x).to_host()), 0.0);
    expect("  operator A^H z: mixed against promoted factors", rel(mixed.conj_apply(z).to_host(), full.conj_apply(z).to_host()), 0.0);
    ctx.synchronize();
}

int main() {
    int rc = 0;
    try {
        check<double>("mixed<double>", 3, 2, 40, 24, 3, 61);
        check<c64>("mixed<c64>", 2, 2, 30, 20, 9, 62);
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
