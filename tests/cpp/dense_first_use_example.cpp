// First use of the dense kernels from two host threads at once, through the C ABI (include/rusty_compression_amd.h): two std::threads,
// each with its own context on device 0 and released together, run the pivoted QR and the SVD of one seeded 1024 x 96 f64 matrix; after
// the join the main thread repeats both calls on a third context.  1024 x 96 is the smallest tall-skinny shape of the CholeskyQR2 route
// (m >= 1024, m >= 4 n) whose f64 launches need more than the default 64 KiB of dynamic LDS (k_chol_inv 76 928 B, k_qrcp_small /
// k_qrcp_small_q2 about 77 KiB, k_householder_signs 74 496 B): in a fresh process every one of them is raised on first use by
// whichever thread gets there first, and a lost or misordered raise is a failed launch.  Required: every status RC_OK, health 0 on
// all three contexts, all three result sets equal byte for byte.  Prints one line per check and exits non-zero when one fails; the
// CPU suite only compiles and links it.
#include <atomic>
#include <cstdio>
#include <cstring>
#include <functional>
#include <string>
#include <thread>
#include <unistd.h>
#include <vector>

#include "rusty_compression_amd.h"

namespace {

constexpr int64_t M = 1024, N = 96;
constexpr uint64_t SEED_QR = 41, SEED_SVD = 42;

struct Result {
    std::vector<unsigned char> bytes;  // q, r, ind of the QR, then u, s, vt of the SVD
    int32_t health = -1;
    int bad_status = 0;  // the first status that was not RC_OK (0: none), and the call that returned it
    const char *bad_call = "";
    std::string message;
};

rc_matrix rowmajor(void *p, int64_t rows, int64_t cols) { return rc_matrix{p, rows, cols, cols, 1}; }

void run(Result &out, std::atomic<int> *arrived, int parties) {
    rc_context *ctx = nullptr;
    auto ok = [&](rc_status s, const char *call) {
        if (s != RC_OK && !out.bad_status) {
            out.bad_status = (int)s;
            out.bad_call = call;
            if (ctx) out.message = rc_last_error_message(ctx);
        }
        return s == RC_OK;
    };
    const size_t a_b = M * N * 8, r_b = N * N * 8, i_b = N * 8, s_b = N * 8;
    void *a_qr = nullptr, *a_svd = nullptr, *q = nullptr, *r = nullptr, *ind = nullptr, *u = nullptr, *s = nullptr, *vt = nullptr;
    bool good = ok(rc_create(&ctx, 0, nullptr), "rc_create") && ok(rc_device_malloc(ctx, a_b, &a_qr), "malloc") && ok(rc_device_malloc(ctx, a_b, &a_svd), "malloc") &&
                ok(rc_device_malloc(ctx, a_b, &q), "malloc") && ok(rc_device_malloc(ctx, r_b, &r), "malloc") &&
                ok(rc_device_malloc(ctx, i_b, &ind), "malloc") && ok(rc_device_malloc(ctx, a_b, &u), "malloc") &&
                ok(rc_device_malloc(ctx, s_b, &s), "malloc") && ok(rc_device_malloc(ctx, r_b, &vt), "malloc") &&
                ok(rc_random_gaussian_f64(ctx, rowmajor(a_qr, M, N), SEED_QR, 0), "rc_random_gaussian_f64") &&
                ok(rc_random_gaussian_f64(ctx, rowmajor(a_svd, M, N), SEED_SVD, 0), "rc_random_gaussian_f64") &&
                ok(rc_synchronize(ctx), "rc_synchronize");
    // the threads leave together (each arrives whatever happened above): the first dense launch of each is a first use for the process
    if (arrived) {
        arrived->fetch_add(1);
        while (arrived->load() < parties) std::this_thread::yield();
    }
    if (good) {
        good = ok(rc_pivoted_qr_f64(ctx, rowmajor(a_qr, M, N), rowmajor(q, M, N), rowmajor(r, N, N), static_cast<int64_t *>(ind)), "rc_pivoted_qr_f64") &&
               ok(rc_compute_svd_f64(ctx, rowmajor(a_svd, M, N), rowmajor(u, M, N), static_cast<double *>(s), rowmajor(vt, N, N)), "rc_compute_svd_f64") &&
               ok(rc_synchronize(ctx), "rc_synchronize");
    }
    if (good) {
        out.bytes.resize(2 * a_b + 2 * r_b + i_b + s_b);
        unsigned char *p = out.bytes.data();
        const struct { void *dev; size_t n; } parts[] = {{q, a_b}, {r, r_b}, {ind, i_b}, {u, a_b}, {s, s_b}, {vt, r_b}};
        for (const auto &part : parts) {
            good = good && ok(rc_memcpy_d2h(ctx, p, part.dev, part.n), "rc_memcpy_d2h");
            p += part.n;
        }
        ok(rc_get_health(ctx, &out.health), "rc_get_health");
    }
    if (!ctx) return;
    for (void *d : {a_qr, a_svd, q, r, ind, u, s, vt})
        if (d) ok(rc_device_free(ctx, d), "rc_device_free");
    ok(rc_destroy(ctx), "rc_destroy");
}

}  // namespace

int main() {
    Result res[3];
    std::atomic<int> arrived{0};
    std::thread t0(run, std::ref(res[0]), &arrived, 2), t1(run, std::ref(res[1]), &arrived, 2);
    t0.join();
    t1.join();
    run(res[2], nullptr, 0);
    int failures = 0;
    const char *who[3] = {"thread 0", "thread 1", "main after the join"};
    for (int i = 0; i < 3; ++i) {
        const bool st = res[i].bad_status == 0, he = res[i].health == 0;
        std::printf("%s: status %s, health %d\n", who[i], st ? "RC_OK" : "FAILED", (int)res[i].health);
        if (!st) std::printf("  %s returned %d: %s\n", res[i].bad_call, res[i].bad_status, res[i].message.c_str());
        failures += !st + !he;
    }
    for (int i = 1; i < 3; ++i) {
        const bool same = !res[0].bytes.empty() && res[i].bytes.size() == res[0].bytes.size() &&
                          std::memcmp(res[i].bytes.data(), res[0].bytes.data(), res[0].bytes.size()) == 0;
        std::printf("%s equals thread 0 byte for byte (%zu bytes): %s\n", who[i], res[0].bytes.size(), same ? "yes" : "NO  FAILED");
        failures += !same;
    }
    std::printf(failures ? "FAILED %d\n" : "ALL OK\n", failures);
    // every context has been destroyed; leave without running the HIP runtime's exit-time teardown (as mirror_examples.cpp)
    std::fflush(stdout);
    _exit(failures ? 1 : 0);
}
