// The LDS Jacobi of a 128 x 128 f64 core as a lone two-workgroup launch (producer + consumer) of 1024 threads, one column pair per
// 16-lane group: k_jacobi_lds of the library and the Jacobi role of k_wq_jacobi_fused.  (The 512-thread layout with two pairs per
// group that this tool compared it with -- +27 % per launch, profiles/r05_fused_ab.txt -- is gone from the library.)
// Prints the median launch time and whether two launches agree bit for bit.  Build: make -C tools/microbench jacobi_lanes
#include "../../rusty_compression_amd/csrc/jacobi_lds.hpp"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

using namespace rc;

#define CHECK(x)                                                                                  \
    do {                                                                                          \
        hipError_t e_ = (x);                                                                      \
        if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 1; } \
    } while (0)

template <int THREADS>
__global__ __launch_bounds__(THREADS) void k_jacobi(JacobiLdsArgs<double> ja) {
    jacobi_lds_body<double, 8, true>(ja, blockIdx.x == 1);
}

struct Result {
    std::vector<double> u, s, v;
    float ms = 0;
    int sweeps = 0, health = 0;
};

template <int THREADS>
static int run(const double *g_dev, Result &out) {
    constexpr int n = 128;
    const size_t nrec = (size_t)kMaxSweeps * (n - 1) * (n / 2);
    double *uc, *vc, *s;
    Rot<double> *log;
    unsigned long long *chk;
    unsigned *vsync, *epoch;
    int *sweeps, *order, *health;
    CHECK(hipMalloc(&uc, n * n * 8));
    CHECK(hipMalloc(&vc, n * n * 8));
    CHECK(hipMalloc(&s, n * 8));
    CHECK(hipMalloc(&log, nrec * sizeof(Rot<double>)));
    CHECK(hipMalloc(&chk, nrec * 8));
    CHECK(hipMalloc(&vsync, (n + 1) * 4));
    CHECK(hipMalloc(&epoch, 4));
    CHECK(hipMalloc(&sweeps, 4));
    CHECK(hipMalloc(&order, n * 4));
    CHECK(hipMalloc(&health, 4));
    const unsigned e0 = 0x2a51u;
    CHECK(hipMemcpy(epoch, &e0, 4, hipMemcpyHostToDevice));
    CHECK(hipMemset(health, 0, 4));
    const int ld = jacobi_pitch<double>(n);
    const size_t lds = jacobi_lds_bytes<double>(n, ld);
    auto kern = k_jacobi<THREADS>;
    CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 2048));
    JacobiLdsArgs<double> ja{Mat<double>(const_cast<double *>(g_dev), n, n, 1, n), log, sweeps, Mat<double>(uc, n, n, 1, n), s, order, kMaxSweeps, 1, vsync, chk, epoch,
                             Mat<double>(vc, n, n, 1, n), health, ld};
    hipEvent_t t0, t1;
    CHECK(hipEventCreate(&t0));
    CHECK(hipEventCreate(&t1));
    std::vector<float> ms;
    for (int it = 0; it < 12; ++it) {
        CHECK(hipMemsetAsync(vsync, 0, (n + 1) * 4, 0));
        CHECK(hipEventRecord(t0, 0));
        hipLaunchKernelGGL(kern, dim3(2), dim3(THREADS), lds, 0, ja);
        CHECK(hipEventRecord(t1, 0));
        CHECK(hipEventSynchronize(t1));
        float t;
        CHECK(hipEventElapsedTime(&t, t0, t1));
        if (it >= 2) ms.push_back(t);
    }
    CHECK(hipGetLastError());
    std::sort(ms.begin(), ms.end());
    out.ms = ms[ms.size() / 2];
    out.u.resize(n * n);
    out.v.resize(n * n);
    out.s.resize(n);
    CHECK(hipMemcpy(out.u.data(), uc, n * n * 8, hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(out.v.data(), vc, n * n * 8, hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(out.s.data(), s, n * 8, hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(&out.sweeps, sweeps, 4, hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(&out.health, health, 4, hipMemcpyDeviceToHost));
    return 0;
}

int main() {
    constexpr int n = 128;
    std::vector<double> g(n * n);
    unsigned long long x = 88172645463325252ull;
    for (double &v : g) {  // sum of four uniforms, centred: close enough to a Gaussian core
        double acc = 0;
        for (int k = 0; k < 4; ++k) {
            x ^= x << 13; x ^= x >> 7; x ^= x << 17;
            acc += (double)(x >> 11) / 9007199254740992.0;
        }
        v = acc - 2.0;
    }
    double *g_dev;
    CHECK(hipMalloc(&g_dev, n * n * 8));
    CHECK(hipMemcpy(g_dev, g.data(), n * n * 8, hipMemcpyHostToDevice));
    Result a, b;
    if (run<1024>(g_dev, a) || run<1024>(g_dev, b)) return 1;
    const bool same = !memcmp(a.u.data(), b.u.data(), n * n * 8) && !memcmp(a.v.data(), b.v.data(), n * n * 8) && !memcmp(a.s.data(), b.s.data(), n * 8);
    printf("{\"n\": %d, \"ms_1024_threads\": [%.4f, %.4f], \"sweeps\": [%d, %d], \"health\": [%d, %d], \"u_s_v_bitwise_equal\": %s}\n", n, a.ms, b.ms, a.sweeps,
           b.sweeps, a.health, b.health, same ? "true" : "false");
    return same && a.health == 0 && b.health == 0 ? 0 : 2;
}
