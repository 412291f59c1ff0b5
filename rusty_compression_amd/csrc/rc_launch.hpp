// What every launch site of the library shares (host only; nothing here needs a HIP header, so the guard compiles and is tested
// on a CPU: tests/cpp/first_use_test.cpp): the LDS budget of a CU under one set of names, the first-use guard behind which a
// kernel's dynamic-LDS limit is raised, the cached CU count, and the grid rule and first-use cap of the persistent batched kernels
// (rc_batched_launch.hpp).  The definitions are in rc_launch.hip.
#pragma once
#include <atomic>
#include <cstddef>
#include <cstdint>
#include <mutex>

struct rc_context;

namespace rc {

// ---- the LDS budget ---------------------------------------------------------------------------------------------------------------
// A CU of the MI355X has 160 KiB of LDS.  No kernel asks for all of it as dynamic LDS: each cap leaves a reserve for the kernel's
// static __shared__ words (reduction and broadcast slots, small tiles).  These numbers decide routes (tsqr_supported,
// wide_lazy_supported, form_q's T-builder, the batched plans) and the domains of the small kernels.
constexpr size_t kCuLdsBytes = 160 * 1024;
// the common cap: the batched family's (BID_MAX_LDS) and that of the single-workgroup dense kernels
constexpr size_t kLdsCap = kCuLdsBytes - 1024;
// the limit of the Jacobi kernels (k_wq_jacobi_fused keeps over 1 KiB of static words beside the Jacobi's array: xw, sh_v, ...) and
// the CholeskyQR2 route's bound on its small kernels
constexpr size_t kLdsCapWide = kCuLdsBytes - 2048;
// what a Jacobi launch may ask for under that limit: the padded pitch is used whenever it fits this (jacobi_pitch)
constexpr size_t kJacobiLdsCap = kLdsCapWide - 64;
// k_rsvd_id_tails: a 16 x 17 tile and 128 64-bit indices of static LDS beside the dynamic array
constexpr size_t kLdsCapTails = kCuLdsBytes - 4096;

// ---- first use per device ---------------------------------------------------------------------------------------------------------
// once(device, action): for device numbers 0..63 the action runs exactly once per device; callers that race wait for it, its effects
// are visible to every later caller, and a device whose action throws is not marked (the next caller runs it again).  After that a
// call is one acquire load and a bit test.  Device numbers outside 0..63 run the action on every call, under the lock.
class FirstUse {
public:
    template <typename Action>
    void operator()(int device, Action &&action) {
        const bool tracked = device >= 0 && device < 64;
        const uint64_t bit = tracked ? uint64_t(1) << device : 0;
        if (done_.load(std::memory_order_acquire) & bit) return;
        std::lock_guard<std::mutex> lock(mu_);
        if (done_.load(std::memory_order_relaxed) & bit) return;
        action();
        done_.fetch_or(bit, std::memory_order_release);
    }

private:
    std::atomic<uint64_t> done_{0};
    std::mutex mu_;
};

// raises kern's dynamic-LDS limit (hipFuncAttributeMaxDynamicSharedMemorySize) to `bytes` on the current device; throws as RC_HIP does
void set_dynamic_lds_limit(const void *kern, size_t bytes);

// One line per launch site: the first launch of Kern on `device` raises its dynamic-LDS limit to `bytes` (one guard per kernel
// instance; every site of an instance passes the same bytes).
template <auto Kern>
inline void raise_lds_limit(int device, size_t bytes) {
    static FirstUse once;
    once(device, [&] { set_dynamic_lds_limit(reinterpret_cast<const void *>(Kern), bytes); });
}

// CUs of the device (256 where the query fails); cached, thread-safe
int device_cus(int device);

// ---- the persistent batched kernels (the rule and its use: rc_batched_launch.hpp) ----------------------------------------------------
constexpr int BATCHED_THREADS = 256;
constexpr size_t BID_MAX_LDS = kLdsCap;
int64_t bid_grid(rc_context *c, const void *kern, size_t lds, size_t ws_per, int32_t count, int64_t *slots);
int batched_kernel_cap(int device, const void *kern);

}  // namespace rc
