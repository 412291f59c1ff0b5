// Host side of rc_launch.hpp (no kernels): the one call that raises a kernel's dynamic-LDS limit, the cached CU count, and the grid
// rule and first-use cap of the persistent batched kernels.
#include <algorithm>
#include <map>
#include <mutex>
#include <utility>

#include "rc_common.hpp"
#include "rc_launch.hpp"

namespace rc {

void set_dynamic_lds_limit(const void *kern, size_t bytes) {
    RC_HIP(hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
}

int device_cus(int device) {
    // (a race on a slot stores the same value twice)
    static std::atomic<int> cached[64];
    const bool slot = device >= 0 && device < 64;
    int cus = slot ? cached[device].load(std::memory_order_relaxed) : 0;
    if (!cus) {
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || cus <= 0) cus = 256;
        if (slot) cached[device].store(cus, std::memory_order_relaxed);
    }
    return cus;
}

// the persistent grid of the whole batched family (the rule: rc_batched_launch.hpp)
int64_t bid_grid(rc_context *c, const void *kern, size_t lds, size_t ws_per, int32_t count, int64_t *slots) {
    const int cus = device_cus(c->device);
    int per_cu = 0;
    RC_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, BATCHED_THREADS, lds));
    int64_t grid = (int64_t)cus * std::max(per_cu, 1);
    if (ws_per) grid = std::min<int64_t>(grid, std::max<int64_t>(cus, (int64_t)((size_t)256 << 20) / (int64_t)ws_per));
    *slots = grid;
    return std::min<int64_t>(grid, count);
}

int batched_kernel_cap(int device, const void *kern) {
    // the calling thread's last answer first: a loop over one entry point takes neither the lock nor the lookup
    thread_local int last_device = -1, last_scratch = 0;
    thread_local const void *last_kern = nullptr;
    if (device == last_device && kern == last_kern) return last_scratch;
    static std::mutex mu;
    static std::map<std::pair<int, const void *>, int> scratch_of;
    std::lock_guard<std::mutex> lock(mu);
    auto it = scratch_of.find({device, kern});
    if (it == scratch_of.end()) {
        set_dynamic_lds_limit(kern, BID_MAX_LDS);
        hipFuncAttributes fa;
        RC_HIP(hipFuncGetAttributes(&fa, kern));
        it = scratch_of.emplace(std::make_pair(device, kern), (int)fa.localSizeBytes).first;
    }
    last_device = device; last_kern = kern;
    return last_scratch = it->second;
}

}  // namespace rc
