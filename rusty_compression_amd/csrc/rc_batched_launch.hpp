// The launch path of the persistent batched kernels (host only, but for the tall recompressions' stage arithmetic): every launcher of kernels_batched_id.hip, kernels_batched_id_c.hip,
// kernels_batched_apply.hip, kernels_block_operator.hip, kernels_batched_residual.hip and kernels_batched_residual_c.hip goes
//     plan (a pure function of the shapes, in its own file)  ->  batched_prepare  ->  ProfScope  ->  workspace()  ->  launch(...)
// so that the LDS cap, the grid rule, the workspace unit (bytes) and the launch check live here once.  The plans and launcher bodies of
// kernels_batched_id.hip and kernels_batched_id_c.hip are written once for all four element types: those of the column and two-sided IDs in
// batched_stages.hpp, with the device stages the real and complex kernels share, the others in batched_launchers.hpp.
#pragma once
#include <algorithm>

#include "rc_common.hpp"
#include "rc_launch.hpp"

namespace rc {

// Declared in rc_launch.hpp and defined in rc_launch.hip, beside the dense launch sites' first-use guard:
//
// BATCHED_THREADS, BID_MAX_LDS, bid_grid: the workgroup of every batched kernel, the dynamic-LDS cap they share, and the persistent
// grid: the resident workgroups of BATCHED_THREADS threads on every CU, fewer when the workspace (ws_per bytes per workgroup, 0 without
// one) would pass 256 MiB unless that leaves less than one workgroup per CU; never more than count.  *slots receives the grid before
// that last bound (slots= in the profile label)
//
// batched_kernel_cap: first use of kern on the device (process-wide, behind a mutex): its dynamic-LDS limit is raised to BID_MAX_LDS
// and its scratch bytes per thread are read.  Every call returns the latter; a thread that asks for the kernel it asked for last gets
// the answer without the lock.

// the tall recompressions (k_batched_recompress<T, true>, k_batched_recompress_c<R, true>): the stage height of their flat Householder TSQR,
// the stages of an m-row left factor of inner rank q, one stage in the workgroup's slot in elements of the kernel's scalar (the copy, H x K at
// pitch H, then taus[K] and pivots[K], the pivots as ints in K elements), and the launchers' own bound on the grid: the workspace of all
// slots stays at or below 2 GiB, never below one workgroup
constexpr int BRT_H = 512;
__host__ __device__ inline int brt_stages(int m, int q) { return m <= BRT_H ? 1 : 1 + (m - BRT_H + (BRT_H - q) - 1) / (BRT_H - q); }
__host__ __device__ inline size_t brt_stage_elems(int K) { return (size_t)BRT_H * K + 2 * (size_t)K; }
constexpr size_t BRT_MAX_WS = (size_t)2 << 30;
inline int64_t brt_grid_cap(int64_t grid, size_t ws_per) {
    return ws_per ? std::min<int64_t>(grid, std::max<int64_t>(1, (int64_t)(BRT_MAX_WS / ws_per))) : grid;
}

// a launcher's plan: where its movable buffers live (Place: the launcher's own flags and core pitch), the dynamic LDS and the workspace
// slot of one workgroup, both in bytes.  Every launcher computes it in a pure function of the shapes, the presence flags and the scalar type.
template <typename Place>
struct BatchedPlan {
    Place at;
    size_t lds, ws;
};

// the first of the n candidate places, in the list's order, whose LDS need lds(place) is at most BID_MAX_LDS; ws(place) is its workspace
template <typename Place, typename Lds, typename Ws>
BatchedPlan<Place> batched_first_fit(const Place *places, size_t n, Lds lds, Ws ws, const char *what) {
    size_t i = 0;
    while (i < n && (size_t)lds(places[i]) > BID_MAX_LDS) ++i;
    RC_REQUIRE(i < n, RC_RUNTIME_ERROR, "%s: %zu bytes of LDS", what, (size_t)lds(places[n - 1]));
    return {places[i], (size_t)lds(places[i]), (size_t)ws(places[i])};
}
template <typename Place, size_t N, typename Lds, typename Ws>
BatchedPlan<Place> batched_first_fit(const Place (&places)[N], Lds lds, Ws ws, const char *what) {
    return batched_first_fit(places, N, lds, ws, what);
}
// the launchers with one movable buffer W of w_bytes: in LDS when lds(true) fits, else in the workspace
template <typename Lds>
BatchedPlan<bool> batched_lds_or_ws(Lds lds, size_t w_bytes, const char *what) {
    const bool places[] = {true, false};
    return batched_first_fit(places, lds, [&](bool w_lds) { return w_lds ? (size_t)0 : w_bytes; }, what);
}

// one prepared launch of kern: grid and slots for the ProfScope label, then the workspace, then the launch
template <typename... P>
struct BatchedLaunch {
    rc_context *c;
    void (*kern)(P...);
    size_t lds, ws_per;  // bytes; ws_per per workgroup
    int64_t grid, slots;
    int scratch;  // bytes per thread the compiler spilled (scratch= in the sketched IDs' labels)

    // the workgroups' slots, workgroup blockIdx.x's at blockIdx.x * ws_per bytes (nullptr without a workspace)
    template <typename T>
    T *workspace() const { return ws_per ? static_cast<T *>(c->alloc_bytes((size_t)grid * ws_per)) : nullptr; }
    void launch(P... args) const {
        hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(BATCHED_THREADS), lds, c->stream, args...);
        RC_HIP(hipGetLastError());
    }
};

// caps kern's LDS on first use, requires lds to fit and sizes the grid for `units` work units by bid_grid's rule
template <typename... P>
BatchedLaunch<P...> batched_prepare(rc_context *c, void (*kern)(P...), const char *what, size_t lds, size_t ws_per, int64_t units) {
    RC_REQUIRE(lds <= BID_MAX_LDS, RC_RUNTIME_ERROR, "%s: %zu bytes of LDS", what, lds);
    BatchedLaunch<P...> l{c, kern, lds, ws_per, 0, 0, 0};
    l.scratch = batched_kernel_cap(c->device, reinterpret_cast<const void *>(kern));
    l.grid = bid_grid(c, reinterpret_cast<const void *>(kern), lds, ws_per, (int32_t)std::min<int64_t>(units, INT32_MAX), &l.slots);
    return l;
}

}  // namespace rc
