// The launcher bodies of the two batched IDs, and the plans and launcher bodies of the batched SVD, the three recompressions, the sketched
// column ID and the range step, written once over the element type E (double, float, cplx<double>, cplx<float>).  Host only.
//
// What a launcher needs of its kernels it takes from BatchedFamily<E>, which kernels_batched_id.hip defines for double and float and
// kernels_batched_id_c.hip for cplx<double> and cplx<float>, each after its kernels:
//   RecompressArgs, SketchIdArgs, RangeStepArgs                      the kernels' argument structs
//   svd_lds_bytes / svd_ws_elems (M, N, BsvPlace)                    dynamic LDS and workspace slot of one workgroup under a place
//   recompress_lds_bytes (m, n, K, BrcPlace), recompress_ws_elems (form, m, n, K, BrcPlace)
//   sketch_id_lds_bytes, range_step_lds_bytes (l, n, w_lds)
//   svd_kernel (BsvPlace), recompress_kernel<FORM> (m, n), sketch_id_kernel, range_step_kernel (a_rows, o_rows)
//                                                                    the instance to launch: the rule differs between the families
// Everything else the families differ in is spelled here, under is_real_elem<E>: a complex core G may leave LDS (one more place at the end of
// every list, written to the complex Args' g_lds), the complex labels and `what` strings, and the range step's conj flag.
#pragma once
#include <algorithm>
#include <cstdio>

#include "batched_stages.hpp"
#include "rc_batched_launch.hpp"
#include "rc_common.hpp"
#include "rc_gemm.hpp"

namespace rc {

template <typename E> struct BatchedFamily;

// where the movable buffers of the SVD (W, V, the core G) and of the recompressions (Wl, Wr, the rotations J, G) live, and the core's
// column pitch; g is true in every place of a real list
struct BsvPlace { bool w, v, g; int ld; };
struct BrcPlace { bool l, r, v, g; int ld; };
// the three recompressions: the small one, a tall left factor, both factors tall
enum { BRC_SMALL = 0, BRC_TALL = 1, BRC_LARGE = 2 };

// ---- the plans: where each launcher's movable buffers live, as pure functions of the shapes (rc_batched_launch.hpp) -------------------------

// SVD, M x N the work orientation: the working copy W (M x N) and V (N x N) in LDS when they fit next to the core (W only with V),
// otherwise in the workgroup's slot.  Most in LDS first; the core's column pitch is k_jacobi_lds's conflict-free one (16 modulo 32
// elements) whenever the plan fits with it, else N | 1.  A real core always fits (N <= 128: 128 KiB in f64); the last place of the complex
// list keeps W, V and G in the slot at pitch N (a 128 x 128 c64 core alone takes 256 KiB, more than BID_MAX_LDS).
template <typename E>
BatchedPlan<BsvPlace> bsv_plan(int m, int n) {
    using F = BatchedFamily<E>;
    const int M = std::max(m, n), N = std::min(m, n);
    const int pad = ((N + 15) / 32) * 32 + 16, odd = N | 1;
    const BsvPlace places[] = {{true, true, true, pad},   {true, true, true, odd},   {false, true, true, pad}, {false, true, true, odd},
                               {false, false, true, pad}, {false, false, true, odd}, {false, false, false, N}};
    return batched_first_fit(places, is_real_elem<E> ? 6 : 7, [&](BsvPlace p) { return F::svd_lds_bytes(M, N, p); },
                             [&](BsvPlace p) { return F::svd_ws_elems(M, N, p) * sizeof(E); }, "svd_rank_batched");
}

template <typename E>
constexpr const char *brc_what[3] = {"lowrank_recompress_batched", is_real_elem<E> ? "lowrank_recompress_tall_batched" : "lowrank_recompress_tall_complex_batched",
                                     is_real_elem<E> ? "lowrank_recompress_large_batched" : "lowrank_recompress_complex_large_batched"};

// recompression: the two working copies Wl (m x K), Wr (n x K) and the rotations J (K x K) by bsv_plan's rule next to the core; a copy that
// does not fit goes to the workgroup's slot, the larger copy first.  A complex core that does not fit in LDS at either pitch (c64,
// K >= 100) goes to the slot with everything else, at pitch K: the last place.
// BRC_TALL: m <= BRT_H is the small plan; above it the stage copies are always in the slot (the copy of left never in LDS), Wr, J and G by
// the small rule.  BRC_LARGE: n <= BRT_H is the tall plan byte for byte; above it the right factor's stage copies are always in the slot,
// the left factor's copy by the small rule for m <= BRT_H and staged above it (the first two places then repeat the next two: first fit
// skips nothing), J and G by the small rule.
template <typename E>
BatchedPlan<BrcPlace> brc_plan(int form, int m, int n, int K) {
    using F = BatchedFamily<E>;
    if (form == BRC_LARGE && n <= BRT_H) form = BRC_TALL;
    if (form == BRC_TALL && m <= BRT_H) form = BRC_SMALL;
    const int pad = ((K + 15) / 32) * 32 + 16, odd = K | 1;
    const bool big_l = m >= n;   // small: the copy that leaves LDS first
    const bool l = m <= BRT_H;   // large: the only copy that may sit in LDS
    const BrcPlace small[] = {{true, true, true, true, pad},     {true, true, true, true, odd},    {!big_l, big_l, true, true, pad},
                              {!big_l, big_l, true, true, odd},  {false, false, true, true, pad},  {false, false, true, true, odd},
                              {false, false, false, true, pad},  {false, false, false, true, odd}, {false, false, false, false, K}};
    const BrcPlace tall[] = {{false, true, true, true, pad},  {false, true, true, true, odd},   {false, false, true, true, pad}, {false, false, true, true, odd},
                             {false, false, false, true, pad}, {false, false, false, true, odd}, {false, false, false, false, K}};
    const BrcPlace large[] = {{l, false, true, true, pad},     {l, false, true, true, odd},      {false, false, true, true, pad}, {false, false, true, true, odd},
                              {false, false, false, true, pad}, {false, false, false, true, odd}, {false, false, false, false, K}};
    const BrcPlace *places = form == BRC_LARGE ? large : form == BRC_TALL ? tall : small;
    const size_t count = (form == BRC_SMALL ? 9 : 7) - (is_real_elem<E> ? 1 : 0);
    return batched_first_fit(places, count, [&](BrcPlace p) { return F::recompress_lds_bytes(m, n, K, p); },
                             [&](BrcPlace p) { return F::recompress_ws_elems(form, m, n, K, p) * sizeof(E); }, brc_what<E>[form]);
}

// sketched column ID: W (l x n) in LDS when it fits next to the chunk images, else in the workgroup's slot
template <typename E>
BatchedPlan<bool> bsi_plan(int l, int n) {
    return batched_lds_or_ws([&](bool w_lds) { return BatchedFamily<E>::sketch_id_lds_bytes(l, n, w_lds); }, (size_t)l * (size_t)n * sizeof(E),
                             "sketch_column_id_rank_batched");
}

template <typename E>
constexpr const char *brs_what = is_real_elem<E> ? "sketch_range_step_batched" : "sketch_range_step_complex_batched";

// range step: the working copy of Y^T (n x l) in LDS when it fits next to the chunk images, else in the workgroup's slot behind Q (complex:
// conj(Q)), which is always there (the projection reads it through the chunk staging, as the sketch reads omega)
template <typename E>
BatchedPlan<bool> brs_plan(int l, int n) {
    const bool places[] = {true, false};
    return batched_first_fit(places, [&](bool w_lds) { return BatchedFamily<E>::range_step_lds_bytes(l, n, w_lds); },
                             [&](bool w_lds) { return (size_t)(w_lds ? 1 : 2) * (size_t)l * (size_t)n * sizeof(E); }, brs_what<E>);
}

// ---- the launchers --------------------------------------------------------------------------------------------------------------------------

// the two IDs: their plans and kernels are one text for all four element types (batched_stages.hpp)
template <typename E>
void batched_column_id(rc_context *c, Mat<E> a, int64_t abs, int32_t count, int64_t k, double tol, Mat<E> cm, int64_t cbs, Mat<E> z, int64_t zbs,
                       int64_t *col_ind, int64_t *ranks) {
    const int m = (int)a.rows, n = (int)a.cols;
    if (count <= 0) return;
    const auto plan = bid_plan<E>(m, n);
    const auto lch = batched_prepare(c, plan.at ? k_batched_id<E, true> : k_batched_id<E, false>, "column_id_rank_batched", plan.lds, plan.ws, count);
    ProfScope ps(c, "op:batched_column_id%s %dx%d k=%lld count=%d grid=%lld slots=%lld plan=W:%s", is_real_elem<E> ? "" : "<complex>", m, n, (long long)k,
                 (int)count, (long long)lch.grid, (long long)lch.slots, plan.at ? "lds" : "ws");
    lch.launch(a, abs, (int)count, (int)k, tol, cm, cbs, z, zbs, col_ind, ranks, lch.template workspace<E>());
}
template <typename E>
void batched_two_sided_id(rc_context *c, Mat<E> a, int64_t abs, int32_t count, int64_t k, double tol, Mat<E> cm, int64_t cbs, Mat<E> x, int64_t xbs, Mat<E> z,
                          int64_t zbs, int64_t *row_ind, int64_t *col_ind, int64_t *ranks) {
    const int m = (int)a.rows, n = (int)a.cols;
    if (count <= 0) return;
    const auto plan = bts_plan<E>(m, n, (int)k);
    const auto lch = batched_prepare(c, plan.at ? k_batched_two_sided<E, true> : k_batched_two_sided<E, false>, "two_sided_id_rank_batched", plan.lds, plan.ws,
                                     count);
    ProfScope ps(c, "op:batched_two_sided_id%s %dx%d k=%lld count=%d grid=%lld slots=%lld plan=W:%s", is_real_elem<E> ? "" : "<complex>", m, n, (long long)k,
                 (int)count, (long long)lch.grid, (long long)lch.slots, plan.at ? "lds" : "ws");
    lch.launch(a, abs, (int)count, (int)k, tol, cm, cbs, x, xbs, z, zbs, row_ind, col_ind, ranks, lch.template workspace<E>());
}

template <typename E>
void batched_svd(rc_context *c, Mat<E> a, int64_t abs, int32_t count, int64_t k, double tol, Mat<E> u, int64_t ubs, real_t<E> *s, Mat<E> vt, int64_t vbs,
                 int64_t *ranks) {
    const int m = (int)a.rows, n = (int)a.cols;
    if (count <= 0) return;
    const bool wide = m < n;
    const auto plan = bsv_plan<E>(m, n);
    const BsvPlace at = plan.at;
    const auto lch = batched_prepare(c, BatchedFamily<E>::svd_kernel(at), "svd_rank_batched", plan.lds, plan.ws, count);
    ProfScope ps(c, "op:batched_svd%s %dx%d k=%lld count=%d grid=%lld slots=%lld plan=W:%s,V:%s,G:%s,ld=%d", is_real_elem<E> ? "" : "<complex>", m, n,
                 (long long)k, (int)count, (long long)lch.grid, (long long)lch.slots, at.w ? "lds" : "ws", at.v ? "lds" : "ws", at.g ? "lds" : "ws", at.ld);
    // the work orientation's U (M x k) and V^H (k x N): u and vt, or for a wide matrix the plain transposed views vt^T and u^T
    const Mat<E> uo = wide ? vt.t() : u, vo = wide ? u.t() : vt;
    const int64_t uobs = wide ? vbs : ubs, vobs = wide ? ubs : vbs;
    lch.launch(a, abs, (int)count, (int)k, tol, uo, uobs, vo, vobs, s, ranks, lch.template workspace<E>(), c->health_word(), at.ld);
}

// One kernel per entry point: the plan only moves base pointers and pitches, and no sum depends on a pitch, so it cannot change a block's
// bits.  BRC_TALL (rc_lowrank_recompress_tall_*batched_*): the same arguments and, for m <= 512, the same plan and the same work per block.
// Above it a slot holds every stage's copy (about 90 MiB at 65536 x 128 in f64, 173 MiB in c64), so the grid is bounded a second time, by
// brt_grid_cap: few workgroups run there.  BRC_LARGE (rc_lowrank_recompress_large_batched_*, rc_lowrank_recompress_complex_large_batched_*):
// for n <= 512 the tall call's plan and instance, so its bits; above it the slot holds the right factor's stages too and the same bound
// applies to the whole slot.
template <typename E, int FORM>
void brc_launch(rc_context *c, Mat<E> left, int64_t lbs, Mat<E> mid, int64_t mbs, const real_t<E> *s, int64_t s_stride, Mat<E> right, int64_t rbs,
                const int64_t *in_ranks, int32_t count, int64_t k, double tol, Mat<E> u, int64_t ubs, real_t<E> *s_out, Mat<E> vt, int64_t vbs, int64_t *ranks) {
    using F = BatchedFamily<E>;
    const int m = (int)left.rows, n = (int)right.cols, K = (int)left.cols;
    if (count <= 0) return;
    const auto plan = brc_plan<E>(FORM, m, n, K);
    const BrcPlace at = plan.at;
    auto lch = batched_prepare(c, F::template recompress_kernel<FORM>(m, n), brc_what<E>[FORM], plan.lds, plan.ws, count);
    char stages[48] = "";
    if (FORM != BRC_SMALL) {
        lch.grid = brt_grid_cap(lch.grid, plan.ws);
        lch.slots = brt_grid_cap(lch.slots, plan.ws);
        // inside plan=: the label keeps the family's fields
        if (FORM == BRC_LARGE) snprintf(stages, sizeof stages, "stages=%d,rstages=%d,", brt_stages(m, K), brt_stages(n, K));
        else snprintf(stages, sizeof stages, "stages=%d,", brt_stages(m, K));
    }
    ProfScope ps(c, "op:batched_recompress%s%s %dx%d k=%d count=%d grid=%lld slots=%lld plan=%sL:%s,R:%s,V:%s,G:%s,ld=%d,kk=%d%s%s",
                 FORM == BRC_LARGE ? "_large" : FORM == BRC_TALL ? "_tall" : "", is_real_elem<E> ? "" : "<complex>", m, n, K, (int)count, (long long)lch.grid,
                 (long long)lch.slots, stages, at.l ? "lds" : "ws", at.r ? "lds" : "ws", at.v ? "lds" : "ws", at.g ? "lds" : "ws", at.ld,
                 (int)std::min<int64_t>(k, K), mid.p ? ",mid" : "", s ? ",s" : "");
    typename F::RecompressArgs a;
    a.left = left; a.mid = mid; a.right = right; a.u = u; a.vt = vt;
    a.lbs = lbs; a.mbs = mbs; a.rbs = rbs; a.ubs = ubs; a.vbs = vbs; a.s_stride = s_stride;
    a.s = s; a.in_ranks = in_ranks; a.s_out = s_out; a.ranks = ranks;
    a.ws = lch.template workspace<E>();
    a.health = c->health_word();
    a.tol = tol; a.count = (int)count; a.k = (int)std::min<int64_t>(k, K); a.ldg = at.ld;
    a.l_lds = at.l; a.r_lds = at.r; a.v_lds = at.v;
    if constexpr (!is_real_elem<E>) a.g_lds = at.g;
    lch.launch(a);
}
template <typename E>
void batched_lowrank_recompress(rc_context *c, Mat<E> left, int64_t lbs, Mat<E> mid, int64_t mbs, const real_t<E> *s, int64_t s_stride, Mat<E> right,
                                int64_t rbs, const int64_t *in_ranks, int32_t count, int64_t k, double tol, Mat<E> u, int64_t ubs, real_t<E> *s_out, Mat<E> vt,
                                int64_t vbs, int64_t *ranks) {
    brc_launch<E, BRC_SMALL>(c, left, lbs, mid, mbs, s, s_stride, right, rbs, in_ranks, count, k, tol, u, ubs, s_out, vt, vbs, ranks);
}
template <typename E>
void batched_lowrank_recompress_tall(rc_context *c, Mat<E> left, int64_t lbs, Mat<E> mid, int64_t mbs, const real_t<E> *s, int64_t s_stride, Mat<E> right,
                                     int64_t rbs, const int64_t *in_ranks, int32_t count, int64_t k, double tol, Mat<E> u, int64_t ubs, real_t<E> *s_out,
                                     Mat<E> vt, int64_t vbs, int64_t *ranks) {
    brc_launch<E, BRC_TALL>(c, left, lbs, mid, mbs, s, s_stride, right, rbs, in_ranks, count, k, tol, u, ubs, s_out, vt, vbs, ranks);
}
template <typename E>
void batched_lowrank_recompress_large(rc_context *c, Mat<E> left, int64_t lbs, Mat<E> mid, int64_t mbs, const real_t<E> *s, int64_t s_stride, Mat<E> right,
                                      int64_t rbs, const int64_t *in_ranks, int32_t count, int64_t k, double tol, Mat<E> u, int64_t ubs, real_t<E> *s_out,
                                      Mat<E> vt, int64_t vbs, int64_t *ranks) {
    brc_launch<E, BRC_LARGE>(c, left, lbs, mid, mbs, s, s_stride, right, rbs, in_ranks, count, k, tol, u, ubs, s_out, vt, vbs, ranks);
}

// the tall and large launchers' plans as numbers (the four rc_lowrank_recompress_*_batched_plan entry points): the stages of the staged
// factors at inner width K, bytes of one slot, and the grid brt_grid_cap leaves of `resident` workgroups
template <typename E>
void batched_lowrank_recompress_tall_plan(int64_t m, int64_t n, int64_t K, int64_t resident, int64_t *stages, int64_t *slot_bytes, int64_t *grid) {
    const size_t ws = brc_plan<E>(BRC_TALL, (int)m, (int)n, (int)K).ws;
    *stages = brt_stages((int)m, (int)K);
    *slot_bytes = (int64_t)ws;
    *grid = brt_grid_cap(resident, ws);
}
template <typename E>
void batched_lowrank_recompress_large_plan(int64_t m, int64_t n, int64_t K, int64_t resident, int64_t *stages_left, int64_t *stages_right, int64_t *slot_bytes,
                                           int64_t *grid) {
    const size_t ws = brc_plan<E>(BRC_LARGE, (int)m, (int)n, (int)K).ws;
    *stages_left = brt_stages((int)m, (int)K);
    *stages_right = brt_stages((int)n, (int)K);
    *slot_bytes = (int64_t)ws;
    *grid = brt_grid_cap(resident, ws);
}

// The plan only moves W's base pointer and pitch, so it cannot change a block's bits.  Four instances of the kernel, by the index of a and
// of omega that the staging loads' lanes run along; each element (complex: each component) of Y is summed in the same order in all four.
// The label carries the launched instance's scratch bytes per thread (the f64 instances sit at the register bound of two waves per SIMD,
// so a compiler that spills more shows up in every profile and in tools/batched_sketch_id_bench.py).
template <typename E>
void batched_sketch_column_id(rc_context *c, Mat<E> a, int64_t abs, Mat<E> omega, int64_t obs, int32_t count, int64_t kk, double tol, Mat<E> y, int64_t ybs,
                              Mat<E> cm, int64_t cbs, Mat<E> z, int64_t zbs, int64_t *col_ind, int64_t *ranks) {
    using F = BatchedFamily<E>;
    const int m = (int)a.rows, n = (int)a.cols, l = (int)omega.rows;
    if (count <= 0) return;
    const auto plan = bsi_plan<E>(l, n);
    // the lanes of the staging loads along the smaller stride of a and of omega (bid_load's rule for a)
    const auto lch = batched_prepare(c, F::sketch_id_kernel(a.rs <= a.cs, omega.rs < omega.cs), "sketch_column_id_rank_batched", plan.lds, plan.ws, count);
    ProfScope ps(c, "op:batched_sketch_id%s %dx%d k=%lld count=%d grid=%lld slots=%lld plan=W:%s,l=%d,rows=%d,cols=%d,scratch=%d", is_real_elem<E> ? "" : "_c", m,
                 n, (long long)kk, (int)count, (long long)lch.grid, (long long)lch.slots, plan.at ? "lds" : "ws", l, BSI_ROWS, BSI_COLS, lch.scratch);
    typename F::SketchIdArgs g;
    g.a = a; g.omega = omega; g.y = y; g.c = cm; g.z = z;
    g.abs = abs; g.obs = obs; g.ybs = ybs; g.cbs = cbs; g.zbs = zbs;
    g.col_ind = col_ind; g.ranks = ranks;
    g.ws = lch.template workspace<E>();
    g.tol = tol; g.count = (int)count; g.kk = (int)kk; g.w_lds = plan.at;
    lch.launch(g);
}

// The plan only moves the working copy's base pointer and pitch, and the four instances (by the index of a and of omega that the sketch's
// staging loads run along; the projection's run along the other index of a and along n in Q) sum every element in the same order, so
// neither can change a block's bits.  The label carries the scratch bytes per thread like the sketched ID's, and the complex one p_conj.
template <typename E>
void batched_sketch_range_step(rc_context *c, Mat<E> a, int64_t abs, Mat<E> omega, int64_t obs, int32_t count, Mat<E> y, int64_t ybs, Mat<E> q, int64_t qbs,
                               Mat<E> p, int64_t pbs, int64_t *ranks, bool p_conj) {
    using F = BatchedFamily<E>;
    const int m = (int)a.rows, n = (int)a.cols, l = (int)omega.rows;
    if (count <= 0) return;
    const auto plan = brs_plan<E>(l, n);
    const auto lch = batched_prepare(c, F::range_step_kernel(a.rs <= a.cs, omega.rs < omega.cs), brs_what<E>, plan.lds, plan.ws, count);
    char conj[16] = "";
    if (!is_real_elem<E>) snprintf(conj, sizeof conj, "conj=%d,", p_conj ? 1 : 0);
    ProfScope ps(c, "op:batched_range_step%s %dx%d l=%d count=%d grid=%lld slots=%lld plan=W:%s,Q:ws,rows=%d,cols=%d,%sscratch=%d", is_real_elem<E> ? "" : "_c",
                 m, n, l, (int)count, (long long)lch.grid, (long long)lch.slots, plan.at ? "lds" : "ws", BSI_ROWS, BSI_COLS, conj, lch.scratch);
    typename F::RangeStepArgs g;
    g.a = a; g.omega = omega; g.y = y; g.q = q; g.p = p;
    g.abs = abs; g.obs = obs; g.ybs = ybs; g.qbs = qbs; g.pbs = pbs;
    g.ranks = ranks;
    g.ws = lch.template workspace<E>();
    g.slot = plan.ws / sizeof(E);
    g.count = (int)count; g.w_lds = plan.at;
    if constexpr (!is_real_elem<E>) g.p_conj = p_conj;
    lch.launch(g);
}

// What a translation unit instantiates for its two element types, in three groups.  The order, group by group, launcher by launcher and E1
// before E2, is the order in which the kernels reach the code object, and the compiler's output for a kernel is not independent of it (the
// real two-sided kernels move): each file keeps the order it had and compares its device assembly after any change (tools/device_asm_diff.py).
#define RC_RECOMPRESS_PARAMS(E) \
    rc_context *, Mat<E>, int64_t, Mat<E>, int64_t, const real_t<E> *, int64_t, Mat<E>, int64_t, const int64_t *, int32_t, int64_t, double, Mat<E>, int64_t, \
        real_t<E> *, Mat<E>, int64_t, int64_t *
#define RC_INSTANTIATE_BATCHED_SKETCH(E1, E2) \
    template void batched_sketch_range_step<E1>(rc_context *, Mat<E1>, int64_t, Mat<E1>, int64_t, int32_t, Mat<E1>, int64_t, Mat<E1>, int64_t, Mat<E1>, int64_t, int64_t *, bool); \
    template void batched_sketch_range_step<E2>(rc_context *, Mat<E2>, int64_t, Mat<E2>, int64_t, int32_t, Mat<E2>, int64_t, Mat<E2>, int64_t, Mat<E2>, int64_t, int64_t *, bool); \
    template void batched_sketch_column_id<E1>(rc_context *, Mat<E1>, int64_t, Mat<E1>, int64_t, int32_t, int64_t, double, Mat<E1>, int64_t, Mat<E1>, int64_t, Mat<E1>, int64_t, int64_t *, int64_t *); \
    template void batched_sketch_column_id<E2>(rc_context *, Mat<E2>, int64_t, Mat<E2>, int64_t, int32_t, int64_t, double, Mat<E2>, int64_t, Mat<E2>, int64_t, Mat<E2>, int64_t, int64_t *, int64_t *);
#define RC_INSTANTIATE_BATCHED_RECOMPRESS(E1, E2) \
    template void batched_lowrank_recompress<E1>(RC_RECOMPRESS_PARAMS(E1)); \
    template void batched_lowrank_recompress<E2>(RC_RECOMPRESS_PARAMS(E2)); \
    template void batched_lowrank_recompress_tall<E1>(RC_RECOMPRESS_PARAMS(E1)); \
    template void batched_lowrank_recompress_tall<E2>(RC_RECOMPRESS_PARAMS(E2)); \
    template void batched_lowrank_recompress_large<E1>(RC_RECOMPRESS_PARAMS(E1)); \
    template void batched_lowrank_recompress_large<E2>(RC_RECOMPRESS_PARAMS(E2)); \
    template void batched_lowrank_recompress_tall_plan<E1>(int64_t, int64_t, int64_t, int64_t, int64_t *, int64_t *, int64_t *); \
    template void batched_lowrank_recompress_tall_plan<E2>(int64_t, int64_t, int64_t, int64_t, int64_t *, int64_t *, int64_t *); \
    template void batched_lowrank_recompress_large_plan<E1>(int64_t, int64_t, int64_t, int64_t, int64_t *, int64_t *, int64_t *, int64_t *); \
    template void batched_lowrank_recompress_large_plan<E2>(int64_t, int64_t, int64_t, int64_t, int64_t *, int64_t *, int64_t *, int64_t *);
#define RC_INSTANTIATE_BATCHED_ID_SVD(E1, E2) \
    template void batched_column_id<E1>(rc_context *, Mat<E1>, int64_t, int32_t, int64_t, double, Mat<E1>, int64_t, Mat<E1>, int64_t, int64_t *, int64_t *); \
    template void batched_column_id<E2>(rc_context *, Mat<E2>, int64_t, int32_t, int64_t, double, Mat<E2>, int64_t, Mat<E2>, int64_t, int64_t *, int64_t *); \
    template void batched_two_sided_id<E1>(rc_context *, Mat<E1>, int64_t, int32_t, int64_t, double, Mat<E1>, int64_t, Mat<E1>, int64_t, Mat<E1>, int64_t, int64_t *, int64_t *, int64_t *); \
    template void batched_two_sided_id<E2>(rc_context *, Mat<E2>, int64_t, int32_t, int64_t, double, Mat<E2>, int64_t, Mat<E2>, int64_t, Mat<E2>, int64_t, int64_t *, int64_t *, int64_t *); \
    template void batched_svd<E1>(rc_context *, Mat<E1>, int64_t, int32_t, int64_t, double, Mat<E1>, int64_t, real_t<E1> *, Mat<E1>, int64_t, int64_t *); \
    template void batched_svd<E2>(rc_context *, Mat<E2>, int64_t, int32_t, int64_t, double, Mat<E2>, int64_t, real_t<E2> *, Mat<E2>, int64_t, int64_t *);

}  // namespace rc
