// C ABI of librusty_compression_amd + the host-side composition of the hot path.
// Every exported function cites (in include/rusty_compression_amd.h) the
// reference trait method it replaces; the compositions below follow the
// reference's call sequences with GEMMs instead of gemv
// loops and one batched triangular solve instead of per-column ?trtrs calls.
#include "rc_common.hpp"

#include <unistd.h>

#include <atomic>
#include <chrono>

#include <algorithm>
#include <cmath>

using namespace rc;

// ===========================================================================
// context / arena
// ===========================================================================
static constexpr size_t kAlign = 256;

void rc_context::retire_arena() {
    if (arena) {
        if (live_graphs > 0) retired.push_back(arena);
        else (void)hipFree(arena);
    }
    arena = nullptr;
    arena_size = 0;
}

void rc_context::swap_arena() {
    std::swap(arena, aux_arena.base);
    std::swap(arena_size, aux_arena.size);
    std::swap(arena_off, aux_arena.off);
    std::swap(arena_high, aux_arena.high);
    std::swap(overflow, aux_arena.overflow);
}

// the active arena (the fields of the context), whose users were issued on `st`
// RC_DEBUG_POISON_WORKSPACE=1 (diagnostic, tests/test_gpu_parity.py): workspace memory that is new to a context is filled with
// small integers (every 32-bit word = 3) before it is handed out -- what recycled allocator memory tends to look like.  Results
// must not depend on it: this is how the fused Jacobi's uncleared hand-over words were pinned down.
__global__ void k_poison_words(unsigned *p, size_t n, unsigned v) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) p[i] = v;
}
static void poison_fresh(void *p, size_t bytes, hipStream_t st) {
    // 1 (2 and above: verbose): every word 3; 3: every word 0xffffffff (a NaN in f32 and f64, -1 as an index)
    static const int level = env_int("RC_DEBUG_POISON_WORKSPACE", 0);
    if (!level || !p || bytes < 4) return;
    if (level > 1) fprintf(stderr, "poison %p %zu bytes\n", p, bytes);
    hipLaunchKernelGGL(k_poison_words, dim3(1024), dim3(256), 0, st, static_cast<unsigned *>(p), bytes / 4, level == 3 ? 0xffffffffu : 3u);
}

static void reset_active_arena(rc_context *c, hipStream_t st) {
    if (!c->overflow.empty()) {
        // the previous call outgrew the arena: rebuild it once, big enough
        (void)hipStreamSynchronize(st);
        for (void *p : c->overflow) (void)hipFree(p);
        c->overflow.clear();
        size_t want = c->arena_high + c->arena_high / 4 + (1u << 20);
        c->retire_arena();
        if (hipMalloc(reinterpret_cast<void **>(&c->arena), want) == hipSuccess) { c->arena_size = want; poison_fresh(c->arena, want, st); }
    }
    c->arena_off = 0;
    c->arena_high = 0;
}

void rc_context::reset_arena() {
    if (aux_stream) {  // the side arena obeys the same rules (its work was joined into `stream` by the call that used it)
        swap_arena();
        reset_active_arena(this, aux_stream);
        swap_arena();
    }
    reset_active_arena(this, stream);
}

void *rc_context::alloc_bytes(size_t bytes) {
    bytes = (bytes + kAlign - 1) / kAlign * kAlign;
    if (bytes == 0) bytes = kAlign;
    void *p = nullptr;
    if (arena_off + bytes <= arena_size) {
        p = arena + arena_off;
    } else {
        RC_REQUIRE(!capturing, RC_RUNTIME_ERROR,
                   "workspace arena too small during hipGraph capture: run the same call once eagerly first (or rc_reserve_workspace)");
        RC_HIP(hipMalloc(&p, bytes));
        overflow.push_back(p);
        poison_fresh(p, bytes, stream);
    }
    arena_off += bytes;
    arena_high = std::max(arena_high, arena_off);
    return p;
}

void rc_context::reserve(size_t bytes) {
    if (bytes <= arena_size) return;
    RC_HIP(hipStreamSynchronize(stream));
    retire_arena();
    RC_HIP(hipMalloc(reinterpret_cast<void **>(&arena), bytes));
    arena_size = bytes;
    poison_fresh(arena, bytes, stream);
}

hipEvent_t rc_context::prof_event() {
    if (!prof_free.empty()) { hipEvent_t e = prof_free.back(); prof_free.pop_back(); return e; }
    hipEvent_t e = nullptr;
    (void)hipEventCreate(&e);
    return e;
}

void rc_context::prof_resolve() {
    if (prof_pending.empty()) return;
    (void)hipStreamSynchronize(stream);
    for (auto &p : prof_pending) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, p.beg, p.end) == hipSuccess) {
            auto &a = prof_acc[p.name];
            a.ms += ms;
            a.calls += 1;
        }
        prof_free.push_back(p.beg);
        prof_free.push_back(p.end);
    }
    prof_pending.clear();
}

int *rc_context::health_word() {
    if (!health) {
        RC_HIP(hipMalloc(reinterpret_cast<void **>(&health), sizeof(int)));
        const int zero = 0;
        RC_HIP(hipMemcpy(health, &zero, sizeof(int), hipMemcpyHostToDevice));  // blocking, complete before the first kernel that ORs into it
    }
    return health;
}

unsigned *rc_context::epoch_word() {
    if (!epoch) {
        RC_HIP(hipMalloc(reinterpret_cast<void **>(&epoch), sizeof(unsigned)));
        // a different, non-zero starting epoch for every context of the process (and of other processes): the records and tagged
        // words of the fused Jacobi are keyed by it, and workspace memory travels between contexts through the allocator
        static std::atomic<unsigned> serial{0};
        const unsigned long long mix = (unsigned long long)std::chrono::steady_clock::now().time_since_epoch().count() * 0x9e3779b97f4a7c15ull ^
                                       (unsigned long long)(uintptr_t)this * 0xd1342543de82ef95ull ^ ((unsigned long long)(++serial) << 40) ^
                                       (unsigned long long)getpid() * 0xff51afd7ed558ccdull;
        unsigned e0 = (unsigned)(mix >> 29) & 0x7fffffu;  // 23 bits: far from the 24-bit wrap
        if (e0 == 0) e0 = 1;
        RC_HIP(hipMemcpy(epoch, &e0, sizeof(unsigned), hipMemcpyHostToDevice));
    }
    return epoch;
}

void rc_context::release_all() {
    (void)hipStreamSynchronize(stream);
    if (health) (void)hipFree(health);
    health = nullptr;
    if (epoch) (void)hipFree(epoch);
    epoch = nullptr;
    prof_resolve();
    for (hipEvent_t e : prof_free) (void)hipEventDestroy(e);
    prof_free.clear();
    for (void *p : overflow) (void)hipFree(p);
    overflow.clear();
    for (void *p : retired) (void)hipFree(p);
    retired.clear();
    if (arena) (void)hipFree(arena);
    arena = nullptr;
    arena_size = 0;
    if (aux_stream) (void)hipStreamSynchronize(aux_stream);
    for (void *p : aux_arena.overflow) (void)hipFree(p);
    aux_arena.overflow.clear();
    if (aux_arena.base) (void)hipFree(aux_arena.base);
    aux_arena = ArenaState();
    if (fork_ev) (void)hipEventDestroy(fork_ev);
    if (join_ev) (void)hipEventDestroy(join_ev);
    if (aux_stream) (void)hipStreamDestroy(aux_stream);
    fork_ev = join_ev = nullptr;
    aux_stream = nullptr;
    if (pinned) (void)hipHostFree(pinned);
    pinned = nullptr;
    if (sync_ev) (void)hipEventDestroy(sync_ev);
    sync_ev = nullptr;
}

// Column-major temporaries.  The lone calls' (tmp_colmajor) have an even pitch, which is all the GEMM's 2-element staging loads ask for.
// The batch's working copy (tmp_colmajor_pitch4, rc_batch.hip) pads the pitch to a multiple of 4 elements: its columns are then 16-byte
// aligned at every m, which is what the blocked QRCP's vector loads ask for (BlockedQrcpJob::vec_ok in k_qrb_step_c, k_qrb_vta).
namespace rc {
template <typename T>
Mat<T> tmp_colmajor_pitch4(rc_context *c, int64_t rows, int64_t cols) {
    int64_t ld = even_ld(std::max<int64_t>(rows, 1));
    if (ld % 4) ld += 4 - ld % 4;
    return colmajor(c->alloc<T>((size_t)ld * std::max<int64_t>(cols, 1)), rows, cols, ld);
}
template Mat<double> tmp_colmajor_pitch4<double>(rc_context *, int64_t, int64_t);
template Mat<float> tmp_colmajor_pitch4<float>(rc_context *, int64_t, int64_t);
}  // namespace rc

namespace {

template <typename T>
Mat<T> tmp_colmajor(rc_context *c, int64_t rows, int64_t cols) {
    int64_t ld = even_ld(std::max<int64_t>(rows, 1));
    return colmajor(c->alloc<T>((size_t)ld * std::max<int64_t>(cols, 1)), rows, cols, ld);
}
template <typename T>
Mat<T> tmp_rowmajor(rc_context *c, int64_t rows, int64_t cols) {
    int64_t ld = even_ld(std::max<int64_t>(cols, 1));
    return rowmajor(c->alloc<T>((size_t)ld * std::max<int64_t>(rows, 1)), rows, cols, ld);
}

void check_view(const rc_matrix &m, const char *name, bool allow_null = false) {
    RC_REQUIRE(m.rows >= 0 && m.cols >= 0, RC_INVALID_ARGUMENT, "%s: negative extent", name);
    if (!allow_null) RC_REQUIRE(m.data != nullptr || m.rows == 0 || m.cols == 0, RC_INVALID_ARGUMENT, "%s: null data", name);
}

// ===========================================================================
// compositions (templated on the scalar type)
// ===========================================================================

__global__ void k_or_flag(int *dst, const int *src) {
    if (threadIdx.x == 0 && blockIdx.x == 0 && *src) atomicOr(dst, *src);
}
// (certificate and health words are set by a kernel of the library on the context's stream, not by hipMemset*: with 16 contexts
// replaying graphs at once, words cleared through the runtime's memset path were read back as byte patterns -- 0x01010101,
// 0x02020202, 0x9f9f9f9f, the same on every context of a round -- although every output was bit-identical to the eager run)
__global__ void k_set_word(int *dst, int v) {
    if (threadIdx.x == 0 && blockIdx.x == 0) *dst = v;
}

// Runs `fast(flag)` (which ORs failure bits into the device int `flag`) and reports whether
// its result may be kept.  Outside graph capture the flag is read back (one small sync) so
// the caller can fall back; during capture the bits go to the context's health word instead.
// RC_DEBUG_MEMSET_PATH (diagnostic, bit mask): 1 = the certificate word is cleared by hipMemsetAsync again (a memset NODE when the call
// is captured), 2 = rc_get_health reads and clears through the null stream (pageable hipMemcpy + hipMemset) again -- the two round-2
// code paths, switchable one at a time so that tools/rsvd_repeat_diag.py shows which of them delivers the byte patterns.
static int debug_memset_path() {
    static const int v = env_int("RC_DEBUG_MEMSET_PATH", 0);
    return v;
}

template <typename F>
bool run_certified(rc_context *c, F &&fast) {
    int *flag = c->alloc<int>(1);
    if (debug_memset_path() & 1) RC_HIP(hipMemsetAsync(flag, 0, sizeof(int), c->stream));
    else hipLaunchKernelGGL(k_set_word, dim3(1), dim3(64), 0, c->stream, flag, 0);
    fast(flag);
    if (c->capturing) {
        hipLaunchKernelGGL(k_or_flag, dim3(1), dim3(64), 0, c->stream, c->health_word(), flag);
        return true;
    }
    int h = 0;
    read_back(c, flag, &h, 1);
    return h == 0;
}

// Q from a ?geqp3-format factorization goes into q where q is column-major with room for whole columns, otherwise into a column-major
// temporary that is then copied out: q_target names the matrix to form Q in, q_deliver copies it out if it was the temporary.
template <typename T>
Mat<T> q_target(rc_context *c, Mat<T> q) {
    return q.empty() || (q.rs == 1 && q.cs >= q.rows) ? q : tmp_colmajor<T>(c, q.rows, q.cols);
}
template <typename T>
void q_deliver(rc_context *c, Mat<T> qw, Mat<T> q) {
    if (qw.p != q.p) copy_mat(c, qw, q);
}
// q = H_0 ... H_{k-1} [I ; 0], reflector j in column ind[j] of w
template <typename T>
void form_q_into(rc_context *c, Mat<T> w, const int64_t *ind, const T *tau, int64_t k, Mat<T> q) {
    if (q.empty()) return;
    Mat<T> qw = q_target(c, q);
    form_q(c, w, ind, tau, k, qw);
    q_deliver(c, qw, q);
}

// Pivoted QR of the column-major working matrix w (destroyed).
//   q: m x k (may be empty to skip), r: k x n (may be empty), ind: n, k <= min(m, n)
// Tall-skinny inputs take the CholeskyQR2 + LDS-QRCP + sign-fix path (kernels_tsqr.hip) and
// fall back to the Householder chain when its certificate fails (cond(w)^2 eps not << 1).
// keep_w: w (any layout) must survive -- the tall-skinny path and the cooperative short-wide kernel only READ their input, so
// they run on it where it lies; every other path gets a column-major working copy first (B = Q^H A is shared by the two
// consumers of rc_rsvd_id: the copy, one pass over B per compression, is only taken when a fallback needs it).
template <typename T>
void qrcp_core(rc_context *c, Mat<T> w, int64_t k, bool pivot, Mat<T> q, Mat<T> r, int64_t *ind, bool keep_w = false) {
    const int64_t n = w.cols;
    ArenaMark mark(c);
    if (c->opt_tsqr && k >= 1 && tsqr_supported<T>(w.rows, n)) {
        if (run_certified(c, [&](int *flag) { qrcp_tall_fast<T>(c, w, k, pivot, q, r, ind, flag); })) return;
    }
    static const int direct_ok = env_int("RC_QRCP_KEEP_DIRECT", 1);
    if (keep_w && !(direct_ok && c->opt_wide_coop && pivot && k >= 1 && wide_coop_supported<T>(w.rows, n, c->device))) {
        Mat<T> cp = tmp_colmajor<T>(c, w.rows, n);
        copy_mat(c, w, cp);
        w = cp;
        keep_w = false;
    }
    if (c->opt_wide_coop && pivot && k >= 1 && wide_coop_supported<T>(w.rows, n, c->device)) {
        T *tau = c->alloc<T>((size_t)k);
        Mat<T> wf = tmp_colmajor<T>(c, w.rows, n);
        if (run_certified(c, [&](int *flag) { geqp3_wide_coop<T>(c, w, wf, k, ind, tau, flag); })) {
            if (!r.empty()) extract_r(c, wf, ind, r);
            form_q_into(c, wf, ind, tau, k, q);
            return;
        }
    }
    if (keep_w) {  // the cooperative kernel did not certify (eager mode: fall back on a copy)
        Mat<T> cp = tmp_colmajor<T>(c, w.rows, n);
        copy_mat(c, w, cp);
        w = cp;
    }
    if (c->opt_wide_lazy && pivot && k >= 1 && wide_lazy_supported<T>(w.rows, n)) {
        geqp3_wide_lazy<T>(c, w, k, ind, q, r);
        return;
    }
    T *tau = c->alloc<T>((size_t)std::max<int64_t>(k, 1));
    if (c->opt_blocked && pivot && !c->capturing && geqp3_blocked_supported<T>(w.rows, n, k)) {
        // blocked ?laqps panels; Q comes out of the same job (block reflectors with the panels' T factors)
        Mat<T> qw = q_target(c, q);
        geqp3_blocked<T>(c, w, k, ind, tau, qw);
        if (!r.empty()) extract_r(c, w, ind, r);
        q_deliver(c, qw, q);
        return;
    }
    T *vn = c->alloc<T>((size_t)std::max<int64_t>(2 * n, 1));
    geqp3_inplace(c, w, k, pivot, ind, tau, vn);
    if (!r.empty()) extract_r(c, w, ind, r);
    form_q_into(c, w, ind, tau, k, q);
}

// PivotedQR::pivoted_qr  (/root/reference/src/pivoted_qr.rs:25-31, :81-119)
template <typename T>
void pivoted_qr(rc_context *c, Mat<T> a, Mat<T> q, Mat<T> r, int64_t *ind) {
    const int64_t m = a.rows, n = a.cols, k = q.cols;
    RC_REQUIRE(q.rows == m && r.cols == n && r.rows == k, RC_INVALID_ARGUMENT,
               "pivoted_qr: a %lld x %lld, q %lld x %lld, r %lld x %lld", (long long)m, (long long)n, (long long)q.rows,
               (long long)q.cols, (long long)r.rows, (long long)r.cols);
    RC_REQUIRE(k <= std::min(m, n), RC_INVALID_ARGUMENT, "pivoted_qr: rank %lld exceeds min(m, n)", (long long)k);
    if (n == 0) return;
    ArenaMark mark(c);
    Mat<T> w = tmp_colmajor<T>(c, m, n);  // the reference's F-order working copy (pivoted_qr.rs:28-29)
    // input scale: the copy is 2^-e a, e the exponent of a's largest entry (a device word); R takes 2^e back
    const int *e = input_exponent(c, a);
    copy_mat_scaled(c, a, w, e);
    qrcp_core(c, w, k, true, q, r, ind);
    rescale(c, r, e, 1);
}

// ---- LAPACK granularity (for a maintainer who swaps only the `$qrf` call at /root/reference/src/pivoted_qr.rs:139-172
// and `lax::q` at :104-108, or the `solve_triangular` calls at src/qr.rs:298, :392)
// ?geqp3: a (m x n) is overwritten with LAPACK's output -- the factorization of A P with its columns IN pivoted order: R on and above
// the diagonal of the first kmax rows, the Householder vectors below it in the first kmax columns; jpvt 0-based (device, n), tau
// (device, kmax).  kmax == min(m, n) is ?geqp3; kmax < min(m, n) stops after kmax steps (rows >= kmax of the columns >= kmax are
// then unspecified).
template <typename T>
void lapack_geqp3(rc_context *c, Mat<T> a, int64_t kmax, int64_t *jpvt, T *tau) {
    const int64_t m = a.rows, n = a.cols;
    RC_REQUIRE(kmax >= 0 && kmax <= std::min(m, n), RC_INVALID_ARGUMENT, "geqp3: need 0 <= kmax <= min(m, n)");
    RC_REQUIRE(jpvt != nullptr && (kmax == 0 || tau != nullptr), RC_INVALID_ARGUMENT, "geqp3: null jpvt / tau");
    if (n == 0) return;
    if (kmax == 0 || m == 0) { iota_i64(c, jpvt, n); return; }
    ArenaMark mark(c);
    Mat<T> w = tmp_colmajor<T>(c, m, n);
    const int *e = input_exponent(c, a);  // (input scale, as pivoted_qr)
    copy_mat_scaled(c, a, w, e);
    Mat<T> src = w;
    bool done = false;
    if (c->opt_wide_coop && wide_coop_supported<T>(m, n, c->device)) {
        Mat<T> wf = tmp_colmajor<T>(c, m, n);
        if (run_certified(c, [&](int *flag) { geqp3_wide_coop<T>(c, w, wf, kmax, jpvt, tau, flag); })) { src = wf; done = true; }
    }
    if (!done && c->opt_blocked && !c->capturing && geqp3_blocked_supported<T>(m, n, kmax)) {
        geqp3_blocked<T>(c, w, kmax, jpvt, tau, Mat<T>());
        done = true;
    }
    if (!done) {
        T *vn = c->alloc<T>((size_t)std::max<int64_t>(2 * n, 1));
        geqp3_inplace(c, w, kmax, true, jpvt, tau, vn);
    }
    gather_cols(c, src, jpvt, a);  // a[:, p] = factored column jpvt[p]
    rescale(c, a, e, 1, kmax);     // R (and, kmax < min(m, n), the trailing block) carries 2^e; the reflectors and tau do not
}
// ?orgqr: q (m x k) = H_0 ... H_{k-1} [I; 0] from the reflectors below the diagonal of the first k columns of a (LAPACK format) and tau
template <typename T>
void lapack_orgqr(rc_context *c, Mat<T> a, const T *tau, int64_t k, Mat<T> q) {
    const int64_t m = a.rows;
    RC_REQUIRE(k >= 0 && k <= std::min(m, a.cols) && q.rows == m && q.cols == k, RC_INVALID_ARGUMENT,
               "orgqr: need k <= min(m, n) reflectors in a and q of m x k");
    if (k == 0 || m == 0) return;
    RC_REQUIRE(tau != nullptr, RC_INVALID_ARGUMENT, "orgqr: null tau");
    ArenaMark mark(c);
    int64_t *ident = c->alloc<int64_t>((size_t)k);
    iota_i64(c, ident, k);
    Mat<T> w = a.sub(0, m, 0, k);
    if (!(w.rs == 1 && w.cs >= m)) {  // the kernels address reflector j as a contiguous column
        Mat<T> wc = tmp_colmajor<T>(c, m, k);
        copy_mat(c, w, wc);
        w = wc;
    }
    form_q_into(c, w, ident, tau, k, q);
}

// The tail of svd_core: from the SVD of the core (uc, s, vc) and the orthogonal factor of the tall QR -- qw, or q1 r2i when it
// stayed factored -- to the factors of the matrix itself.  u_in_place (transposed only): the caller had the SVD of the core write
// uc into u's storage, so u = uc needs no copy.  small (factored only): r2i vc (transposed) or r2i uc where a launch before this
// has formed it already (rsvd_id_tails); empty: formed here, by the same body.
template <typename T>
void svd_finish(rc_context *c, bool transposed, bool factored, Mat<T> qw, Mat<T> q1, Mat<T> r2i, Mat<T> uc, Mat<T> vc, const T *s, Mat<T> u, Mat<T> vt,
                bool u_in_place = false, Mat<T> small = Mat<T>()) {
    const int64_t r = uc.rows;
    complete_left_basis(c, uc, s);  // (?gesdd: U stays orthonormal when singular values are zero; no-op otherwise)
    if (factored && small.empty()) {
        small = tmp_colmajor<T>(c, r, r);
        small_tri_product<T>(c, r2i, transposed ? vc : uc, small);
    }
    if (!transposed) {
        // a = Q_w R = (Q_w Uc) S Vc^T
        if (factored) gemm<T>(c, 1, q1, small, 0, u);
        else gemm<T>(c, 1, qw, uc, 0, u);
        copy_mat(c, vc.t(), vt);
    } else {
        // a = L Q_w^T = Uc S (Q_w Vc)^T
        if (!u_in_place) copy_mat(c, uc, u);
        if (factored) gemm_chain<T>(c, 1, small.t(), q1.t(), 0, vt);
        else gemm<T>(c, 1, vc.t(), qw.t(), 0, vt);
    }
}

// ComputeSVD::compute_svd on a working matrix: wt is the TALL orientation
// (M x r column-major, destroyed), i.e. a itself when m >= n, a^T otherwise.
template <typename T>
void svd_core(rc_context *c, Mat<T> wt, bool transposed, Mat<T> u, T *s, Mat<T> vt) {
    const int64_t M = wt.rows, r = wt.cols;
    ArenaMark mark(c);
    Mat<T> core = tmp_colmajor<T>(c, r, r);
    Mat<T> qw, q1, r2i;
    bool done = false;
    const int fold = tsqr_fold();
    if (c->opt_tsqr && tsqr_supported<T>(M, r)) {
        // tall: core = R ; wide: core = L = R^T  (a = L Q_w^T).  Q_w stays factored (Q1 R2^-1): R2^-1 goes into the small
        // factor that multiplies Q_w below, one pass over the tall matrix less
        if (fold) {
            q1 = rowmajor(c->alloc<T>((size_t)M * even_ld(r)), M, r, even_ld(r));
            r2i = rowmajor(c->alloc<T>((size_t)r * even_ld(r)), r, r, even_ld(r));
            done = run_certified(c, [&](int *flag) { tsqr_cholqr2_factored<T>(c, wt, q1, r2i, transposed ? core.t() : core, flag); });
        } else {
            qw = tmp_colmajor<T>(c, M, r);
            done = run_certified(c, [&](int *flag) { tsqr_cholqr2<T>(c, wt, qw, transposed ? core.t() : core, flag); });
        }
    }
    const bool factored = done && fold;
    if (!done) {
        qw = tmp_colmajor<T>(c, M, r);
        int64_t *jp = c->alloc<int64_t>((size_t)std::max<int64_t>(r, 1));
        T *tau = c->alloc<T>((size_t)std::max<int64_t>(r, 1));
        T *vn = c->alloc<T>((size_t)std::max<int64_t>(2 * r, 1));
        geqp3_inplace(c, wt, r, false, jp, tau, vn);
        extract_r(c, wt, jp, transposed ? core.t() : core);
        form_q(c, wt, jp, tau, r, qw);
    }
    Mat<T> vwork = tmp_colmajor<T>(c, r, r), uc = tmp_colmajor<T>(c, r, r), vc = tmp_colmajor<T>(c, r, r);
    jacobi_svd(c, core, vwork, uc, s, vc);
    svd_finish(c, transposed, factored, qw, q1, r2i, uc, vc, s, u, vt);
}

// /root/reference/src/compute_svd.rs:18-27
template <typename T>
void compute_svd(rc_context *c, Mat<T> a, Mat<T> u, T *s, Mat<T> vt) {
    const int64_t m = a.rows, n = a.cols, r = std::min(m, n);
    RC_REQUIRE(u.rows == m && u.cols == r && vt.rows == r && vt.cols == n, RC_INVALID_ARGUMENT,
               "compute_svd: a %lld x %lld needs u %lld x %lld, vt %lld x %lld", (long long)m, (long long)n, (long long)m,
               (long long)r, (long long)r, (long long)n);
    if (r == 0) return;
    ArenaMark mark(c);
    const bool transposed = m < n;
    Mat<T> src = transposed ? a.t() : a;
    Mat<T> wt = tmp_colmajor<T>(c, src.rows, src.cols);
    const int *e = input_exponent(c, a);  // (input scale, as pivoted_qr: s takes 2^e back)
    copy_mat_scaled(c, src, wt, e);
    svd_core(c, wt, transposed, u, s, vt);
    rescale(c, Mat<T>(s, r, 1, 1, 1), e, 1);
}

// Z of a column / row ID in one launch (RC_ID_FUSED)
static int id_fused() {
    static const int fused = env_int("RC_ID_FUSED", 1);
    return fused;
}

// QRTraits::column_id  (/root/reference/src/qr.rs:270-309)
// own_ind: `ind` was written by the library in this call (a pivoted QR's output: a permutation by construction).  A caller's
// `ind` (rc_qr_column_id_*, rc_lq_row_id_*) is checked: entries out of range are skipped, columns of Z no entry names are zero,
// health bit 32 ("Index arrays").
template <typename T>
void qr_column_id(rc_context *c, Mat<T> q, Mat<T> r, const int64_t *ind, Mat<T> cm, Mat<T> z, bool own_ind) {
    const int64_t m = q.rows, k = q.cols, n = r.cols;
    RC_REQUIRE(r.rows == k && cm.rows == m && cm.cols == k && z.rows == k && z.cols == n, RC_INVALID_ARGUMENT,
               "column_id: q %lld x %lld, r %lld x %lld, c %lld x %lld, z %lld x %lld", (long long)m, (long long)k,
               (long long)r.rows, (long long)n, (long long)cm.rows, (long long)cm.cols, (long long)z.rows, (long long)z.cols);
    RC_REQUIRE(k <= n, RC_INVALID_ARGUMENT, "column_id: rank exceeds the number of columns");
    if (n == 0) return;
    ArenaMark mark(c);
    if (id_fused() && k < n) {
        // Z in ONE launch (k_id_z: the chain below with the same arithmetic, every column written to its final place)
        if (own_ind) {
            id_z_from_r(c, r, k, ind, z);
        } else {
            int64_t *inv = c->alloc<int64_t>((size_t)n);
            invert_perm(c, ind, n, inv);
            id_z_from_r_checked(c, r, k, ind, inv, z);
        }
        gemm<T>(c, 1, q, r.sub(0, k, 0, k), 0, cm);
        return;
    }
    int64_t *inv = c->alloc<int64_t>((size_t)n);
    invert_perm(c, ind, n, inv);
    Mat<T> zt = tmp_rowmajor<T>(c, k, n);
    if (k == n) {
        // not rank deficient (qr.rs:274-281): C = Q R, Z = I with the COLINV permutation
        gemm<T>(c, 1, q, r, 0, cm);
        fill_identity(c, zt);
    } else {
        // Z = [I | R11^{-1} R12] (qr.rs:285-301, one batched solve), C = Q R11 (qr.rs:287-288)
        fill_identity(c, zt.sub(0, k, 0, k));
        copy_mat(c, r.sub(0, k, k, n - k), zt.sub(0, k, k, n - k));
        trsm_upper(c, r.sub(0, k, 0, k), zt.sub(0, k, k, n - k));
        gemm<T>(c, 1, q, r.sub(0, k, 0, k), 0, cm);
    }
    gather_cols(c, zt, inv, z);  // apply_permutation(ind, COLINV): out[:, i] = in[:, inv[i]]
}

// LQTraits::row_id (/root/reference/src/qr.rs:363-403) is the column ID of the
// transposed factors: X = Z'^T, R_rows = C'^T with (C', Z') = column_id(Q^T, L^T).
template <typename T>
void lq_row_id(rc_context *c, Mat<T> l, Mat<T> q, const int64_t *ind, Mat<T> x, Mat<T> rrows, bool own_ind) {
    qr_column_id(c, q.t(), l.t(), ind, rrows.t(), x.t(), own_ind);
}

// MaxColNorm (/root/reference/src/random_sampling.rs:184-191) -> device scalar
template <typename T>
void max_col_norm_dev(rc_context *c, Mat<T> y, T *out_dev) {
    ArenaMark mark(c);
    T *ss = c->alloc<T>((size_t)std::max<int64_t>(y.cols, 1));
    col_sumsq(c, y, ss);
    max_sqrt(c, ss, y.cols, out_dev);
}

// ---- the real family's spelling of the primitives rc_dense_shared.hpp is written in (OpView, the range finders, qr_from_range,
// rank_by_tolerance, apply_perm_matrix and their entry points stand there, once for real and complex) ----
template <typename T>
Mat<T> tmp_omega(rc_context *c, int64_t rows, int64_t cols) { return tmp_rowmajor<T>(c, rows, cols); }
template <typename T>
void product(rc_context *c, int alpha, bool adj_a, Mat<T> a, Mat<T> b, int beta, Mat<T> cm) {
    gemm<T>(c, (T)alpha, adj_a ? a.t() : a, b, (T)beta, cm);
}
template <typename T>
void qrcp(rc_context *c, Mat<T> w, int64_t k, Mat<T> q, Mat<T> r, int64_t *ind) { qrcp_core(c, w, k, true, q, r, ind); }

}  // namespace

#include "rc_dense_shared.hpp"

namespace {

// SVDTraits::compute_from_range_estimate (/root/reference/src/svd.rs:171-183): the tall or the wide orientation for svd_core
template <typename T>
void svd_from_range(rc_context *c, Mat<T> range, const OpView<T> &a, Mat<T> u, T *s, Mat<T> vt) {
    const int64_t m = a.rows, n = a.cols, rr = range.cols, r = std::min(rr, n);
    RC_REQUIRE(range.rows == m && u.rows == m && u.cols == r && vt.rows == r && vt.cols == n, RC_INVALID_ARGUMENT,
               "svd_from_range_estimate: shape mismatch");
    ArenaMark mark(c);
    Mat<T> ub = tmp_colmajor<T>(c, rr, r);
    if (rr <= n) {
        // B (rr x n, wide): its tall orientation B^T is column-major n x rr == B row-major
        Mat<T> b = tmp_rowmajor<T>(c, rr, n);
        a.project(c, range, b);
        svd_core(c, b.t(), true, ub, s, vt);
    } else {
        Mat<T> b = tmp_colmajor<T>(c, rr, n);
        a.project(c, range, b);
        svd_core(c, b, false, ub, s, vt);
    }
    gemm<T>(c, 1, range, ub, 0, u);
}

// Fork / join of a side branch onto the context's second stream (created on first use, outside graph capture).
// While the side branch is issued, `stream` and the arena of the context are the side ones, so every helper
// below works unchanged; back() returns to the main stream, join() makes the main stream wait for the side one.
struct Fork {
    rc_context *c;
    hipStream_t main_stream = nullptr;
    bool active = false;
    explicit Fork(rc_context *ctx, bool want) : c(ctx) {
        if (!want || !c->opt_fork) return;
        if (!c->aux_stream) {
            if (c->capturing) return;  // cannot create a stream inside a capture: this graph stays single-stream
            RC_HIP(hipStreamCreateWithFlags(&c->aux_stream, hipStreamNonBlocking));
            RC_HIP(hipEventCreateWithFlags(&c->fork_ev, hipEventDisableTiming));
            RC_HIP(hipEventCreateWithFlags(&c->join_ev, hipEventDisableTiming));
        }
        main_stream = c->stream;
        RC_HIP(hipEventRecord(c->fork_ev, main_stream));
        RC_HIP(hipStreamWaitEvent(c->aux_stream, c->fork_ev, 0));
        c->stream = c->aux_stream;
        c->swap_arena();
        active = true;
    }
    void back() {
        if (!active) return;
        RC_HIP(hipEventRecord(c->join_ev, c->aux_stream));
        c->stream = main_stream;
        c->swap_arena();
    }
    void join() {
        if (!active) return;
        RC_HIP(hipStreamWaitEvent(main_stream, c->join_ev, 0));
        active = false;
    }
    ~Fork() {  // error path: leave the context on its main stream / arena
        if (active && c->stream == c->aux_stream) { c->stream = main_stream; c->swap_arena(); }
    }
};

template <typename T>
void rsvd_id_consumers(rc_context *c, Mat<T> range, Mat<T> b, const rc_rsvd_id_out &o);

// cfg3 "rSVD + ID" without host synchronisation
template <typename T>
void rsvd_id(rc_context *c, const OpView<T> &a, int64_t k, int64_t p, Mat<T> omega, uint64_t seed, const rc_rsvd_id_out &o) {
    const int64_t m = a.rows, n = a.cols;
    RC_REQUIRE(k >= 1 && k + p <= m && k <= n, RC_INVALID_ARGUMENT, "rsvd_id: need 1 <= k, k + p <= m, k <= n");
    ArenaMark mark(c);
    Mat<T> range = from_c<T>(o.range_q);
    if (range.p == nullptr) range = tmp_colmajor<T>(c, m, k);
    RC_REQUIRE(range.rows == m && range.cols == k, RC_INVALID_ARGUMENT, "rsvd_id: range_q must be m x k");
    {
        ProfScope ps(c, "stage:sample_range_by_rank");
        sample_range_by_rank(c, a, k, p, omega, seed, range);
    }
    // B = Q^H A once, shared by the SVD and the QR consumers
    Mat<T> b = tmp_rowmajor<T>(c, k, n);
    {
        ProfScope ps(c, "stage:project B=Q^H A");
        a.project(c, range, b);
    }
    rsvd_id_consumers(c, range, b, o);
}

// ---- the two consumers with the pivoted QR of B and the Jacobi SVD of the core in ONE launch (RC_OPT_FUSED_CONSUMERS) ----
// With a few compressions in flight the process's kernel slots are the bound: the Jacobi of the core
// holds a slot with two workgroups, the cooperative QRCP of B with 32.  Both only depend on B, so they share a launch.  With
// eight or more side by side the chip is the bound and the staged QRCP (fewer CU-steps) is the right shape: not taken there.
template <typename T>
bool fused_consumers_qualify(rc_context *c, int64_t k, int64_t n) {
    return c->opt_fused_consumers && c->opt_wide_coop && c->opt_tsqr && tsqr_fold() && c->lanes_in_flight() < 8 && tsqr_supported<T>(n, k) &&
           wide_coop_jacobi_supported<T>(k, n, c->device);
}

// Order: tall QR of B^T (B^T = Q_w R, B = L Q_w^T; L = R^T is the core), then the fused launch (B -> pivoted QR, L -> its SVD), then the tails of the
// two branches as rsvd_id_consumers / qrcp_core / svd_core have them: every kernel sees the operands it sees there, so all outputs
// are the same bits.  Returns false, with B untouched, when the tall QR does not certify (eager calls only): the caller's
// old order then runs.
template <typename T>
bool rsvd_id_consumers_fused(rc_context *c, Mat<T> range, Mat<T> b, const rc_rsvd_id_out &o) {
    const int64_t m = range.rows, k = b.rows, n = b.cols;
    ArenaMark mark(c);
    Mat<T> core = tmp_colmajor<T>(c, k, k);
    Mat<T> q1 = rowmajor(c->alloc<T>((size_t)n * even_ld(k)), n, k, even_ld(k));
    Mat<T> r2i = rowmajor(c->alloc<T>((size_t)k * even_ld(k)), k, k, even_ld(k));
    {
        ProfScope ps(c, "stage:tall QR of B^T");
        // tsqr_cholqr2_factored only READS its input (two Gram products and one application into q1): B stays where it lies for
        // the cooperative QRCP below, and for the old order when this does not certify
        if (!run_certified(c, [&](int *flag) { tsqr_cholqr2_factored<T>(c, b.t(), q1, r2i, core.t(), flag); })) return false;
    }
    // (ub: the Jacobi writes the left vectors of the core where U = range ub reads them -- no copy in svd_finish)
    Mat<T> ub = tmp_colmajor<T>(c, k, k), vc = tmp_colmajor<T>(c, k, k);
    Mat<T> qb = tmp_colmajor<T>(c, k, k);
    Mat<T> small = tmp_colmajor<T>(c, k, k);  // r2i vc for svd_finish
    Mat<T> r = o.qr_r.data ? from_c<T>(o.qr_r) : tmp_rowmajor<T>(c, k, n);
    int64_t *ind = o.qr_ind ? o.qr_ind : c->alloc<int64_t>((size_t)n);
    T *tau = c->alloc<T>((size_t)k);
    Mat<T> wf = tmp_colmajor<T>(c, k, n);
    T *s = static_cast<T *>(o.s);
    bool qr_done, small_done = false;
    {
        ProfScope ps(c, "stage:qrcp of B | svd of the core");
        qr_done = run_certified(c, [&](int *flag) { geqp3_wide_coop_jacobi<T>(c, b, wf, k, ind, tau, flag, core, ub, s, vc); });
    }
    {
        ProfScope ps(c, "stage:qrcp of B + column_id");
        const bool want_cz = o.id_c.data || o.id_z.data;
        Mat<T> cm = from_c<T>(o.id_c), z = from_c<T>(o.id_z);
        // R, Q_b and Z read only wf, ind and tau: one launch (k_rsvd_id_tails) in place of extract_r, form_q and id_z_from_r
        const bool tails = qr_done && k < n && id_fused();
        if (tails) {
            if (want_cz)
                RC_REQUIRE(cm.rows == m && cm.cols == k && z.rows == k && z.cols == n, RC_INVALID_ARGUMENT, "column_id: c %lld x %lld, z %lld x %lld",
                           (long long)cm.rows, (long long)cm.cols, (long long)z.rows, (long long)z.cols);
            // (and r2i vc of the SVD branch: both operands are complete, and the launch is as long as its Z role either way)
            rsvd_id_tails(c, wf, ind, tau, qb, r, want_cz ? z : Mat<T>(), r2i, vc, small);
            small_done = true;
        } else if (qr_done) {
            extract_r(c, wf, ind, r);
            form_q(c, wf, ind, tau, k, qb);
        } else {
            // the cooperative workgroups did not all become resident in time (eager calls only).  The SVD of the core stands (it does
            // not depend on them) and nothing below needs B any more: the pivoted QR takes its other paths on B itself
            qrcp_core(c, b, k, true, qb, r, ind);
        }
        Mat<T> q = o.qr_q.data ? from_c<T>(o.qr_q) : tmp_colmajor<T>(c, m, k);
        gemm_chain<T>(c, 1, range, qb, 0, q);
        if (want_cz && tails) gemm_chain<T>(c, 1, q, r.sub(0, k, 0, k), 0, cm);  // C = Q R11, as qr_column_id has it
        else if (want_cz) qr_column_id(c, q, r, ind, cm, z, /*own_ind=*/true);
    }
    {
        ProfScope ps(c, "stage:svd of B + U=Q Ub");
        svd_finish(c, /*transposed=*/true, /*factored=*/true, Mat<T>(), q1, r2i, ub, vc, s, ub, from_c<T>(o.vt), /*u_in_place=*/true, small_done ? small : Mat<T>());
        gemm_chain<T>(c, 1, range, ub, 0, from_c<T>(o.u));
    }
    return true;
}

// the two consumers of B = range^H A (k x n, destroyed): SVD::compute_from_range_estimate (src/svd.rs:171-183) and
// QR::compute_from_range_estimate + column_id (src/qr.rs:311-323, :270-309); outputs have range.rows rows
template <typename T>
void rsvd_id_consumers(rc_context *c, Mat<T> range, Mat<T> b, const rc_rsvd_id_out &o) {
    const int64_t m = range.rows, k = b.rows, n = b.cols;
    const bool want_id = o.id_c.data || o.id_z.data || o.qr_q.data || o.qr_r.data || o.qr_ind;
    const bool want_svd = o.u.data || o.s || o.vt.data;
    if (want_svd) RC_REQUIRE(o.u.data && o.s && o.vt.data, RC_INVALID_ARGUMENT, "rsvd_id: u, s, vt must be given together");
    // the two consumers of B are independent: the ID branch goes to the side stream, the SVD branch stays here.  Side by side
    // (RC_OPT_FORK_BRANCHES) the ID branch works on its own copy of B, taken before the fork (the SVD branch may overwrite B);
    // one after the other the pivoted QR reads B where it lies
    if (want_id && want_svd && !c->opt_fork && fused_consumers_qualify<T>(c, k, n)) {
        RC_REQUIRE(!(o.id_c.data || o.id_z.data) || (o.id_c.data && o.id_z.data), RC_INVALID_ARGUMENT, "rsvd_id: id_c and id_z must be given together");
        if (rsvd_id_consumers_fused(c, range, b, o)) return;
    }
    Mat<T> wq;
    if (want_id && want_svd && c->opt_fork) {
        wq = tmp_colmajor<T>(c, k, n);
        copy_mat(c, b, wq);
    }
    Fork fork(c, want_svd && want_id);
    if (want_id) {
        ProfScope ps(c, "stage:qrcp of B + column_id");
        Mat<T> qb = tmp_colmajor<T>(c, k, k);
        Mat<T> r = o.qr_r.data ? from_c<T>(o.qr_r) : tmp_rowmajor<T>(c, k, n);
        int64_t *ind = o.qr_ind ? o.qr_ind : c->alloc<int64_t>((size_t)n);
        if (wq.p) qrcp_core(c, wq, k, true, qb, r, ind);
        else qrcp_core(c, b, k, true, qb, r, ind, /*keep_w=*/want_svd);   // the SVD consumer below still needs B
        Mat<T> q = o.qr_q.data ? from_c<T>(o.qr_q) : tmp_colmajor<T>(c, m, k);
        gemm<T>(c, 1, range, qb, 0, q);
        if (o.id_c.data || o.id_z.data) {
            RC_REQUIRE(o.id_c.data && o.id_z.data, RC_INVALID_ARGUMENT, "rsvd_id: id_c and id_z must be given together");
            qr_column_id(c, q, r, ind, from_c<T>(o.id_c), from_c<T>(o.id_z), /*own_ind=*/true);
        }
    }
    fork.back();
    if (want_svd) {
        ProfScope ps(c, "stage:svd of B + U=Q Ub");
        Mat<T> ub = tmp_colmajor<T>(c, k, k);
        svd_core(c, b.t(), true, ub, static_cast<T *>(o.s), from_c<T>(o.vt));  // destroys b
        gemm<T>(c, 1, range, ub, 0, from_c<T>(o.u));
    }
    fork.join();
}

// One matrix sharded by ROWS over the ranks of `comm` (comm == nullptr: one rank).  This rank holds
// a (m_r x n, m_r >= k + p).  The sketch, the factorizations of the tall blocks and every product with A stay local; what
// crosses the links is the l x l factor of every rank (all-gather) and the k x n projection (all-reduce):
//   Omega            the same Philox stream on every rank, nothing is sent      (src/random_sampling.rs:103-118)
//   Y_r = A_r Omega, Y_r P_r = Q_r R_r, S_r = R_r P_r^T (l x l)                   local
//   S = [S_0; ...; S_{W-1}] all-gathered; S P = Q_S R redundantly on every rank  => Y P = blockdiag(Q_r) Q_S R is THE pivoted
//                    QR of Y: S has the column norms and inner products of Y, so pivots and R are ?geqp3's of the whole Y
//   range_r = Q_r Q_S[block r, :k];  B = sum_r range_r^H A_r (one all-reduce);  SVD / pivoted QR / ID of B redundantly,
//   U_r = range_r U_b, Q_r' = range_r Q_b, C_r = Q_r' R11                         local (src/svd.rs:171-183, src/qr.rs:311-323)
// Row-sharded outputs: range_q, u, qr_q, id_c (m_r rows); replicated, bit-identical on every rank: s, vt, qr_r, qr_ind, id_z.
template <typename T>
void rsvd_id_row_sharded(rc_comm *comm, rc_context *c, Mat<T> a, int64_t k, int64_t p, uint64_t seed, const rc_rsvd_id_out &o) {
    int32_t world = 1, rank = 0;
    if (comm) RC_REQUIRE(rc_comm_world(comm, &world, &rank) == RC_OK, RC_INVALID_ARGUMENT, "rsvd_id_row_sharded: bad communicator");
    const int64_t mr = a.rows, n = a.cols, l = k + p;
    RC_REQUIRE(k >= 1 && p >= 0 && k <= n, RC_INVALID_ARGUMENT, "rsvd_id_row_sharded: need 1 <= k <= n, p >= 0");
    RC_REQUIRE(l <= mr, RC_INVALID_ARGUMENT, "rsvd_id_row_sharded: every rank needs at least k + p = %lld rows, this one has %lld", (long long)l, (long long)mr);
    RC_REQUIRE(!c->capturing, RC_INVALID_ARGUMENT, "rsvd_id_row_sharded: not capturable (the collectives may be staged through the host)");
    auto comm_ok = [&](rc_status st, const char *what) {
        if (st != RC_OK) fail(st, "rsvd_id_row_sharded: %s failed: %s", what, rc_comm_last_error_message(comm));
    };
    ArenaMark mark(c);
    Mat<T> range = from_c<T>(o.range_q);
    if (range.p == nullptr) range = tmp_colmajor<T>(c, mr, k);
    RC_REQUIRE(range.rows == mr && range.cols == k, RC_INVALID_ARGUMENT, "rsvd_id_row_sharded: range_q must be m_r x k");
    {
        ProfScope ps(c, "stage:sharded range (local sketch + QR, all-gather of the l x l factors)");
        ArenaMark inner(c);
        Mat<T> omega = tmp_rowmajor<T>(c, n, l);
        fill_gaussian(c, omega, seed, 0);
        Mat<T> y = tmp_colmajor<T>(c, mr, l);
        gemm<T>(c, 1, a, omega, 0, y);
        Mat<T> qr = tmp_colmajor<T>(c, mr, l), rr = tmp_rowmajor<T>(c, l, l);
        int64_t *ind = c->alloc<int64_t>((size_t)l), *inv = c->alloc<int64_t>((size_t)l);
        qrcp_core(c, y, l, true, qr, rr, ind);
        invert_perm(c, ind, l, inv);
        const size_t blk = (size_t)l * (size_t)rr.rs;  // one rank's factor incl. the row padding of the temporaries
        Mat<T> sall = rowmajor(c->alloc<T>(blk * (size_t)world), (int64_t)world * l, l, rr.rs);
        Mat<T> sr = sall.sub((int64_t)rank * l, l, 0, l);
        fill_words(c, sr.p, blk * sizeof(T), 0u);
        gather_cols(c, rr, inv, sr);  // S_r = R_r P_r^T
        if (comm) comm_ok(rc_comm_all_gather(comm, c, sr.p, sall.p, blk * sizeof(T)), "all-gather");
        Mat<T> ws = tmp_colmajor<T>(c, sall.rows, l), qs = tmp_colmajor<T>(c, sall.rows, k);
        copy_mat(c, sall, ws);
        int64_t *ind2 = c->alloc<int64_t>((size_t)l);
        qrcp_core(c, ws, k, true, qs, Mat<T>(), ind2);  // only the first k steps influence Q_S[:, :k]
        gemm<T>(c, 1, qr, qs.sub((int64_t)rank * l, l, 0, k), 0, range);
    }
    Mat<T> b = tmp_rowmajor<T>(c, k, n);
    {
        ProfScope ps(c, "stage:sharded project B = sum_r range_r^H A_r (all-reduce)");
        if (b.rs != n) fill_words(c, b.p, (size_t)k * (size_t)b.rs * sizeof(T), 0u);
        product(c, 1, true, range, a, 0, b);  // B = range^H A
        if (comm) comm_ok(rc_comm_all_reduce_sum(comm, c, b.p, (size_t)k * (size_t)b.rs, (int32_t)sizeof(T)), "all-reduce");
    }
    rsvd_id_consumers(c, range, b, o);
}

template <typename T>
void svd_rank_by_tolerance(rc_context *c, const T *s, int64_t len, double tol, int64_t *rank) {
    RC_REQUIRE(tol < 1.0 && 0.0 <= tol, RC_INVALID_ARGUMENT, "Require 0 <= tol < 1.0");
    RC_REQUIRE(len >= 1, RC_COMPRESSION_ERROR, "svd_rank_by_tolerance: empty spectrum");
    std::vector<T> h((size_t)len);
    read_back(c, s, h.data(), (size_t)len);
    for (int64_t i = 0; i < len; ++i) {
        if ((double)(h[i] / h[0]) < tol) { *rank = i; return; }  // svd.rs:95
    }
    fail(RC_COMPRESSION_ERROR, "Could not compress to desired tolerance");
}

}  // namespace

namespace rc {

// Whether the rank-k column ID of an m x n matrix on this context takes the truncated blocked factorization, whose output the ID is
// read from directly (column_id_from_qrcp).  One predicate for the lone call below and for rc_batch_column_id_* (rc_batch.hip), which
// promises the lone call's bits: every other shape -- tall-skinny, short-wide, k == n, too small for the panels -- goes through
// qrcp_core and qr_column_id in both.
template <typename T>
bool column_id_blocked_route(rc_context *c, int64_t m, int64_t n, int64_t k) {
    static const int long_way = env_int("RC_COLUMN_ID_FORM_Q", 0);
    return !long_way && k < n && c->opt_blocked && !c->capturing && geqp3_blocked_supported<T>(m, n, k) &&
           !(c->opt_tsqr && tsqr_supported<T>(m, n)) && !(c->opt_wide_coop && wide_coop_supported<T>(m, n, c->device)) && !(c->opt_wide_lazy && wide_lazy_supported<T>(m, n));
}

// cfg5 unit: rank-k column ID of a dense matrix through the truncated factorization
template <typename T>
void column_id_rank(rc_context *c, Mat<T> a, int64_t k, Mat<T> cm, Mat<T> z, int64_t *col_ind) {
    const int64_t m = a.rows, n = a.cols;
    k = std::min(k, std::min(m, n));
    ArenaMark mark(c);
    Mat<T> w = tmp_colmajor<T>(c, m, n);
    copy_mat(c, a, w);
    // Fast path: the truncated blocked factorization leaves w in the ?geqp3 format; Z and C come straight from it (column_id_from_qrcp,
    // kernels_qr.hip: C = Q R11 is the selected columns of A themselves -- no Q is formed).  The other factorization paths
    // (tall-skinny, short-wide, under capture) return Q and R and go through qr_column_id.
    if (column_id_blocked_route<T>(c, m, n, k)) {
        T *tau = c->alloc<T>((size_t)std::max<int64_t>(k, 1));
        geqp3_blocked<T>(c, w, k, col_ind, tau, Mat<T>(), /*restore_from=*/a);
        column_id_from_qrcp(c, a, w, k, col_ind, cm, z);
        return;
    }
    Mat<T> q = tmp_colmajor<T>(c, m, k);
    Mat<T> r = tmp_rowmajor<T>(c, k, n);
    qrcp_core(c, w, k, true, q, r, col_ind);
    qr_column_id(c, q, r, col_ind, cm, z, /*own_ind=*/true);
}

template bool column_id_blocked_route<double>(rc_context *, int64_t, int64_t, int64_t);
template bool column_id_blocked_route<float>(rc_context *, int64_t, int64_t, int64_t);
template void column_id_rank<double>(rc_context *, Mat<double>, int64_t, Mat<double>, Mat<double>, int64_t *);
template void column_id_rank<float>(rc_context *, Mat<float>, int64_t, Mat<float>, Mat<float>, int64_t *);

}  // namespace rc

// ===========================================================================
// extern "C"
// ===========================================================================
extern "C" {

int32_t rc_abi_version(void) { return RC_ABI_VERSION; }

rc_status rc_create(rc_context **ctx, int32_t device, void *hip_stream) {
    if (!ctx) return RC_INVALID_ARGUMENT;
    *ctx = nullptr;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || device < 0 || device >= count) return RC_RUNTIME_ERROR;
    rc_context *c = new rc_context();
    c->device = device;
    c->stream = static_cast<hipStream_t>(hip_stream);
    {
        DeviceGuard dg(device);
        try { (void)c->health_word(); (void)c->epoch_word(); coop_prepare(device); } catch (const Error &) { delete c; return RC_RUNTIME_ERROR; }
    }
    *ctx = c;
    return RC_OK;
}

rc_status rc_stream_create(int32_t device, void **hip_stream) {
    if (!hip_stream) return RC_INVALID_ARGUMENT;
    *hip_stream = nullptr;
    DeviceGuard dg(device);
    hipStream_t st = nullptr;
    if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) return RC_RUNTIME_ERROR;
    *hip_stream = st;
    return RC_OK;
}
rc_status rc_stream_destroy(int32_t device, void *hip_stream) {
    if (!hip_stream) return RC_OK;
    DeviceGuard dg(device);
    return hipStreamDestroy(static_cast<hipStream_t>(hip_stream)) == hipSuccess ? RC_OK : RC_RUNTIME_ERROR;
}

rc_status rc_destroy(rc_context *ctx) {
    if (!ctx) return RC_OK;
    {
        DeviceGuard dg(ctx->device);
        ctx->release_all();
    }
    delete ctx;
    return RC_OK;
}

rc_status rc_set_stream(rc_context *ctx, void *hip_stream) {
    if (!ctx) return RC_INVALID_ARGUMENT;
    DeviceGuard dg(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);  // the arena may still be in use on the old stream
    ctx->stream = static_cast<hipStream_t>(hip_stream);
    return RC_OK;
}

rc_status rc_get_stream(rc_context *ctx, void **hip_stream) {
    if (!ctx || !hip_stream) return RC_INVALID_ARGUMENT;
    *hip_stream = ctx->stream;
    return RC_OK;
}

rc_status rc_synchronize(rc_context *ctx) {
    if (!ctx) return RC_INVALID_ARGUMENT;
    DeviceGuard dg(ctx->device);
    hipError_t e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) { ctx->last_error = hipGetErrorString(e); return RC_RUNTIME_ERROR; }
    return RC_OK;
}

// Record a completion event behind the last command of EVERY context first, wait for them afterwards.  With dozens of
// busy streams a stream-by-stream hipStreamSynchronize returned after max(259 ms, work) on this stack (DESIGN.md,
// "Completion waits"); with an event on every stream before the first wait the waits come back on time.
rc_status rc_synchronize_all(rc_context *const *ctxs, int32_t n) {
    if (n < 0 || (n > 0 && !ctxs)) return RC_INVALID_ARGUMENT;
    rc_status st = RC_OK;
    for (int32_t i = 0; i < n; ++i) {
        rc_context *c = ctxs[i];
        if (!c) return RC_INVALID_ARGUMENT;
        DeviceGuard dg(c->device);
        if (!c->sync_ev && hipEventCreateWithFlags(&c->sync_ev, hipEventDisableTiming) != hipSuccess) { c->last_error = "hipEventCreate failed"; return RC_RUNTIME_ERROR; }
        hipError_t e = hipEventRecord(c->sync_ev, c->stream);
        if (e != hipSuccess) { c->last_error = hipGetErrorString(e); st = RC_RUNTIME_ERROR; }
    }
    for (int32_t i = 0; i < n; ++i) {
        rc_context *c = ctxs[i];
        DeviceGuard dg(c->device);
        hipError_t e = hipEventSynchronize(c->sync_ev);
        if (e == hipSuccess && c->aux_stream) e = hipStreamSynchronize(c->aux_stream);
        if (e != hipSuccess) { c->last_error = hipGetErrorString(e); st = RC_RUNTIME_ERROR; }
    }
    return st;
}

rc_status rc_reserve_workspace(rc_context *ctx, size_t bytes) {
    if (!ctx) return RC_INVALID_ARGUMENT;
    DeviceGuard dg(ctx->device);
    try { ctx->reserve(bytes); } catch (const Error &e) { ctx->last_error = e.msg; return e.code; }
    return RC_OK;
}

const char *rc_last_error_message(const rc_context *ctx) { return ctx ? ctx->last_error.c_str() : "null context"; }

rc_status rc_device_malloc(rc_context *ctx, size_t bytes, void **ptr) {
    if (!ctx || !ptr) return RC_INVALID_ARGUMENT;
    DeviceGuard dg(ctx->device);
    hipError_t e = hipMalloc(ptr, bytes ? bytes : 1);
    if (e != hipSuccess) { ctx->last_error = hipGetErrorString(e); return RC_RUNTIME_ERROR; }
    return RC_OK;
}
rc_status rc_device_free(rc_context *ctx, void *ptr) {
    if (!ctx) return RC_INVALID_ARGUMENT;
    DeviceGuard dg(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    hipError_t e = hipFree(ptr);
    if (e != hipSuccess) { ctx->last_error = hipGetErrorString(e); return RC_RUNTIME_ERROR; }
    return RC_OK;
}
rc_status rc_memcpy_h2d(rc_context *ctx, void *dst_dev, const void *src_host, size_t bytes) {
    if (!ctx) return RC_INVALID_ARGUMENT;
    DeviceGuard dg(ctx->device);
    hipError_t e = hipMemcpyAsync(dst_dev, src_host, bytes, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);  // pageable host memory: keep it simple and safe
    if (e != hipSuccess) { ctx->last_error = hipGetErrorString(e); return RC_RUNTIME_ERROR; }
    return RC_OK;
}
rc_status rc_memcpy_d2h(rc_context *ctx, void *dst_host, const void *src_dev, size_t bytes) {
    if (!ctx) return RC_INVALID_ARGUMENT;
    DeviceGuard dg(ctx->device);
    hipError_t e = hipMemcpyAsync(dst_host, src_dev, bytes, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) { ctx->last_error = hipGetErrorString(e); return RC_RUNTIME_ERROR; }
    return RC_OK;
}

// ---- hipGraph capture of the work issued on the context's stream -------------
rc_status rc_graph_begin_capture(rc_context *ctx) {
    if (!ctx) return RC_INVALID_ARGUMENT;
    DeviceGuard dg(ctx->device);
    if (ctx->capturing) { ctx->last_error = "capture already in progress"; return RC_INVALID_ARGUMENT; }
    if (!ctx->overflow.empty() || !ctx->aux_arena.overflow.empty()) ctx->reset_arena();  // settle the arenas before anything is baked into a graph
    hipError_t e = hipStreamBeginCapture(ctx->stream, hipStreamCaptureModeThreadLocal);
    if (e != hipSuccess) { ctx->last_error = hipGetErrorString(e); return RC_RUNTIME_ERROR; }
    ctx->capturing = true;
    return RC_OK;
}
rc_status rc_graph_end_capture(rc_context *ctx, void **graph_exec) {
    if (!ctx || !graph_exec) return RC_INVALID_ARGUMENT;
    DeviceGuard dg(ctx->device);
    *graph_exec = nullptr;
    hipGraph_t graph = nullptr;
    hipError_t e = hipStreamEndCapture(ctx->stream, &graph);
    ctx->capturing = false;
    if (e != hipSuccess || !graph) { ctx->last_error = std::string("hipStreamEndCapture: ") + hipGetErrorString(e); return RC_RUNTIME_ERROR; }
    hipGraphExec_t exec = nullptr;
    e = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
    (void)hipGraphDestroy(graph);
    if (e != hipSuccess) { ctx->last_error = std::string("hipGraphInstantiate: ") + hipGetErrorString(e); return RC_RUNTIME_ERROR; }
    *graph_exec = exec;
    ctx->live_graphs += 1;
    return RC_OK;
}
rc_status rc_graph_launch(rc_context *ctx, void *graph_exec) {
    if (!ctx || !graph_exec) return RC_INVALID_ARGUMENT;
    DeviceGuard dg(ctx->device);
    hipError_t e = hipGraphLaunch(static_cast<hipGraphExec_t>(graph_exec), ctx->stream);
    if (e != hipSuccess) { ctx->last_error = hipGetErrorString(e); return RC_RUNTIME_ERROR; }
    return RC_OK;
}
rc_status rc_graph_destroy(rc_context *ctx, void *graph_exec) {
    if (!ctx) return RC_INVALID_ARGUMENT;
    if (!graph_exec) return RC_OK;
    DeviceGuard dg(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    (void)hipGraphExecDestroy(static_cast<hipGraphExec_t>(graph_exec));
    if (ctx->live_graphs > 0 && --ctx->live_graphs == 0) {
        for (void *p : ctx->retired) (void)hipFree(p);
        ctx->retired.clear();
    }
    return RC_OK;
}

// ---- options / health -----------------------------------------------------------
rc_status rc_set_option(rc_context *ctx, int32_t option, int64_t value) {
    if (!ctx) return RC_INVALID_ARGUMENT;
    switch (option) {
        case RC_OPT_TALL_SKINNY_FAST_PATH: ctx->opt_tsqr = value != 0; return RC_OK;
        case RC_OPT_WIDE_LAZY_QRCP: ctx->opt_wide_lazy = value != 0; return RC_OK;
        case RC_OPT_WIDE_COOP_QRCP: ctx->opt_wide_coop = value != 0; return RC_OK;
        case RC_OPT_POWER_ITERATION_FIXED: ctx->opt_power_fixed = value != 0; return RC_OK;
        case RC_OPT_FORK_BRANCHES: ctx->opt_fork = value != 0; return RC_OK;
        case RC_OPT_BLOCKED_QRCP: ctx->opt_blocked = value != 0; return RC_OK;
        case RC_OPT_COOP_PANEL: ctx->opt_coop_panel = value != 0; return RC_OK;
        case RC_OPT_CONCURRENCY_HINT: ctx->opt_lanes = (int)std::max<int64_t>(1, std::min<int64_t>(value, 1024)); return RC_OK;
        case RC_OPT_KERNEL_SLOTS: ctx->opt_slots = (int)std::max<int64_t>(1, std::min<int64_t>(value, 1024)); return RC_OK;
        case RC_OPT_FUSED_CONSUMERS: ctx->opt_fused_consumers = value != 0; return RC_OK;
        default: ctx->last_error = "unknown option"; return RC_INVALID_ARGUMENT;
    }
}
rc_status rc_get_health(rc_context *ctx, int32_t *word) {
    if (!ctx || !word) return RC_INVALID_ARGUMENT;
    DeviceGuard dg(ctx->device);
    *word = 0;
    if (!ctx->health) return RC_OK;
    // read and clear on the context's own stream (pinned read-back, then a one-thread kernel): no null-stream traffic
    int h = 0;
    if (debug_memset_path() & 2) {  // diagnostic: the round-2 path
        hipError_t e = hipStreamSynchronize(ctx->stream);
        if (e == hipSuccess) e = hipMemcpy(&h, ctx->health, sizeof(int), hipMemcpyDeviceToHost);
        if (e == hipSuccess) e = hipMemset(ctx->health, 0, sizeof(int));
        if (e != hipSuccess) { ctx->last_error = hipGetErrorString(e); return RC_RUNTIME_ERROR; }
        *word = h;
        return RC_OK;
    }
    try {
        read_back(ctx, ctx->health, &h, 1);
        hipLaunchKernelGGL(k_set_word, dim3(1), dim3(64), 0, ctx->stream, ctx->health, 0);
        RC_HIP(hipStreamSynchronize(ctx->stream));
    } catch (const Error &e) { ctx->last_error = e.msg; return e.code; }
    *word = h;
    return RC_OK;
}

// ---- stage / kernel timers ----------------------------------------------------
rc_status rc_profile_enable(rc_context *ctx, int32_t on) {
    if (!ctx) return RC_INVALID_ARGUMENT;
    ctx->prof_on = on != 0;
    return RC_OK;
}
rc_status rc_profile_reset(rc_context *ctx) {
    if (!ctx) return RC_INVALID_ARGUMENT;
    DeviceGuard dg(ctx->device);
    ctx->prof_resolve();
    ctx->prof_acc.clear();
    return RC_OK;
}
rc_status rc_profile_count(rc_context *ctx, int32_t *n) {
    if (!ctx || !n) return RC_INVALID_ARGUMENT;
    DeviceGuard dg(ctx->device);
    ctx->prof_resolve();
    *n = (int32_t)ctx->prof_acc.size();
    return RC_OK;
}
rc_status rc_profile_get(rc_context *ctx, int32_t i, char *name, int32_t name_cap, double *total_ms, int64_t *calls) {
    if (!ctx || i < 0 || i >= (int32_t)ctx->prof_acc.size()) return RC_INVALID_ARGUMENT;
    auto it = ctx->prof_acc.begin();
    std::advance(it, i);
    if (name && name_cap > 0) {
        std::strncpy(name, it->first.c_str(), (size_t)name_cap - 1);
        name[name_cap - 1] = 0;
    }
    if (total_ms) *total_ms = it->second.ms;
    if (calls) *calls = it->second.calls;
    return RC_OK;
}

const char *rc_last_gemm_kernel_name(const rc_context *ctx) { return ctx ? ctx->last_gemm_kernel.c_str() : ""; }

rc_status rc_random_bits_u32(rc_context *ctx, uint32_t *out, int64_t n, uint64_t seed, uint64_t word_offset) {
    return guarded(ctx, [&] {
        RC_REQUIRE(n >= 0 && (out != nullptr || n == 0), RC_INVALID_ARGUMENT, "random_bits: null output");
        philox_words(ctx, out, n, seed, word_offset);
    });
}

rc_status rc_invert_permutation(rc_context *ctx, const int64_t *perm, int64_t n, int64_t *inverse) {
    return guarded(ctx, [&] { invert_perm(ctx, perm, n, inverse); });
}

#define RC_DEFINE_TYPED(SUF, T)                                                                                                          \
    rc_status rc_random_gaussian_##SUF(rc_context *ctx, rc_matrix out, uint64_t seed, uint64_t offset) {                                 \
        return guarded(ctx, [&] { check_view(out, "out"); fill_gaussian<T>(ctx, from_c<T>(out), seed, offset); });                      \
    }                                                                                                                                    \
    rc_status rc_matmat_##SUF(rc_context *ctx, rc_matrix a, rc_matrix x, rc_matrix y) {                                                  \
        return guarded(ctx, [&] { gemm<T>(ctx, 1, from_c<T>(a), from_c<T>(x), 0, from_c<T>(y)); });                                     \
    }                                                                                                                                    \
    rc_status rc_conj_matmat_##SUF(rc_context *ctx, rc_matrix a, rc_matrix x, rc_matrix y) {                                             \
        return guarded(ctx, [&] { gemm<T>(ctx, 1, from_c<T>(a).t(), from_c<T>(x), 0, from_c<T>(y)); });                                 \
    }                                                                                                                                    \
    rc_status rc_gemm_##SUF(rc_context *ctx, int32_t ta, int32_t tb, T alpha, rc_matrix a, rc_matrix b, T beta, rc_matrix c) {           \
        return guarded(ctx, [&] {                                                                                                        \
            Mat<T> A = from_c<T>(a), B = from_c<T>(b);                                                                                   \
            gemm<T>(ctx, alpha, ta ? A.t() : A, tb ? B.t() : B, beta, from_c<T>(c));                                                     \
        });                                                                                                                              \
    }                                                                                                                                    \
    rc_status rc_rel_diff_fro_##SUF(rc_context *ctx, rc_matrix first, rc_matrix second, T *out) {                                        \
        return guarded(ctx, [&] {                                                                                                        \
            T *d = ctx->alloc<T>(2);                                                                                                     \
            fro_diff<T>(ctx, from_c<T>(first), from_c<T>(second), d);                                                                    \
            T h[2];                                                                                                                      \
            read_back(ctx, d, h, 2);                                                                                                     \
            *out = std::sqrt(h[0]) / std::sqrt(h[1]);                                                                                    \
        });                                                                                                                              \
    }                                                                                                                                    \
    rc_status rc_pivoted_qr_##SUF(rc_context *ctx, rc_matrix a, rc_matrix q, rc_matrix r, int64_t *ind) {                                \
        return guarded(ctx, [&] { pivoted_qr<T>(ctx, from_c<T>(a), from_c<T>(q), from_c<T>(r), ind); });                                 \
    }                                                                                                                                    \
    rc_status rc_pivoted_lq_##SUF(rc_context *ctx, rc_matrix a, rc_matrix l, rc_matrix q, int64_t *ind) {                                \
        return guarded(ctx, [&] { pivoted_qr<T>(ctx, from_c<T>(a).t(), from_c<T>(q).t(), from_c<T>(l).t(), ind); });                     \
    }                                                                                                                                    \
    rc_status rc_geqp3_##SUF(rc_context *ctx, rc_matrix a, int64_t kmax, int64_t *jpvt, T *tau) {                                        \
        return guarded(ctx, [&] { lapack_geqp3<T>(ctx, from_c<T>(a), kmax, jpvt, tau); });                                               \
    }                                                                                                                                    \
    rc_status rc_orgqr_##SUF(rc_context *ctx, rc_matrix a, const T *tau, int64_t k, rc_matrix q) {                                       \
        return guarded(ctx, [&] { lapack_orgqr<T>(ctx, from_c<T>(a), tau, k, from_c<T>(q)); });                                          \
    }                                                                                                                                    \
    rc_status rc_trsm_upper_##SUF(rc_context *ctx, rc_matrix t, rc_matrix b) {                                                           \
        return guarded(ctx, [&] {                                                                                                        \
            Mat<T> tt = from_c<T>(t), bb = from_c<T>(b);                                                                                 \
            RC_REQUIRE(tt.rows == tt.cols && tt.rows == bb.rows, RC_INVALID_ARGUMENT, "trsm_upper: t must be k x k, b k x nrhs");       \
            trsm_upper<T>(ctx, tt, bb);                                                                                                  \
        });                                                                                                                              \
    }                                                                                                                                    \
    rc_status rc_compute_svd_##SUF(rc_context *ctx, rc_matrix a, rc_matrix u, T *s, rc_matrix vt) {                                      \
        return guarded(ctx, [&] { compute_svd<T>(ctx, from_c<T>(a), from_c<T>(u), s, from_c<T>(vt)); });                                 \
    }                                                                                                                                    \
    rc_status rc_qr_to_mat_##SUF(rc_context *ctx, rc_matrix q, rc_matrix r, const int64_t *ind, rc_matrix out) {                         \
        return guarded(ctx, [&] {                                                                                                        \
            Mat<T> R = from_c<T>(r);                                                                                                     \
            int64_t *inv = ctx->alloc<int64_t>((size_t)std::max<int64_t>(R.cols, 1));                                                   \
            invert_perm(ctx, ind, R.cols, inv);                                                                                          \
            Mat<T> rp = tmp_rowmajor<T>(ctx, R.rows, R.cols);                                                                            \
            gather_cols<T>(ctx, R, inv, rp);                                                                                             \
            gemm<T>(ctx, 1, from_c<T>(q), rp, 0, from_c<T>(out));                                                                        \
        });                                                                                                                              \
    }                                                                                                                                    \
    rc_status rc_lq_to_mat_##SUF(rc_context *ctx, rc_matrix l, rc_matrix q, const int64_t *ind, rc_matrix out) {                         \
        return guarded(ctx, [&] {                                                                                                        \
            Mat<T> L = from_c<T>(l);                                                                                                     \
            int64_t *inv = ctx->alloc<int64_t>((size_t)std::max<int64_t>(L.rows, 1));                                                   \
            invert_perm(ctx, ind, L.rows, inv);                                                                                          \
            Mat<T> lp = tmp_rowmajor<T>(ctx, L.rows, L.cols);                                                                            \
            gather_cols<T>(ctx, L.t(), inv, lp.t());                                                                                     \
            gemm<T>(ctx, 1, lp, from_c<T>(q), 0, from_c<T>(out));                                                                        \
        });                                                                                                                              \
    }                                                                                                                                    \
    rc_status rc_qr_column_id_##SUF(rc_context *ctx, rc_matrix q, rc_matrix r, const int64_t *ind, rc_matrix c, rc_matrix z) {           \
        return guarded(ctx, [&] { qr_column_id<T>(ctx, from_c<T>(q), from_c<T>(r), ind, from_c<T>(c), from_c<T>(z), /*own_ind=*/false); }); \
    }                                                                                                                                    \
    rc_status rc_lq_row_id_##SUF(rc_context *ctx, rc_matrix l, rc_matrix q, const int64_t *ind, rc_matrix x, rc_matrix rr) {             \
        return guarded(ctx, [&] { lq_row_id<T>(ctx, from_c<T>(l), from_c<T>(q), ind, from_c<T>(x), from_c<T>(rr), /*own_ind=*/false); }); \
    }                                                                                                                                    \
    rc_status rc_svd_rank_by_tolerance_##SUF(rc_context *ctx, const T *s, int64_t len, double tol, int64_t *rank) {                      \
        return guarded(ctx, [&] { svd_rank_by_tolerance<T>(ctx, s, len, tol, rank); });                                                  \
    }                                                                                                                                    \
    rc_status rc_svd_to_mat_##SUF(rc_context *ctx, rc_matrix u, const T *s, rc_matrix vt, rc_matrix out) {                               \
        return guarded(ctx, [&] {                                                                                                        \
            Mat<T> VT = from_c<T>(vt);                                                                                                   \
            Mat<T> sv = tmp_rowmajor<T>(ctx, VT.rows, VT.cols);                                                                          \
            scale_rows<T>(ctx, s, VT, sv);                                                                                               \
            gemm<T>(ctx, 1, from_c<T>(u), sv, 0, from_c<T>(out));                                                                        \
        });                                                                                                                              \
    }                                                                                                                                    \
    rc_status rc_svd_to_qr_##SUF(rc_context *ctx, rc_matrix u, const T *s, rc_matrix vt, rc_matrix q, rc_matrix r, int64_t *ind) {       \
        return guarded(ctx, [&] {                                                                                                        \
            Mat<T> VT = from_c<T>(vt), Q = from_c<T>(q);                                                                                 \
            Mat<T> w = tmp_colmajor<T>(ctx, VT.rows, VT.cols);                                                                           \
            scale_rows<T>(ctx, s, VT, w);                                                                                                \
            const int64_t k = Q.cols;                                                                                                    \
            RC_REQUIRE(k <= std::min(VT.rows, VT.cols), RC_INVALID_ARGUMENT, "svd_to_qr: rank exceeds min(r, n)");                       \
            Mat<T> qb = tmp_colmajor<T>(ctx, VT.rows, k);                                                                                \
            qrcp_core<T>(ctx, w, k, true, qb, from_c<T>(r), ind);                                                                        \
            gemm<T>(ctx, 1, from_c<T>(u), qb, 0, Q);                                                                                     \
        });                                                                                                                              \
    }                                                                                                                                    \
    rc_status rc_column_id_two_sided_##SUF(rc_context *ctx, rc_matrix c, rc_matrix c_out, rc_matrix x, int64_t *row_ind) {               \
        return guarded(ctx, [&] {                                                                                                        \
            Mat<T> C = from_c<T>(c);                                                                                                     \
            const int64_t m = C.rows, k = C.cols, kk = std::min(m, k);                                                                   \
            Mat<T> l = tmp_rowmajor<T>(ctx, m, kk), ql = tmp_rowmajor<T>(ctx, kk, k);                                                    \
            pivoted_qr<T>(ctx, C.t(), ql.t(), l.t(), row_ind); /* LQ::compute_from, qr.rs:354-362 */                                     \
            lq_row_id<T>(ctx, l, ql, row_ind, from_c<T>(c_out), from_c<T>(x), /*own_ind=*/true);                                         \
        });                                                                                                                              \
    }                                                                                                                                    \
    rc_status rc_row_id_two_sided_##SUF(rc_context *ctx, rc_matrix r, rc_matrix x, rc_matrix r_out, int64_t *col_ind) {                  \
        return guarded(ctx, [&] {                                                                                                        \
            Mat<T> R = from_c<T>(r);                                                                                                     \
            const int64_t k = R.rows, n = R.cols, kk = std::min(k, n);                                                                   \
            Mat<T> q = tmp_colmajor<T>(ctx, k, kk), rr = tmp_rowmajor<T>(ctx, kk, n);                                                    \
            pivoted_qr<T>(ctx, R, q, rr, col_ind);                                                                                       \
            qr_column_id<T>(ctx, q, rr, col_ind, from_c<T>(x), from_c<T>(r_out), /*own_ind=*/true);                                      \
        });                                                                                                                              \
    }                                                                                                                                    \
    rc_status rc_rsvd_id_##SUF(rc_context *ctx, rc_matrix a, int64_t k, int64_t p, rc_matrix omega, uint64_t seed,                       \
                               const rc_rsvd_id_out *out) {                                                                              \
        return guarded(ctx, [&] {                                                                                                        \
            RC_REQUIRE(out != nullptr, RC_INVALID_ARGUMENT, "rsvd_id: null output descriptor");                                          \
            rsvd_id<T>(ctx, OpView<T>::of(from_c<T>(a)), k, p, from_c<T>(omega), seed, *out);                                            \
        });                                                                                                                              \
    }                                                                                                                                    \
    /* the same composition over the host's operator callbacks (rc_operator) */                                                          \
    rc_status rc_rsvd_id_op_##SUF(rc_context *ctx, const rc_operator *op, int64_t k, int64_t p, rc_matrix omega, uint64_t seed,          \
                                  const rc_rsvd_id_out *out) {                                                                           \
        return guarded(ctx, [&] {                                                                                                        \
            RC_REQUIRE(out != nullptr, RC_INVALID_ARGUMENT, "rsvd_id: null output descriptor");                                          \
            rsvd_id<T>(ctx, OpView<T>::of(op), k, p, from_c<T>(omega), seed, *out);                                                      \
        });                                                                                                                              \
    }                                                                                                                                    \
    rc_status rc_rsvd_id_row_sharded_##SUF(rc_comm *comm, rc_context *ctx, rc_matrix a_local, int64_t k, int64_t p, uint64_t seed,       \
                                           const rc_rsvd_id_out *out) {                                                                  \
        return guarded(ctx, [&] {                                                                                                        \
            RC_REQUIRE(out != nullptr, RC_INVALID_ARGUMENT, "rsvd_id_row_sharded: null output descriptor");                              \
            rsvd_id_row_sharded<T>(comm, ctx, from_c<T>(a_local), k, p, seed, *out);                                                     \
        });                                                                                                                              \
    }                                                                                                                                    \
    rc_status rc_column_id_rank_##SUF(rc_context *ctx, rc_matrix a, int64_t k, rc_matrix c, rc_matrix z, int64_t *col_ind) {             \
        return guarded(ctx, [&] { column_id_rank<T>(ctx, from_c<T>(a), k, from_c<T>(c), from_c<T>(z), col_ind); });                      \
    }

RC_DEFINE_TYPED(f64, double)
RC_DEFINE_TYPED(f32, float)
RC_DEFINE_DENSE_SHARED(f64, double, double)
RC_DEFINE_DENSE_SHARED(f32, float, float)

}  // extern "C"
