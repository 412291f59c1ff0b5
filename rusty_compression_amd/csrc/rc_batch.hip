// Batches of independent matrices (BASELINE.json configs[4]: 64 x (4096 x 4096 f32), rank-64 column ID, 8 per GPU)
// and the one exchange step of the path: the gather of the finished factor blocks over RCCL.
//
// Reference call sequence per matrix (examples/interpolative_decomposition.rs:25-32):
//     QR::compute_from(a) -> compress(RANK(k)) -> column_id()
// (src/qr.rs:354-362 via pivoted_qr, :169-184, :270-309).  The reference has no batch or communication layer: it is
// single-process host code; SURVEY.md section 8(b) / 8(e) define these entry points.
//
// rc_batch_column_id_*: the matrices of one GPU are spread over the caller's contexts (one stream each) and pipelined: every
// lane carries an event behind its ?laqps panel (the panel length is data dependent, so the host has to look at its state),
// the host serves the lanes first in, first out -- wait for that lane only, issue its panel-end kernels and its next panel,
// or its C, Z, ind and the set-up of the lane's next matrix -- so the latency-bound pivot steps of some matrices overlap the
// streaming kernels and the host-side launches of the others.  Results land in one packed device buffer, which is exactly
// what rc_comm_gather moves.
//
// RCCL is opened at run time (dlopen) so that the library has no link-time dependency on it: hosts that never gather,
// and the CPU-side symbol tests, do not need it.  Inside a PyTorch process the soname resolves to the copy torch loaded.
#include "rc_common.hpp"
#include <chrono>

#include <dlfcn.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <deque>
#include <mutex>
#include <vector>

using namespace rc;

namespace {

template <typename T>
void batch_column_id(rc_context *const *ctxs, int nctx, const rc_matrix *mats, int count, int64_t k, void *packed) {
    RC_REQUIRE(nctx >= 1 && count >= 0 && k >= 1, RC_INVALID_ARGUMENT, "batch_column_id: need >= 1 context, k >= 1");
    if (count == 0) return;
    RC_REQUIRE(mats != nullptr && packed != nullptr, RC_INVALID_ARGUMENT, "batch_column_id: null argument");
    const int64_t m = mats[0].rows, n = mats[0].cols;
    for (int i = 0; i < count; ++i)
        RC_REQUIRE(mats[i].rows == m && mats[i].cols == n && mats[i].data, RC_INVALID_ARGUMENT, "batch_column_id: all matrices must have the shape of the first");
    RC_REQUIRE(k <= std::min(m, n), RC_INVALID_ARGUMENT, "batch_column_id: rank %lld exceeds min(m, n)", (long long)k);
    for (int l = 0; l < nctx; ++l) RC_REQUIRE(ctxs[l] && !ctxs[l]->capturing, RC_INVALID_ARGUMENT, "batch_column_id: bad context");
    // which lane a matrix runs on depends on the timing: the lanes must all choose the factorization ctxs[0] chooses, on its device
    for (int l = 1; l < nctx; ++l) {
        const rc_context *a = ctxs[0], *b = ctxs[l];
        RC_REQUIRE(b->device == a->device, RC_INVALID_ARGUMENT, "batch_column_id: context %d is on device %d, context 0 on device %d", l, b->device, a->device);
        RC_REQUIRE(!b->opt_blocked == !a->opt_blocked && !b->opt_coop_panel == !a->opt_coop_panel && !b->opt_tsqr == !a->opt_tsqr &&
                       !b->opt_wide_coop == !a->opt_wide_coop && !b->opt_wide_lazy == !a->opt_wide_lazy,
                   RC_INVALID_ARGUMENT, "batch_column_id: context %d differs from context 0 in an option that selects the factorization (RC_OPT_BLOCKED_QRCP, "
                   "RC_OPT_COOP_PANEL, RC_OPT_TALL_SKINNY_FAST_PATH, RC_OPT_WIDE_COOP_QRCP, RC_OPT_WIDE_LAZY_QRCP)", l);
        // (what the launches are sized for: the K splits of the products and the launches of the small pivoted QR follow it, and bits with them)
        RC_REQUIRE(b->lanes_in_flight() == a->lanes_in_flight(), RC_INVALID_ARGUMENT,
                   "batch_column_id: context %d sizes its launches for %d compressions in flight, context 0 for %d (min(RC_OPT_CONCURRENCY_HINT, RC_OPT_KERNEL_SLOTS))", l,
                   b->lanes_in_flight(), a->lanes_in_flight());
    }
    // the lone call's route (rc_api.hip): the truncated blocked factorization, pipelined below, or the lone call's own routine on the lane
    const bool blocked = column_id_blocked_route<T>(ctxs[0], m, n, k);
    struct Lane {
        rc_context *c = nullptr;
        int idx = -1;
        Mat<T> w;
        int64_t *ind = nullptr;
        QrbJobPtr<T> job;  // non-null while the lane has a blocked factorization in progress
    };
    std::vector<Lane> lanes((size_t)nctx);
    for (int l = 0; l < nctx; ++l) lanes[(size_t)l].c = ctxs[l];
    // Every lane is quiescent before the jobs go and before the call returns -- also when it unwinds on an error: any lane may still have
    // work in flight, and the caller frees `packed` and reuses the arenas afterwards.  The lanes own their jobs, so this depends on the
    // order of declaration: `quiesce` stands AFTER `lanes` and is therefore destroyed (waits) BEFORE them.
    struct Quiesce {
        rc_context *const *ctxs;
        int nctx;
        ~Quiesce() { (void)rc_synchronize_all(ctxs, (int32_t)nctx); }
    } quiesce{ctxs, nctx};
    // Set-up of matrix idx on a lane.  Blocked route: working copy and the job of the blocked factorization (true: the caller issues its
    // panels and the lane has something to finish).  Every other route (tall-skinny, short-wide, k == n, shapes the panels do not take):
    // the lone call's own routine, whole, on the lane's stream into the slot (false: nothing left to do)
    auto start = [&](Lane &ln, int idx) -> bool {
        ln.idx = idx;
        DeviceGuard dg(ln.c->device);
        ln.c->reset_arena();
        if (!blocked) {
            const PackedSlot<T> s = packed_slot<T>(packed, idx, m, n, k);
            // (the permutation is built in a lane-owned buffer; it is copied into the packed slot at the end)
            ln.ind = ln.c->template alloc<int64_t>((size_t)n);
            column_id_rank<T>(ln.c, from_c<T>(mats[idx]), k, s.cm, s.z, ln.ind);
            RC_HIP(hipMemcpyAsync(s.ind, ln.ind, (size_t)n * sizeof(int64_t), hipMemcpyDeviceToDevice, ln.c->stream));
            return false;
        }
        ln.w = tmp_colmajor_pitch4<T>(ln.c, m, n);
        T *tau = ln.c->template alloc<T>((size_t)k);
        ln.ind = ln.c->template alloc<int64_t>((size_t)n);
        copy_mat(ln.c, from_c<T>(mats[idx]), ln.w);  // the reference's F-order working copy (pivoted_qr.rs:28-29)
        ln.job = qrb_begin<T>(ln.c, ln.w, k, ln.ind, tau);
        return true;
    };
    // C, Z and ind of a finished blocked factorization into the matrix's slot: read from the factored working copy, no Q (the lone call's
    // tail).  The job is done with: the lane is free for its next matrix.
    auto post = [&](Lane &ln) {
        const PackedSlot<T> s = packed_slot<T>(packed, ln.idx, m, n, k);
        column_id_from_qrcp(ln.c, from_c<T>(mats[ln.idx]), ln.w, k, ln.ind, s.cm, s.z);
        RC_HIP(hipMemcpyAsync(s.ind, ln.ind, (size_t)n * sizeof(int64_t), hipMemcpyDeviceToDevice, ln.c->stream));
        ln.job.reset();
    };
    // Optimistic schedule (default where it applies: blocked factorization on cooperative panels, no Q wanted): EVERY matrix is
    // enqueued in full on its lane -- all panels on their usual outcome (qrb_issue_optimistic), then C, Z, ind -- with no host
    // wait in between; one wait for all lanes at the end, then the per-panel states are checked and the (rare) matrices whose
    // assumptions failed are redone through the per-panel pipeline below.  The lanes' chains then overlap on the GPU without the
    // bubbles of a host round trip per panel.  Measured (8 x 4096^2 f32, k = 64): the host issues the 8 matrices in 0.6 ms and waits 2.05 ms --
    // the batch is bound on the GPU, so this schedule by itself is neutral against the pipeline below (2560 matrices/s either way); with 256
    // instead of 512 candidates per panel both reach 2810-2860.
    std::vector<int> todo;  // what is left to do through the per-panel schedule: everything, or the matrices the optimistic pass has to redo
    auto everything = [&] {
        todo.clear();
        for (int i2 = 0; i2 < count; ++i2) todo.push_back(i2);
    };
    static const int opt_on = env_int("RC_BATCH_OPTIMISTIC", 1), dbg = env_int("RC_BATCH_DEBUG", 0);
    if (opt_on && blocked) {
        struct Pending { int idx; QrbOptimistic o; };
        std::vector<Pending> pending;
        // all lanes waited for: check what is pending; the pinned slots are free again
        auto flush = [&] {
            RC_REQUIRE(rc_synchronize_all(ctxs, (int32_t)nctx) == RC_OK, RC_RUNTIME_ERROR, "batch_column_id: wait failed");
            for (auto &pd : pending)
                if (!pd.o.verified()) todo.push_back(pd.idx);
            pending.clear();
            for (auto &ln : lanes) ln.c->reset_pinned_slots();
        };
        bool possible = true;
        int flushes = 0;  // waits in the middle of the pass: a lane ran out of pinned state slots
        const auto t_begin = std::chrono::steady_clock::now();
        for (auto &ln : lanes) ln.c->reset_pinned_slots();
        for (int idx = 0; idx < count && possible; ++idx) {
            Lane &ln = lanes[(size_t)(idx % nctx)];
            start(ln, idx);
            QrbOptimistic o = qrb_issue_optimistic(ln.job.get());
            if (o.status == QrbOptimistic::NoSlots) {  // no pinned slots left on this lane: wait, check, go on
                flush();
                ++flushes;
                o = qrb_issue_optimistic(ln.job.get());
                RC_REQUIRE(o.status == QrbOptimistic::Issued, RC_RUNTIME_ERROR, "batch_column_id: no pinned state slots");
            }
            if (o.status == QrbOptimistic::Issued) {
                pending.push_back({idx, o});
                post(ln);
            } else {  // (first matrix only in practice: all matrices share one shape) -- everything through the pipeline below
                possible = false;
                ln.job.reset();
                flush();
                everything();
            }
        }
        const auto t_issued = std::chrono::steady_clock::now();
        if (possible) flush();
        if (dbg) {
            const auto t_end = std::chrono::steady_clock::now();
            std::string which;  // the matrices to redo, by index
            for (int i2 : todo) which += " " + std::to_string(i2);
            fprintf(stderr, "rc_batch optimistic: %d matrices issued in %.3f ms, waited %.3f ms, %zu to redo, %d flushes, redo:%s\n", count,
                    std::chrono::duration<double, std::milli>(t_issued - t_begin).count(), std::chrono::duration<double, std::milli>(t_end - t_issued).count(), todo.size(), flushes,
                    which.c_str());
        }
    } else {
        everything();
    }
    // Pipeline: every lane carries an event behind its panel; the host serves the lanes in the order their panels were
    // issued (first in, first out): wait for that lane only, enqueue its panel-end kernels and its next panel (or its C, Z,
    // ind and the set-up of the lane's next matrix), go on to the next lane.  The lanes drift apart by the host time of one
    // lane's launches, so the host-bound phases of some matrices (dozens of small launches) run while the latency-bound
    // cooperative panels of the others occupy the GPU, instead of everything waiting for the slowest panel of a round.
    // (All lanes are on ctxs[0]'s device, which the entry point's guard has made current.)
    auto issue = [&](Lane &ln) {
        rc_context *c = ln.c;
        qrb_issue(ln.job.get());
        if (!c->sync_ev) RC_HIP(hipEventCreateWithFlags(&c->sync_ev, hipEventDisableTiming));
        RC_HIP(hipEventRecord(c->sync_ev, c->stream));
    };
    size_t next = 0;
    std::deque<int> fifo;
    for (;;) {
        for (int l = 0; l < nctx && next < todo.size(); ++l) {  // idle lanes take the next matrices
            Lane &ln = lanes[(size_t)l];
            if (ln.job) continue;
            if (start(ln, todo[next++])) {
                issue(ln);
                fifo.push_back(l);
            }
        }
        if (fifo.empty()) {
            if (next >= todo.size()) break;
            continue;
        }
        const int l = fifo.front();
        Lane &ln = lanes[(size_t)l];
        fifo.pop_front();
        RC_HIP(hipEventSynchronize(ln.c->sync_ev));
        if (qrb_finish(ln.job.get())) {
            post(ln);  // (the lane is handed its next matrix at the top of the loop)
        } else {
            issue(ln);
            fifo.push_back(l);
        }
    }
    RC_REQUIRE(rc_synchronize_all(ctxs, (int32_t)nctx) == RC_OK, RC_RUNTIME_ERROR, "batch_column_id: wait failed");
}

// ---------------------------------------------------------------- RCCL, opened at run time
struct Rccl {
    void *handle = nullptr;
    ncclResult_t (*GetUniqueId)(ncclUniqueId *) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t *, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*Send)(const void *, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*Recv)(void *, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*AllGather)(const void *, void *, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*AllReduce)(const void *, void *, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*GroupStart)() = nullptr;
    ncclResult_t (*GroupEnd)() = nullptr;
    const char *(*GetErrorString)(ncclResult_t) = nullptr;
    std::string error;
};

Rccl *rccl() {
    static Rccl r;
    static std::once_flag once;
    std::call_once(once, [] {
        for (const char *name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
            r.handle = dlopen(name, RTLD_NOW | RTLD_LOCAL);
            if (r.handle) break;
        }
        if (!r.handle) { r.error = std::string("librccl could not be opened: ") + dlerror(); return; }
        auto sym = [&](const char *n) { void *p = dlsym(r.handle, n); if (!p && r.error.empty()) r.error = std::string("RCCL symbol missing: ") + n; return p; };
        r.GetUniqueId = reinterpret_cast<decltype(r.GetUniqueId)>(sym("ncclGetUniqueId"));
        r.CommInitRank = reinterpret_cast<decltype(r.CommInitRank)>(sym("ncclCommInitRank"));
        r.CommDestroy = reinterpret_cast<decltype(r.CommDestroy)>(sym("ncclCommDestroy"));
        r.Send = reinterpret_cast<decltype(r.Send)>(sym("ncclSend"));
        r.Recv = reinterpret_cast<decltype(r.Recv)>(sym("ncclRecv"));
        r.AllGather = reinterpret_cast<decltype(r.AllGather)>(sym("ncclAllGather"));
        r.AllReduce = reinterpret_cast<decltype(r.AllReduce)>(sym("ncclAllReduce"));
        r.GroupStart = reinterpret_cast<decltype(r.GroupStart)>(sym("ncclGroupStart"));
        r.GroupEnd = reinterpret_cast<decltype(r.GroupEnd)>(sym("ncclGroupEnd"));
        r.GetErrorString = reinterpret_cast<decltype(r.GetErrorString)>(sym("ncclGetErrorString"));
    });
    return &r;
}

}  // namespace

struct rc_comm {
    ncclComm_t comm = nullptr;  // RCCL transport (rc_comm_init), or
    rc_host_all_gather_fn host_gather = nullptr;  // the host's own collectives (rc_comm_init_host): buffers staged through the host
    rc_host_all_reduce_sum_fn host_reduce = nullptr;
    void *user = nullptr;
    std::vector<char> stage_in, stage_out;
    int world = 1, rank = 0, device = 0;
    std::string last_error;
};

extern "C" {

size_t rc_batch_packed_bytes(int64_t m, int64_t n, int64_t k, int32_t elem_size) {
    if (m < 0 || n < 0 || k < 0 || elem_size <= 0) return 0;
    const size_t cz = ((size_t)m * (size_t)k + (size_t)k * (size_t)n) * (size_t)elem_size;  // C and Z; the indices follow 8-byte aligned
    return ((cz + 7) & ~(size_t)7) + (size_t)n * 8;
}

rc_status rc_batch_shard_range(int64_t n_items, int32_t world, int32_t rank, int64_t *start, int64_t *count) {
    if (n_items < 0 || world < 1 || rank < 0 || rank >= world || !start || !count) return RC_INVALID_ARGUMENT;
    const int64_t base = n_items / world, extra = n_items % world;
    *start = rank * base + std::min<int64_t>(rank, extra);
    *count = base + (rank < extra ? 1 : 0);
    return RC_OK;
}

rc_status rc_batch_column_id_f64(rc_context *const *ctxs, int32_t nctx, const rc_matrix *mats, int32_t count, int64_t k, void *packed) {
    if (!ctxs || nctx < 1 || !ctxs[0]) return RC_INVALID_ARGUMENT;
    return guarded(ctxs[0], [&] { batch_column_id<double>(ctxs, nctx, mats, count, k, packed); });
}
rc_status rc_batch_column_id_f32(rc_context *const *ctxs, int32_t nctx, const rc_matrix *mats, int32_t count, int64_t k, void *packed) {
    if (!ctxs || nctx < 1 || !ctxs[0]) return RC_INVALID_ARGUMENT;
    return guarded(ctxs[0], [&] { batch_column_id<float>(ctxs, nctx, mats, count, k, packed); });
}

rc_status rc_comm_unique_id(void *id128) {
    if (!id128) return RC_INVALID_ARGUMENT;
    Rccl *r = rccl();
    if (!r->error.empty()) return RC_RUNTIME_ERROR;
    ncclUniqueId id;
    if (r->GetUniqueId(&id) != ncclSuccess) return RC_RUNTIME_ERROR;
    static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId is 128 bytes");
    std::memcpy(id128, &id, sizeof(id));
    return RC_OK;
}

rc_status rc_comm_init(rc_comm **comm, int32_t world, int32_t rank, const void *id128, int32_t device) {
    if (!comm) return RC_INVALID_ARGUMENT;
    *comm = nullptr;
    if (world < 1 || rank < 0 || rank >= world || !id128) return RC_INVALID_ARGUMENT;
    Rccl *r = rccl();
    if (!r->error.empty()) return RC_RUNTIME_ERROR;
    DeviceGuard dg(device);
    ncclUniqueId id;
    std::memcpy(&id, id128, sizeof(id));
    rc_comm *c = new rc_comm();
    c->world = world; c->rank = rank; c->device = device;
    if (r->CommInitRank(&c->comm, world, id, rank) != ncclSuccess) { delete c; return RC_RUNTIME_ERROR; }
    *comm = c;
    return RC_OK;
}

const char *rc_comm_last_error_message(const rc_comm *comm) {
    if (comm) return comm->last_error.c_str();
    return rccl()->error.c_str();
}

// Gather `bytes_per_rank` bytes from every rank into recv[rank * bytes_per_rank ...] on `root`, on the context's stream
// (asynchronous; grouped ncclSend / ncclRecv: every peer uses its own direct xGMI link to the root).
rc_status rc_comm_gather(rc_comm *comm, rc_context *ctx, const void *send, void *recv, size_t bytes_per_rank, int32_t root) {
    if (!comm || !ctx || root < 0 || root >= comm->world) return RC_INVALID_ARGUMENT;
    if (bytes_per_rank == 0) return RC_OK;
    if (!send || (comm->rank == root && !recv)) return RC_INVALID_ARGUMENT;
    if (!comm->comm) {  // host transport: the gather is the all-gather's block on the root
        comm->last_error = "rc_comm_gather needs the RCCL transport (use rc_comm_all_gather with a host communicator)";
        ctx->last_error = comm->last_error;
        return RC_INVALID_ARGUMENT;
    }
    Rccl *r = rccl();
    DeviceGuard dg(comm->device);
    auto chk = [&](ncclResult_t e) {
        if (e == ncclSuccess) return true;
        comm->last_error = r->GetErrorString ? r->GetErrorString(e) : "RCCL error";
        ctx->last_error = comm->last_error;
        return false;
    };
    bool ok = chk(r->GroupStart());
    if (ok && comm->rank == root)
        for (int p = 0; ok && p < comm->world; ++p)
            ok = chk(r->Recv(static_cast<char *>(recv) + (size_t)p * bytes_per_rank, bytes_per_rank, ncclUint8, p, comm->comm, ctx->stream));
    if (ok) ok = chk(r->Send(send, bytes_per_rank, ncclUint8, root, comm->comm, ctx->stream));
    const bool ended = chk(r->GroupEnd());
    return ok && ended ? RC_OK : RC_RUNTIME_ERROR;
}

rc_status rc_comm_init_host(rc_comm **comm, int32_t world, int32_t rank, int32_t device, rc_host_all_gather_fn all_gather,
                            rc_host_all_reduce_sum_fn all_reduce_sum, void *user) {
    if (!comm) return RC_INVALID_ARGUMENT;
    *comm = nullptr;
    if (world < 1 || rank < 0 || rank >= world || !all_gather || !all_reduce_sum) return RC_INVALID_ARGUMENT;
    rc_comm *c = new rc_comm();
    c->world = world; c->rank = rank; c->device = device;
    c->host_gather = all_gather; c->host_reduce = all_reduce_sum; c->user = user;
    *comm = c;
    return RC_OK;
}

rc_status rc_comm_world(const rc_comm *comm, int32_t *world, int32_t *rank) {
    if (!comm) return RC_INVALID_ARGUMENT;
    if (world) *world = comm->world;
    if (rank) *rank = comm->rank;
    return RC_OK;
}

namespace {
bool comm_fail(rc_comm *comm, rc_context *ctx, const std::string &msg) {
    comm->last_error = msg;
    ctx->last_error = msg;
    return false;
}
bool comm_hip(rc_comm *comm, rc_context *ctx, hipError_t e, const char *what) {
    return e == hipSuccess ? true : comm_fail(comm, ctx, std::string(what) + ": " + hipGetErrorString(e));
}
}  // namespace

// recv[r * bytes_per_rank ...] = rank r's `send`, on every rank, ordered on the context's stream.  `send` may be the
// rank's own block inside `recv` (in place).  RCCL transport: asynchronous (ncclAllGather); host transport: the stream is
// waited for, the host's callback runs on host copies, the result is copied back before the call returns.
rc_status rc_comm_all_gather(rc_comm *comm, rc_context *ctx, const void *send, void *recv, size_t bytes_per_rank) {
    if (!comm || !ctx) return RC_INVALID_ARGUMENT;
    if (bytes_per_rank == 0) return RC_OK;
    if (!send || !recv) return RC_INVALID_ARGUMENT;
    DeviceGuard dg(comm->device);
    char *own = static_cast<char *>(recv) + (size_t)comm->rank * bytes_per_rank;
    if (comm->world == 1 && !comm->comm) {  // (an RCCL communicator of one rank still goes through ncclAllGather)
        if (own != send && !comm_hip(comm, ctx, hipMemcpyAsync(own, send, bytes_per_rank, hipMemcpyDeviceToDevice, ctx->stream), "all_gather copy")) return RC_RUNTIME_ERROR;
        return RC_OK;
    }
    if (comm->host_gather) {
        comm->stage_in.resize(bytes_per_rank);
        comm->stage_out.resize(bytes_per_rank * (size_t)comm->world);
        if (!comm_hip(comm, ctx, hipMemcpyAsync(comm->stage_in.data(), send, bytes_per_rank, hipMemcpyDeviceToHost, ctx->stream), "all_gather D2H")) return RC_RUNTIME_ERROR;
        if (!comm_hip(comm, ctx, hipStreamSynchronize(ctx->stream), "all_gather wait")) return RC_RUNTIME_ERROR;
        if (comm->host_gather(comm->user, comm->stage_in.data(), comm->stage_out.data(), bytes_per_rank) != 0) {
            comm_fail(comm, ctx, "the host's all_gather callback reported an error");
            return RC_RUNTIME_ERROR;
        }
        if (!comm_hip(comm, ctx, hipMemcpyAsync(recv, comm->stage_out.data(), comm->stage_out.size(), hipMemcpyHostToDevice, ctx->stream), "all_gather H2D")) return RC_RUNTIME_ERROR;
        if (!comm_hip(comm, ctx, hipStreamSynchronize(ctx->stream), "all_gather wait")) return RC_RUNTIME_ERROR;
        return RC_OK;
    }
    Rccl *r = rccl();
    if (!r->error.empty() || !r->AllGather || !comm->comm) { comm_fail(comm, ctx, r->error.empty() ? "communicator has no transport" : r->error); return RC_RUNTIME_ERROR; }
    ncclResult_t e = r->AllGather(send, recv, bytes_per_rank, ncclUint8, comm->comm, ctx->stream);
    if (e != ncclSuccess) { comm_fail(comm, ctx, r->GetErrorString ? r->GetErrorString(e) : "RCCL error"); return RC_RUNTIME_ERROR; }
    return RC_OK;
}

// buf[i] = sum over the ranks of buf[i], in place, the same bits on every rank; elem_size 8: double, 4: float
rc_status rc_comm_all_reduce_sum(rc_comm *comm, rc_context *ctx, void *buf, size_t count, int32_t elem_size) {
    if (!comm || !ctx || (elem_size != 4 && elem_size != 8)) return RC_INVALID_ARGUMENT;
    if (count == 0 || (comm->world == 1 && !comm->comm)) return RC_OK;
    if (!buf) return RC_INVALID_ARGUMENT;
    DeviceGuard dg(comm->device);
    const size_t bytes = count * (size_t)elem_size;
    if (comm->host_reduce) {
        comm->stage_in.resize(bytes);
        if (!comm_hip(comm, ctx, hipMemcpyAsync(comm->stage_in.data(), buf, bytes, hipMemcpyDeviceToHost, ctx->stream), "all_reduce D2H")) return RC_RUNTIME_ERROR;
        if (!comm_hip(comm, ctx, hipStreamSynchronize(ctx->stream), "all_reduce wait")) return RC_RUNTIME_ERROR;
        if (comm->host_reduce(comm->user, comm->stage_in.data(), count, elem_size) != 0) {
            comm_fail(comm, ctx, "the host's all_reduce callback reported an error");
            return RC_RUNTIME_ERROR;
        }
        if (!comm_hip(comm, ctx, hipMemcpyAsync(buf, comm->stage_in.data(), bytes, hipMemcpyHostToDevice, ctx->stream), "all_reduce H2D")) return RC_RUNTIME_ERROR;
        if (!comm_hip(comm, ctx, hipStreamSynchronize(ctx->stream), "all_reduce wait")) return RC_RUNTIME_ERROR;
        return RC_OK;
    }
    Rccl *r = rccl();
    if (!r->error.empty() || !r->AllReduce || !comm->comm) { comm_fail(comm, ctx, r->error.empty() ? "communicator has no transport" : r->error); return RC_RUNTIME_ERROR; }
    ncclResult_t e = r->AllReduce(buf, buf, count, elem_size == 8 ? ncclDouble : ncclFloat, ncclSum, comm->comm, ctx->stream);
    if (e != ncclSuccess) { comm_fail(comm, ctx, r->GetErrorString ? r->GetErrorString(e) : "RCCL error"); return RC_RUNTIME_ERROR; }
    return RC_OK;
}

rc_status rc_comm_destroy(rc_comm *comm) {
    if (!comm) return RC_OK;
    Rccl *r = rccl();
    DeviceGuard dg(comm->device);
    if (comm->comm && r->CommDestroy) (void)r->CommDestroy(comm->comm);
    delete comm;
    return RC_OK;
}

}  // extern "C"
