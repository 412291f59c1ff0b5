// Small-core SVD for gfx950: one-sided (Hestenes) Jacobi on a square n x n
// matrix, n <= 1024.
//
// Replaces the dense core of LAPACK ?gesdd as the reference reaches it through
// ndarray-linalg `svddc_into(JobSvd::Some)` (/root/reference/src/compute_svd.rs:19).
// The tall/wide input is first reduced to its square triangular factor by the
// Householder QR of kernels_qr.hip (rc_api.hip: svd_core), so this file only
// ever sees min(m, n) x min(m, n).  One-sided Jacobi computes every singular
// value to high RELATIVE accuracy, which is what the f64 <= 1e-12 round-trip
// bound of the reference tests (src/svd.rs:290-297) needs.
//
// MI355X mapping
//  * k_jacobi_lds: the whole core lives in the 160 KiB LDS of ONE CU (128 x 128
//    f64 = 128 KiB).  Round-robin (circle) ordering gives n/2 independent column
//    pairs per round; 16 lanes (one DPP row) own a pair, keep both columns in
//    registers between the three dot products and the rotation (one LDS read +
//    one LDS write of the pair per round), reduce with DPP row operations (no
//    LDS traffic for the reductions) and the 1024-thread workgroup needs ONE
//    barrier per round.  Every rotation (c, s) is published to a log in HBM
//    (write-only stream); up to n = 128 a second workgroup of the same launch
//    accumulates the right singular vectors from it as it is written.
//  * k_jacobi_replay_v: V = product of the logged rotations for the larger
//    cores.  Rotations act on columns, so every ROW of V is independent: one
//    wave per row keeps its row in LDS and streams the log -- no barrier at all.
//  * k_jacobi_global: fallback for cores that do not fit LDS (n <= 1024),
//    everything in L2-resident global memory.
#include "rc_common.hpp"
#include "rc_device.hpp"

namespace rc {

template <typename T> __device__ inline T dpp_row_sum(T v) { return group_sum_dpp<16>(v); }

// Workgroup barrier that orders LDS traffic only.  __syncthreads() also waits for
// outstanding GLOBAL stores (vmcnt(0)); the rotation-log stores are write-only and
// must stay in flight across rounds, so the round barrier waits for lgkmcnt alone.
__device__ inline void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// one rotation record of the log
template <typename T> struct Rot { T c, s; };

// Fused right-vector accumulation (second workgroup of k_jacobi_lds): the records travel from the producer to the
// consumer workgroup through agent-scope atomics and the producer never waits for its stores.  Every record has a
// check word hash(c, s) ^ magic ^ f(epoch); the epoch is a per-context device counter that both workgroups read at
// their start and the consumer bumps at its end, so a torn combination, or a complete record of an EARLIER launch
// that still sits at the same workspace address, never validates -- nothing has to be cleared before a launch.
#define RC_AGENT __HIP_MEMORY_SCOPE_AGENT
constexpr unsigned long long kRotMagic = 0x9e3779b97f4a7c15ull;
__device__ inline unsigned long long rot_hash(Rot<double> r) { return (unsigned long long)__double_as_longlong(r.c) ^ ((unsigned long long)__double_as_longlong(r.s) * 3ull); }
__device__ inline unsigned long long rot_hash(Rot<float> r) { return ((unsigned long long)__float_as_uint(r.s) << 32) | __float_as_uint(r.c); }
__device__ inline unsigned long long epoch_key(unsigned e) { return kRotMagic ^ ((unsigned long long)e * 0xd1342543de82ef95ull); }
__device__ inline void rot_publish(Rot<double> *p, unsigned long long *chk, Rot<double> r, unsigned long long key) {
    __hip_atomic_store(&p->c, r.c, __ATOMIC_RELAXED, RC_AGENT);
    __hip_atomic_store(&p->s, r.s, __ATOMIC_RELAXED, RC_AGENT);
    __hip_atomic_store(chk, rot_hash(r) ^ key, __ATOMIC_RELAXED, RC_AGENT);
}
__device__ inline void rot_publish(Rot<float> *p, unsigned long long *chk, Rot<float> r, unsigned long long key) {
    __hip_atomic_store(reinterpret_cast<unsigned long long *>(p), rot_hash(r), __ATOMIC_RELAXED, RC_AGENT);
    __hip_atomic_store(chk, rot_hash(r) ^ key, __ATOMIC_RELAXED, RC_AGENT);
}
__device__ inline bool rot_fetch(const Rot<double> *p, const unsigned long long *chk, Rot<double> &r, unsigned long long key) {
    r.c = __hip_atomic_load(&p->c, __ATOMIC_RELAXED, RC_AGENT);
    r.s = __hip_atomic_load(&p->s, __ATOMIC_RELAXED, RC_AGENT);
    return __hip_atomic_load(chk, __ATOMIC_RELAXED, RC_AGENT) == (rot_hash(r) ^ key);
}
__device__ inline bool rot_fetch(const Rot<float> *p, const unsigned long long *chk, Rot<float> &r, unsigned long long key) {
    const unsigned long long w = __hip_atomic_load(reinterpret_cast<const unsigned long long *>(p), __ATOMIC_RELAXED, RC_AGENT);
    r.c = __uint_as_float((unsigned)w);
    r.s = __uint_as_float((unsigned)(w >> 32));
    return __hip_atomic_load(chk, __ATOMIC_RELAXED, RC_AGENT) == (w ^ key);
}
// small integers (sweep count, sorted position + 1) travel as (epoch << 8) | payload
__device__ inline void tagged_put(unsigned *p, unsigned e, unsigned payload) { __hip_atomic_store(p, (e << 8) | payload, __ATOMIC_RELAXED, RC_AGENT); }
__device__ inline unsigned tagged_get(const unsigned *p, unsigned e) {  // 0 = not there yet
    const unsigned w = __hip_atomic_load(p, __ATOMIC_RELAXED, RC_AGENT);
    return (w >> 8) == (e & 0xffffffu) ? (w & 0xffu) : 0u;
}

__global__ void k_clear_words(unsigned *p, int n) {
    for (int i = threadIdx.x; i < n; i += blockDim.x) p[i] = 0u;
}

// Lanes per column pair: one DPP row.
constexpr int kLPP = 16;
static_assert(kMaxSweeps < 255, "sweep count must fit a tagged word");

// ---------------------------------------------------------------------------
// LDS-resident one-sided Jacobi.  16 lanes own one column pair and keep NE = n / 16 rows (rounded up) of both columns in
// registers; 1024 threads = 64 groups, one per pair slot of a 128 x 128 core.
//   g      : n x n column-major input (global), destroyed
//   log    : [max_sweeps][N-1][N/2] rotations (c = 1, s = 0 where none)
//   sweeps : number of sweeps performed (device scalar out)
//   uc, s  : left singular vectors / singular values, sorted descending
//   order  : order[j] = sorted position of original column j (for the V replay)
// ---------------------------------------------------------------------------
//   fused  : != 0: launched with TWO workgroups; the second one accumulates V from the published records while the first
//            is still rotating (vsync[0] = number of sweeps once known, vsync[1 + j] = order[j] + 1; both zeroed before)
// PROTOCOL INVARIANTS of the fused launch (two workgroups; reviewed against the code in round 3 -- keep list and code in step)
//  J1  One direction only: workgroup 0 (producer) publishes, workgroup 1 (consumer) reads; the producer never waits for the
//      consumer, so the two need not be co-resident and the producer's result (U, S) never depends on the consumer.
//  J2  Everything that crosses is an 8-byte (records, check words) or 4-byte (vsync) agent-scope relaxed atomic.  A rotation record
//      is valid iff its check word equals hash(c, s) ^ key(epoch): a torn combination of two publications and a complete record of
//      an EARLIER launch at the same workspace address (other epoch, other key) both fail the test, so records need no clearing.
//  J3  epoch is a per-context device counter, started at a pseudo-random 23-bit value, read by both workgroups at their start and
//      incremented by the consumer at its very end; launches of one context are stream ordered, so every launch sees a new epoch.
//  J4  The small hand-over words vsync[0] (number of sweeps) and vsync[1 + j] (sorted position + 1) travel as (epoch << 8) | payload
//      AND are cleared (k_clear_words, same stream, in front) before every launch: payload 0 means "not there yet".
//  J5  The consumer learns that sweep s exists from the first record of sweep s validating, and that it does not from
//      vsync[0] <= s; the producer writes exactly one of the two after sweep s - 1.  Index of a record: (sweep, round, pair slot),
//      the same expression on both sides (FULL: pair slot = group).
//  J6  Every consumer spin is bounded (kSpin); on expiry health bit 8 is raised and V is reported incomplete -- never silently wrong.
//   FULL   : n == 16 * NE and one group per pair slot: no row / column bounds, no slot loop (the round is bound by the
//            number of instructions the 16 waves issue, and the predicates were a quarter of them)
template <typename T, int NE, bool FULL>
__global__ __launch_bounds__(1024) void k_jacobi_lds(Mat<T> g, Rot<T> *log, int *sweeps_out, Mat<T> uc, T *s, int *order_out, int max_sweeps, int fused,
                                                  unsigned *vsync, unsigned long long *chk, unsigned *epoch_p, Mat<T> vc, int *health, int ld) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const int n = (int)g.rows;
    // ld: column pitch chosen by the host (jacobi_pitch): the two column groups of a 32-lane half read neighbouring columns
    T *G = reinterpret_cast<T *>(smem_raw);
    T *sig = G + (size_t)ld * n;
    int *order = reinterpret_cast<int *>(sig + n);
    // a static LDS word: behind a pointer into the dynamic array the compiler lost the address space and issued FLAT
    // stores + s_waitcnt vmcnt(0) for it, which also waited for the rotation records in flight
    __shared__ int sh_rot_word;
#define sh_rot sh_rot_word
    const int tid = threadIdx.x, nthr = blockDim.x;
    const int ll = tid % kLPP, grp = tid / kLPP, ngrp = nthr / kLPP;
    const int N = (n + 1) & ~1;
    const int npairs = N / 2;
    const unsigned epoch = fused ? __hip_atomic_load(epoch_p, __ATOMIC_RELAXED, RC_AGENT) & 0xffffffu : 0u;
    const unsigned long long key = epoch_key(epoch);
    if (fused && blockIdx.x == 1) {
        // ---- consumer: V = product of the rotations, columns in LDS, the producer's pairing (one slot per group) ----
        constexpr int kSpin = 1 << 24;
        T *V = G;
        for (int e = tid; e < n * n; e += nthr) {
            const int i = e % n, j = e / n;
            V[j * ld + i] = (i == j) ? (T)1 : (T)0;
        }
        __syncthreads();
        bool lost = false;
        for (int sweep = 0;; ++sweep) {
            if (tid == 0) {  // has the producer started this sweep, or did it finish before it?
                int fin = 2;
                for (int it = 0; it < kSpin; ++it) {
                    const unsigned d = tagged_get(vsync, epoch);
                    if (d != 0u && (int)d <= sweep) { fin = 1; break; }
                    Rot<T> r0;
                    if (sweep < max_sweeps && rot_fetch(log + (size_t)sweep * (N - 1) * npairs, chk + (size_t)sweep * (N - 1) * npairs, r0, key)) { fin = 0; break; }
                    __builtin_amdgcn_s_sleep(8);
                }
                sh_rot = fin;
            }
            __syncthreads();
            const int fin = sh_rot;
            __syncthreads();
            if (fin) { lost = fin == 2; break; }
            int pr = grp % (N - 1), qr = ((N - 1) - grp % (N - 1)) % (N - 1);
            for (int r = 0; r < N - 1; ++r) {
                if (FULL || grp < npairs) {
                    int p = grp == 0 ? N - 1 : pr, q = grp == 0 ? pr : qr;
                    if (p > q) { const int t = p; p = q; q = t; }
                    pr = pr + 1 == N - 1 ? 0 : pr + 1;
                    qr = qr + 1 == N - 1 ? 0 : qr + 1;
                    Rot<T> rot{(T)1, (T)0};
                    const size_t rec = ((size_t)sweep * (N - 1) + r) * npairs + grp;
                    bool ok = false;
                    for (int it = 0; it < kSpin && !(ok = rot_fetch(log + rec, chk + rec, rot, key)); ++it) __builtin_amdgcn_s_sleep(2);
                    if (!ok) lost = true;
                    if (ok && (FULL || q < n) && rot.s != (T)0) {
                        T *vp = V + p * ld, *vq = V + q * ld;
#pragma unroll
                        for (int e = 0; e < NE; ++e) {
                            const int i = ll + kLPP * e;
                            if (FULL || i < n) {
                                const T a = vp[i], b = vq[i];
                                vp[i] = rot.c * a - rot.s * b;
                                vq[i] = rot.s * a + rot.c * b;
                            }
                        }
                    }
                }
                lds_barrier();
            }
        }
        // columns go out in the sorted order the producer publishes at its very end
        for (int j = grp; j < n; j += ngrp) {
            unsigned enc = 0;
            for (int it = 0; it < kSpin && (enc = tagged_get(vsync + 1 + j, epoch)) == 0u; ++it) __builtin_amdgcn_s_sleep(8);
            if (enc == 0u) { lost = true; continue; }
            const int dst = (int)enc - 1;
            for (int i = ll; i < n; i += kLPP) vc.at(i, dst) = V[j * ld + i];
        }
        if (lost && ll == 0) atomicOr(health, 8);  // the producer never showed up within the spin bound: V is incomplete
        __syncthreads();
        if (tid == 0) __hip_atomic_fetch_add(epoch_p, 1u, __ATOMIC_RELAXED, RC_AGENT);  // the next launch uses a new key
        return;
    }
    const T tol = sqrt((T)n) * JEps<T>::eps();
    const T tol2 = tol * tol;

    for (int e = tid; e < n * n; e += nthr) {
        int i = e % n, j = e / n;
        G[j * ld + i] = g.p[(int64_t)j * g.cs + i];
    }
    __syncthreads();

    int sweep = 0;
    bool converged = false;
    for (; sweep < max_sweeps; ++sweep) {
        if (tid == 0) sh_rot = 0;
        __syncthreads();
        // circle-method pair of this group, advanced round by round when the group owns one pair slot (no integer
        // modulo on the per-round critical path): slot 0 pairs N - 1 with r, slot pi pairs (r + pi) with (r - pi) mod N - 1
        const bool one_slot = FULL || npairs <= ngrp;
        int pr = grp % (N - 1), qr = ((N - 1) - grp % (N - 1)) % (N - 1);
        for (int r = 0; r < N - 1; ++r) {
            for (int pi = grp; pi < npairs; pi += FULL ? (1 << 20) : ngrp) {  // FULL: exactly one trip
                int p, q;
                if (one_slot) {
                    p = grp == 0 ? N - 1 : pr;
                    q = grp == 0 ? pr : qr;
                    if (p > q) { const int t = p; p = q; q = t; }
                    pr = pr + 1 == N - 1 ? 0 : pr + 1;
                    qr = qr + 1 == N - 1 ? 0 : qr + 1;
                } else {
                    rr_pair(N, r, pi, p, q);
                }
                Rot<T> rot{(T)1, (T)0};
                if (FULL || q < n) {  // p < q; q == n is the dummy column of an odd n
                    T *gp = G + p * ld, *gq = G + q * ld;
                    T a[NE], b[NE];
                    T app = 0, aqq = 0, apq = 0;
#pragma unroll
                    for (int e = 0; e < NE; ++e) {
                        int i = ll + kLPP * e;
                        a[e] = (FULL || i < n) ? gp[i] : (T)0;
                        b[e] = (FULL || i < n) ? gq[i] : (T)0;
                        app = fma(a[e], a[e], app);
                        aqq = fma(b[e], b[e], aqq);
                        apq = fma(a[e], b[e], apq);
                    }
                    app = group_sum_dpp<kLPP>(app);
                    aqq = group_sum_dpp<kLPP>(aqq);
                    apq = group_sum_dpp<kLPP>(apq);
                    // rotate iff |apq| > tol * sqrt(app * aqq)   (uniform over the 16 lanes)
                    if (apq * apq > tol2 * app * aqq) {
                        jacobi_rotation(app, aqq, apq, rot.c, rot.s);
#pragma unroll
                        for (int e = 0; e < NE; ++e) {
                            int i = ll + kLPP * e;
                            if (FULL || i < n) {
                                gp[i] = rot.c * a[e] - rot.s * b[e];
                                gq[i] = rot.s * a[e] + rot.c * b[e];
                            }
                        }
                        // flag 2 = another sweep is needed.  A rotation by the angle (c, s) of a pair whose cosine was g leaves
                        // at most |s| * (largest cosine of this sweep) behind in pairs that were already annihilated, so a sweep
                        // may be the last one only if every rotation in it had BOTH a small cosine (g <= sqrt(tol) / 4, 9e-9 in
                        // f64) AND a small angle (|s| <= 4 sqrt(tol)): for well separated singular values the second follows
                        // from the first (quadratic convergence), for clustered / repeated ones (sigma_p ~ sigma_q: the angle is
                        // O(1) however small g is) it does not, and such sweeps are followed by another one until an all-quiet
                        // or all-small sweep has been seen
                        if (ll == 0 && (apq * apq > tol * (T)0.0625 * app * aqq || rot.s * rot.s > (T)16 * tol)) sh_rot = 2;  // plain store: every writer writes 2
                    }
                }
                if (ll == 0) {
                    if (fused) rot_publish(log + ((size_t)sweep * (N - 1) + r) * npairs + pi, chk + ((size_t)sweep * (N - 1) + r) * npairs + pi, rot, key);
                    else log[((size_t)sweep * (N - 1) + r) * npairs + pi] = rot;
                }
            }
            lds_barrier();  // pairs of one round are disjoint; the next round re-pairs the columns
        }
        const int rotated = sh_rot;
        __syncthreads();
        if (rotated < 2) { ++sweep; converged = true; break; }
    }
    // max_sweeps exhausted with rotations still above the thresholds: reported, never silent (health bit 4, value 16)
    if (tid == 0 && !converged && health) atomicOr(health, 16);
    if (tid == 0) {
        *sweeps_out = sweep;
        if (fused) tagged_put(vsync, epoch, (unsigned)sweep);
    }

    // singular values = column norms; stable descending rank sort (gesdd order)
    for (int j = grp; j < n; j += ngrp) {
        const T *gj = G + j * ld;
        T acc = 0;
        for (int i = ll; i < n; i += kLPP) acc += gj[i] * gj[i];
        acc = group_sum_dpp<kLPP>(acc);
        if (ll == 0) sig[j] = sqrt(acc);
    }
    __syncthreads();
    for (int i = tid; i < n; i += nthr) {
        int rank = 0;
        const T si = sig[i];
        for (int j = 0; j < n; ++j) rank += (sig[j] > si || (sig[j] == si && j < i)) ? 1 : 0;
        order[i] = rank;
        order_out[i] = rank;
        if (fused) tagged_put(vsync + 1 + i, epoch, (unsigned)(rank + 1));
        s[rank] = si;
    }
    __syncthreads();
    for (int j = grp; j < n; j += ngrp) {
        const int dst = order[j];
        const T sj = sig[j];
        const T inv = sj > (T)0 ? (T)1 / sj : (T)0;
        const T *gj = G + j * ld;
        for (int i = ll; i < n; i += kLPP) uc.at(i, dst) = gj[i] * inv;
    }
#undef sh_rot
}

// ---------------------------------------------------------------------------
// V = J_1 J_2 ... applied to I, row by row: one wave per row of V.  Runs for the cores the fused launch of k_jacobi_lds
// cannot take (more than 64 pair slots), so every lane walks several pair slots of a round.
// ---------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void k_jacobi_replay_v(int n, const Rot<T> *log, const int *sweeps, const int *order, Mat<T> vc) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    T *rows = reinterpret_cast<T *>(smem_raw);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int N = (n + 1) & ~1, npairs = N / 2;
    const int ns = *sweeps;
    const int row = blockIdx.x * 4 + wv;
    if (row >= n) return;  // whole wave; no barriers in this kernel
    T *v = rows + (size_t)wv * (n + 1);
    for (int j = lane; j < n; j += 64) v[j] = (j == row) ? (T)1 : (T)0;
    for (int sw = 0; sw < ns; ++sw)
        for (int r = 0; r < N - 1; ++r) {
            const Rot<T> *lr = log + ((size_t)sw * (N - 1) + r) * npairs;
            for (int pi = lane; pi < npairs; pi += 64) {
                const Rot<T> rot = lr[pi];
                if (rot.s != (T)0) {
                    int p, q;
                    rr_pair(N, r, pi, p, q);
                    T a = v[p], b = v[q];
                    v[p] = rot.c * a - rot.s * b;
                    v[q] = rot.s * a + rot.c * b;
                }
            }
            // a wave executes its LDS operations in order: the next round (other pairing of the
            // same row) sees these writes without a barrier
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        }
    for (int j = lane; j < n; j += 64) vc.at(row, order[j]) = v[j];
}

// ---------------------------------------------------------------------------
// Cores that do not fit the LDS of one CU: the same one-sided Jacobi with G and V in (L2-resident)
// global memory, one LAUNCH per round of the circle-method schedule -- the N/2 pairs of a round are
// disjoint, so one wave per pair needs no synchronisation inside the round and the whole chip works
// on it.  state[0] = "some pair rotated in this sweep", state[1] = converged, state[2] = sweeps done.
// ---------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void k_jacobi_round(Mat<T> g, Mat<T> v, int r, int *state) {
    if (state[1]) return;
    const int n = (int)g.rows, N = (n + 1) & ~1;
    const int lane = threadIdx.x & 63;
    const int pi = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (pi >= N / 2) return;
    int p, q;
    rr_pair(N, r, pi, p, q);
    if (q >= n) return;  // the dummy column of an odd n
    const T tol = sqrt((T)n) * JEps<T>::eps();
    T *gp = g.p + (int64_t)p * g.cs, *gq = g.p + (int64_t)q * g.cs;
    T app = 0, aqq = 0, apq = 0;
    for (int i = lane; i < n; i += 64) {
        const T a = gp[i], b = gq[i];
        app = fma(a, a, app);
        aqq = fma(b, b, aqq);
        apq = fma(a, b, apq);
    }
    app = wave_sum_dpp(app);
    aqq = wave_sum_dpp(aqq);
    apq = wave_sum_dpp(apq);
    if (apq == (T)0 || fabs(apq) <= tol * sqrt(app) * sqrt(aqq)) return;
    T cs, sn;
    jacobi_rotation(app, aqq, apq, cs, sn);
    for (int i = lane; i < n; i += 64) {
        const T a = gp[i], b = gq[i];
        gp[i] = cs * a - sn * b;
        gq[i] = sn * a + cs * b;
    }
    T *vp = v.p + (int64_t)p * v.cs, *vq = v.p + (int64_t)q * v.cs;
    for (int i = lane; i < n; i += 64) {
        const T a = vp[i], b = vq[i];
        vp[i] = cs * a - sn * b;
        vq[i] = sn * a + cs * b;
    }
    if (lane == 0) state[0] = 1;
}
__global__ void k_jacobi_check(const int *state, int *health) {
    if (threadIdx.x == 0 && !state[1]) atomicOr(health, 16);  // sweep budget exhausted before an all-quiet sweep
}
__global__ void k_jacobi_sweep_end(int *state) {
    if (threadIdx.x != 0 || state[1]) return;
    state[2] += 1;
    if (state[0] == 0) state[1] = 1;
    state[0] = 0;
}
// singular values = column norms of the rotated G; sig/order live in global memory
template <typename T>
__global__ __launch_bounds__(256) void k_jacobi_norms(Mat<T> g, T *sig) {
    const int n = (int)g.rows, lane = threadIdx.x & 63;
    const int j = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (j >= n) return;
    const T *gj = g.p + (int64_t)j * g.cs;
    T acc = 0;
    for (int i = lane; i < n; i += 64) { const T a = gj[i]; acc = fma(a, a, acc); }
    acc = wave_sum_dpp(acc);
    if (lane == 0) sig[j] = sqrt(acc);
}
template <typename T>
__global__ __launch_bounds__(256) void k_jacobi_rank(int n, const T *sig, int *order, T *s) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const T si = sig[i];
    int rank = 0;
    for (int j = 0; j < n; ++j) {
        const T sj = sig[j];
        rank += (sj > si || (sj == si && j < i)) ? 1 : 0;
    }
    order[i] = rank;
    s[rank] = si;
}
template <typename T>
__global__ __launch_bounds__(256) void k_jacobi_emit(Mat<T> g, Mat<T> v, const T *sig, const int *order, Mat<T> uc, Mat<T> vc) {
    const int n = (int)g.rows, lane = threadIdx.x & 63;
    const int j = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (j >= n) return;
    const int dst = order[j];
    const T sj = sig[j];
    const T inv = sj > (T)0 ? (T)1 / sj : (T)0;
    const T *gj = g.p + (int64_t)j * g.cs, *vj = v.p + (int64_t)j * v.cs;
    for (int i = lane; i < n; i += 64) {
        uc.at(i, dst) = gj[i] * inv;
        vc.at(i, dst) = vj[i];
    }
}

template <typename T>
static void jacobi_global(rc_context *c, Mat<T> g, Mat<T> v, Mat<T> uc, T *s, Mat<T> vc) {
    const int n = (int)g.rows, N = (n + 1) & ~1;
    ArenaMark mark(c);
    int *state = c->alloc<int>(4);
    T *sig = c->alloc<T>((size_t)n);
    int *order = c->alloc<int>((size_t)n);
    fill_words(c, state, 4 * sizeof(int), 0u);
    fill_identity(c, v);
    // outside a graph capture the convergence flag is read back after every sweep; inside one a fixed number
    // of sweeps is recorded (converged sweeps return immediately)
    const int max_sweeps = c->capturing ? 16 : 60;
    const unsigned grid = (unsigned)((N / 2 + 3) / 4);
    for (int sweep = 0; sweep < max_sweeps; ++sweep) {
        for (int r = 0; r < N - 1; ++r) hipLaunchKernelGGL(k_jacobi_round<T>, dim3(grid), dim3(256), 0, c->stream, g, v, r, state);
        hipLaunchKernelGGL(k_jacobi_sweep_end, dim3(1), dim3(64), 0, c->stream, state);
        if (!c->capturing) {
            int h[4] = {0, 0, 0, 0};
            RC_HIP(hipMemcpyAsync(h, state, sizeof(h), hipMemcpyDeviceToHost, c->stream));
            RC_HIP(hipStreamSynchronize(c->stream));
            if (h[1]) break;
        }
    }
    hipLaunchKernelGGL(k_jacobi_check, dim3(1), dim3(64), 0, c->stream, state, c->health_word());
    hipLaunchKernelGGL(k_jacobi_norms<T>, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, c->stream, g, sig);
    hipLaunchKernelGGL(k_jacobi_rank<T>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, n, sig, order, s);
    hipLaunchKernelGGL(k_jacobi_emit<T>, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, c->stream, g, v, sig, order, uc, vc);
}

template <typename T, int NE, bool FULL>
static void launch_lds_impl(rc_context *c, Mat<T> g, Mat<T> uc, T *s, Mat<T> vc, size_t lds, int ld) {
    const int n = (int)g.rows, N = (n + 1) & ~1;
    ArenaMark mark(c);
    Rot<T> *log = c->alloc<Rot<T>>((size_t)kMaxSweeps * (N - 1) * (N / 2));
    int *sweeps = c->alloc<int>(1);
    int *order = c->alloc<int>((size_t)n);
    auto kern = k_jacobi_lds<T, NE, FULL>;
    static bool attr_set[64] = {};
    if (!attr_set[c->device & 63]) {
        RC_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 2048));
        attr_set[c->device & 63] = true;
    }
    // one 16-lane group per pair, rounded up to whole waves
    const int threads = std::min(1024, std::max(64, (((N / 2) * kLPP + 63) / 64) * 64));
    // fused right vectors: a second workgroup applies the rotations to V as they are published (no replay kernel
    // after the fact); needs one pair slot per group (n <= 128, which also keeps every sorted position + 1 below 255)
    const bool fused = (N / 2) * kLPP <= threads;
    if (fused) {
        unsigned *vsync = c->alloc<unsigned>((size_t)n + 1);
        unsigned long long *chk = c->alloc<unsigned long long>((size_t)kMaxSweeps * (N - 1) * (N / 2));
        // The tagged words are cleared before every launch: a word counts as "published" when its upper 24 bits equal the launch's
        // epoch, and workspace memory that is new to the context (first call, arena growth) holds whatever its last owner left --
        // on a context's first launch (epoch 0 until round 2) any small integer there passed for a sweep count or a sorted
        // position, and the consumer wrote V's columns to the wrong places without noticing (seen as one wrong `vt` among 16
        // contexts' first calls).  The epoch itself now starts at a per-context pseudo-random value (rc_context::epoch_word).
        hipLaunchKernelGGL(k_clear_words, dim3(1), dim3(256), 0, c->stream, vsync, n + 1);
        hipLaunchKernelGGL(kern, dim3(2), dim3(threads), lds, c->stream, g, log, sweeps, uc, s, order, kMaxSweeps, 1, vsync, chk, c->epoch_word(), vc, c->health_word(), ld);
    } else {
        hipLaunchKernelGGL(kern, dim3(1), dim3(threads), lds, c->stream, g, log, sweeps, uc, s, order, kMaxSweeps, 0, (unsigned *)nullptr, (unsigned long long *)nullptr,
                           (unsigned *)nullptr, vc, c->health_word(), ld);
        hipLaunchKernelGGL(k_jacobi_replay_v<T>, dim3((unsigned)((n + 3) / 4)), dim3(256), 4 * (size_t)(n + 1) * sizeof(T), c->stream, n, log, sweeps, order, vc);
    }
    if (c->prof_on && !c->capturing) {  // diagnostic: number of sweeps, reported through the profile table
        int h = 0;
        (void)hipMemcpyAsync(&h, sweeps, sizeof(int), hipMemcpyDeviceToHost, c->stream);  // on the context's own stream
        (void)hipStreamSynchronize(c->stream);
        char nm[64];
        snprintf(nm, sizeof(nm), "info:jacobi_sweeps n=%d", n);
        auto &a = c->prof_acc[nm];
        a.ms += h;
        a.calls += 1;
    }
}

template <typename T, int NE>
static void launch_lds(rc_context *c, Mat<T> g, Mat<T> uc, T *s, Mat<T> vc, size_t lds, int ld) {
    // the bound-free instance: every lane row and every pair slot is real (n = 32, 64, 128); 192 columns would need 1536 threads
    if constexpr (NE <= 8) {
        if (g.rows == kLPP * NE) return launch_lds_impl<T, NE, true>(c, g, uc, s, vc, lds, ld);
    }
    launch_lds_impl<T, NE, false>(c, g, uc, s, vc, lds, ld);
}

// ?gesdd returns an orthonormal U also for a rank-deficient matrix; the one-sided Jacobi iteration leaves a ZERO left vector for
// every zero singular value.  This pass completes them (LAPACK's convention up to the choice of the basis of the null space, which
// no caller can observe through U S V^T): for each zero column, the unit vector with the largest component outside the span of the
// columns before it, orthogonalised twice against them (classical Gram-Schmidt with one re-orthogonalisation) and normalised.
// One workgroup; returns at once when the smallest singular value is positive (the values are sorted), which is every call of
// the hot path.  uc: n x n column-major.
template <typename T>
__global__ __launch_bounds__(1024) void k_complete_left_basis(Mat<T> uc, const T *s) {
    extern __shared__ __attribute__((aligned(16))) char cb_raw[];
    T *v = reinterpret_cast<T *>(cb_raw);          // n
    T *d = v + uc.rows;                            // n: projections
    __shared__ T red_v[16];
    __shared__ int red_i[16];
    __shared__ int sh_p;
    __shared__ T sh_nrm;
    const int n = (int)uc.rows, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (!(s[n - 1] == (T)0)) return;
    int z = 0;  // number of positive singular values (sorted descending): columns z .. n-1 are the zero ones
    for (int j = 0; j < n; ++j) z += s[j] > (T)0 ? 1 : 0;
    for (int j = z; j < n; ++j) {
        // residual of every unit vector: 1 - sum_c U(p, c)^2 over the columns before j
        T best = (T)-1;
        int bp = 0;
        for (int p = tid; p < n; p += 1024) {
            T acc = 1;
            for (int c2 = 0; c2 < j; ++c2) { const T x = uc.p[p + (int64_t)c2 * uc.cs]; acc = fma(-x, x, acc); }
            if (acc > best) { best = acc; bp = p; }
        }
        const T mx = wave_max_dpp(best);
        const int cand = wave_min_dpp(best == mx ? bp : 0x7fffffff);
        if (lane == 0) { red_v[wv] = mx; red_i[wv] = cand; }
        __syncthreads();
        if (tid == 0) {
            T b = red_v[0];
            int bi = red_i[0];
            for (int w = 1; w < 16; ++w)
                if (red_v[w] > b || (red_v[w] == b && red_i[w] < bi)) { b = red_v[w]; bi = red_i[w]; }
            sh_p = bi;
        }
        __syncthreads();
        const int p = sh_p;
        for (int i = tid; i < n; i += 1024) v[i] = i == p ? (T)1 : (T)0;
        __syncthreads();
        for (int pass = 0; pass < 2; ++pass) {
            for (int c2 = tid; c2 < j; c2 += 1024) {
                T acc = 0;
                for (int i = 0; i < n; ++i) acc = fma(uc.p[i + (int64_t)c2 * uc.cs], v[i], acc);
                d[c2] = acc;
            }
            __syncthreads();
            for (int i = tid; i < n; i += 1024) {
                T acc = v[i];
                for (int c2 = 0; c2 < j; ++c2) acc = fma(-uc.p[i + (int64_t)c2 * uc.cs], d[c2], acc);
                v[i] = acc;
            }
            __syncthreads();
        }
        T part = 0;
        for (int i = tid; i < n; i += 1024) part = fma(v[i], v[i], part);
        part = wave_sum_dpp(part);
        if (lane == 0) red_v[wv] = part;
        __syncthreads();
        if (tid == 0) {
            T t = 0;
            for (int w = 0; w < 16; ++w) t += red_v[w];
            sh_nrm = sqrt(t);
        }
        __syncthreads();
        const T inv = (T)1 / sh_nrm;
        for (int i = tid; i < n; i += 1024) uc.p[i + (int64_t)j * uc.cs] = v[i] * inv;
        __threadfence();
        __syncthreads();
    }
}

template <typename T>
void complete_left_basis(rc_context *c, Mat<T> uc, const T *s) {
    if (uc.rows == 0 || uc.rows != uc.cols || uc.rs != 1) return;
    const size_t lds = 2 * (size_t)uc.rows * sizeof(T);
    if (lds > 64 * 1024) return;  // (cores beyond 4096 x 4096 f64 keep the zero vectors)
    hipLaunchKernelGGL(k_complete_left_basis<T>, dim3(1), dim3(1024), lds, c->stream, uc, s);
}
template void complete_left_basis<double>(rc_context *, Mat<double>, const double *);
template void complete_left_basis<float>(rc_context *, Mat<float>, const float *);

template <typename T>
void jacobi_svd(rc_context *c, Mat<T> g, Mat<T> vwork, Mat<T> uc, T *s, Mat<T> vc) {
    RC_REQUIRE(g.rows == g.cols && g.rs == 1 && vwork.rs == 1, RC_LAYOUT_ERROR, "jacobi_svd: square column-major core required");
    const int n = (int)g.rows;
    if (n == 0) return;
    ProfScope ps(c, "op:jacobi_svd n=%lld", (long long)g.rows);
    // Column pitch in LDS.  A 32-lane half of a wave holds the groups of two neighbouring pair slots, whose columns are
    // neighbours too (p, p + 1 and q, q - 1): with a pitch of 16 elements modulo 32 the two 16-lane groups read opposite
    // halves of the bank row (ds_read_b64: 64 banks, f32 ds_read_b32: 32 banks) -- conflict-free, where the odd pitch n | 1
    // made every such read two-way conflicted.  The padded pitch is used whenever it fits the CU's LDS.
    const size_t lds_cap = 160 * 1024 - 2048 - 64;
    auto lds_bytes = [&](int pitch) { return ((size_t)pitch * n + n) * sizeof(T) + (size_t)n * sizeof(int) + 64; };
    int ld = ((n + 15) / 32) * 32 + 16;
    if (lds_bytes(ld) > lds_cap) ld = n | 1;
    const size_t lds = lds_bytes(ld);
    if (lds > lds_cap || n > 192) jacobi_global<T>(c, g, vwork, uc, s, vc);
    else if (n <= 32) launch_lds<T, 2>(c, g, uc, s, vc, lds, ld);
    else if (n <= 64) launch_lds<T, 4>(c, g, uc, s, vc, lds, ld);
    else if (n <= 128) launch_lds<T, 8>(c, g, uc, s, vc, lds, ld);
    else launch_lds<T, 12>(c, g, uc, s, vc, lds, ld);  // f32 up to n = 192 (the LDS bound is ~200)
}

template void jacobi_svd<double>(rc_context *, Mat<double>, Mat<double>, Mat<double>, double *, Mat<double>);
template void jacobi_svd<float>(rc_context *, Mat<float>, Mat<float>, Mat<float>, float *, Mat<float>);

}  // namespace rc
