// LDS-resident one-sided Jacobi of a small square core: the device body, shared by its own launch (kernels_svd.hip,
// k_jacobi_lds) and by the launch that runs it beside the cooperative pivoted QR (kernels_wqcoop.hip, k_wq_jacobi_fused).
#pragma once
#include "rc_common.hpp"
#include "rc_device.hpp"
#include "rc_launch.hpp"

namespace rc {

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
#ifndef RC_AGENT
#define RC_AGENT __HIP_MEMORY_SCOPE_AGENT
#endif
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

// Lanes per column pair: one DPP row.
constexpr int kLPP = 16;
static_assert(kMaxSweeps < 255, "sweep count must fit a tagged word");

// Column pitch of the core in LDS and the dynamic LDS of a launch.  A 32-lane half of a wave holds the groups of two neighbouring
// pair slots, whose columns are neighbours too (p, p + 1 and q, q - 1): with a pitch of 16 elements modulo 32 the two 16-lane groups
// read opposite halves of the bank row (ds_read_b64: 64 banks, f32 ds_read_b32: 32 banks) -- conflict-free, where the odd pitch n | 1
// made every such read two-way conflicted.  The padded pitch is used whenever it fits the CU's LDS (kJacobiLdsCap, rc_launch.hpp).
template <typename T>
inline size_t jacobi_lds_bytes(int n, int pitch) { return ((size_t)pitch * n + n) * sizeof(T) + (size_t)n * sizeof(int) + 64; }
template <typename T>
inline int jacobi_pitch(int n) {
    const int ld = ((n + 15) / 32) * 32 + 16;
    return jacobi_lds_bytes<T>(n, ld) > kJacobiLdsCap ? (n | 1) : ld;
}

//   g      : n x n column-major input (global), destroyed
//   log    : [max_sweeps][N-1][N/2] rotations (c = 1, s = 0 where none)
//   sweeps : number of sweeps performed (device scalar out)
//   uc, s  : left singular vectors / singular values, sorted descending
//   order  : order[j] = sorted position of original column j (for the V replay)
//   fused  : != 0: launched with TWO workgroups; the second one accumulates V from the published records while the first
//            is still rotating (vsync[0] = number of sweeps once known, vsync[1 + j] = order[j] + 1; both zeroed before)
//   ld     : column pitch chosen by the host (jacobi_pitch)
template <typename T>
struct JacobiLdsArgs {
    Mat<T> g;
    Rot<T> *log;
    int *sweeps_out;
    Mat<T> uc;
    T *s;
    int *order_out;
    int max_sweeps, fused;
    unsigned *vsync;
    unsigned long long *chk;
    unsigned *epoch_p;
    Mat<T> vc;
    int *health;
    int ld;
};

// the three dot products of one column pair over this lane's rows (the columns stay in registers for the rotation)
template <typename T, int NE, bool FULL>
__device__ inline void jacobi_pair_dots(const T *gp, const T *gq, int ll, int n, T (&a)[NE], T (&b)[NE], T &app, T &aqq, T &apq) {
    app = 0; aqq = 0; apq = 0;
#pragma unroll
    for (int e = 0; e < NE; ++e) {
        int i = ll + kLPP * e;
        a[e] = (FULL || i < n) ? gp[i] : (T)0;
        b[e] = (FULL || i < n) ? gq[i] : (T)0;
        app = fma(a[e], a[e], app);
        aqq = fma(b[e], b[e], aqq);
        apq = fma(a[e], b[e], apq);
    }
}
// The contraction is spelled out (c a - (s b) and s a + (c b), each with the product in brackets rounded first): left to the
// compiler, which product of a sum is fused depends on the code around it, and the instances would differ in the last bit.
template <typename T, int NE, bool FULL>
__device__ inline void jacobi_pair_rotate(T *gp, T *gq, int ll, int n, const T (&a)[NE], const T (&b)[NE], Rot<T> rot) {
#pragma unroll
    for (int e = 0; e < NE; ++e) {
        int i = ll + kLPP * e;
        if (FULL || i < n) {
            gp[i] = fma(rot.c, a[e], -(rot.s * b[e]));
            gq[i] = fma(rot.s, a[e], rot.c * b[e]);
        }
    }
}
// (the two threshold tests of a pair, jacobi_pair_is_coupled and jacobi_rotation_was_large: rc_device.hpp)

// ---------------------------------------------------------------------------
// LDS-resident one-sided Jacobi.  16 lanes own one column pair and keep NE = n / 16 rows (rounded up) of both columns in
// registers; 1024 threads = 64 groups, one per pair slot of a 128 x 128 core.
// ---------------------------------------------------------------------------
// PROTOCOL INVARIANTS of the fused launch (two workgroups; reviewed against the code in round 3 -- keep list and code in step)
//  J1  One direction only: the producer workgroup publishes, the consumer workgroup reads; the producer never waits for the
//      consumer, so the two need not be co-resident and the producer's result (U, S) never depends on the consumer.
//  J2  Everything that crosses is an 8-byte (records, check words) or 4-byte (vsync) agent-scope relaxed atomic.  A rotation record
//      is valid iff its check word equals hash(c, s) ^ key(epoch): a torn combination of two publications and a complete record of
//      an EARLIER launch at the same workspace address (other epoch, other key) both fail the test, so records need no clearing.
//  J3  epoch is a per-context device counter, started at a pseudo-random 23-bit value, read by both workgroups at their start and
//      incremented by the consumer at its very end; launches of one context are stream ordered, so every launch sees a new epoch.
//  J4  The small hand-over words vsync[0] (number of sweeps) and vsync[1 + j] (sorted position + 1) travel as (epoch << 8) | payload
//      AND are cleared on the same stream in front of every launch (fill_words for k_jacobi_lds; for k_wq_jacobi_fused the gate
//      kernel of its cooperative role, k_coop_gate, clears them with the header words): payload 0 means "not there yet".
//  J5  The consumer learns that sweep s exists from the first record of sweep s validating, and that it does not from
//      vsync[0] <= s; the producer writes exactly one of the two after sweep s - 1.  Index of a record: (sweep, round, pair slot),
//      the same expression on both sides.
//  J6  Every consumer spin is bounded (kSpin); on expiry health bit 8 is raised and V is reported incomplete -- never silently wrong.
//   FULL   : n == 16 * NE and one pair slot per group (1024 threads for a 128 x 128 core): no row / column bounds, no slot loop
//            (the round is bound by the number of instructions the waves issue, and the predicates were a quarter of them)
//   consumer: this workgroup is the second one of a fused launch
template <typename T, int NE, bool FULL>
__device__ inline void jacobi_lds_body(const JacobiLdsArgs<T> &ja, bool consumer) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const Mat<T> g = ja.g;
    Rot<T> *log = ja.log;
    unsigned long long *chk = ja.chk;
    unsigned *vsync = ja.vsync;
    const int fused = ja.fused, max_sweeps = ja.max_sweeps, ld = ja.ld;
    const int n = (int)g.rows;
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
    const unsigned epoch = fused ? __hip_atomic_load(ja.epoch_p, __ATOMIC_RELAXED, RC_AGENT) & 0xffffffu : 0u;
    const unsigned long long key = epoch_key(epoch);
    if (fused && consumer) {
        // ---- consumer: V = product of the rotations, columns in LDS, the producer's pairing ----
        constexpr int kSpin = 1 << 24;
        const Mat<T> vc = ja.vc;
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
                                vp[i] = fma(rot.c, a, -(rot.s * b));  // (the contraction of jacobi_pair_rotate)
                                vq[i] = fma(rot.s, a, rot.c * b);
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
        if (lost && ll == 0) atomicOr(ja.health, 8);  // the producer never showed up within the spin bound: V is incomplete
        __syncthreads();
        if (tid == 0) __hip_atomic_fetch_add(ja.epoch_p, 1u, __ATOMIC_RELAXED, RC_AGENT);  // the next launch uses a new key
        return;
    }
    const T tol = sqrt((T)n) * num<T>::eps();
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
                    T app, aqq, apq;
                    jacobi_pair_dots<T, NE, FULL>(gp, gq, ll, n, a, b, app, aqq, apq);
                    app = group_sum_dpp<kLPP>(app);
                    aqq = group_sum_dpp<kLPP>(aqq);
                    apq = group_sum_dpp<kLPP>(apq);
                    // rotate iff |apq| > tol * sqrt(app * aqq)   (uniform over the 16 lanes)
                    const double apq2 = (double)apq * (double)apq;
                    if (jacobi_pair_is_coupled(app, aqq, apq2, tol2)) {
                        jacobi_rotation(app, aqq, apq, rot.c, rot.s);
                        jacobi_pair_rotate<T, NE, FULL>(gp, gq, ll, n, a, b, rot);
                        // flag 2 = another sweep is needed
                        if (ll == 0 && jacobi_rotation_was_large(app, aqq, apq2, rot.s, tol)) sh_rot = 2;  // plain store: every writer writes 2
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
    if (tid == 0 && !converged && ja.health) atomicOr(ja.health, 16);
    if (tid == 0) {
        *ja.sweeps_out = sweep;
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
        ja.order_out[i] = rank;
        if (fused) tagged_put(vsync + 1 + i, epoch, (unsigned)(rank + 1));
        ja.s[rank] = si;
    }
    __syncthreads();
    for (int j = grp; j < n; j += ngrp) {
        const int dst = order[j];
        const T sj = sig[j];
        const T inv = sj > (T)0 ? (T)1 / sj : (T)0;
        const T *gj = G + j * ld;
        for (int i = ll; i < n; i += kLPP) ja.uc.at(i, dst) = gj[i] * inv;
    }
#undef sh_rot
}

}  // namespace rc
