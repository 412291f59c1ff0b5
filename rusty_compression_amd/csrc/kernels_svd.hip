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
#include "jacobi_lds.hpp"

namespace rc {

template <typename T> __device__ inline T dpp_row_sum(T v) { return group_sum_dpp<16>(v); }

__global__ void k_clear_words(unsigned *p, int n) {
    for (int i = threadIdx.x; i < n; i += blockDim.x) p[i] = 0u;
}

// The LDS-resident Jacobi as its own launch (body, arguments and protocol invariants J1-J6: jacobi_lds.hpp): one group per
// pair slot, workgroup 1 of a fused launch is the consumer.
template <typename T, int NE, bool FULL>
__global__ __launch_bounds__(1024) void k_jacobi_lds(JacobiLdsArgs<T> ja) {
    jacobi_lds_body<T, NE, FULL>(ja, blockIdx.x == 1);
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
    const T tol = sqrt((T)n) * num<T>::eps();
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
    // of sweeps is recorded (converged sweeps return immediately): the LDS kernel's budget.  With 16 recorded sweeps a
    // numerically rank-deficient 142 x 142 core (X Y^T of rank 35: 22 sweeps) came back unconverged, health bit 4 raised
    const int max_sweeps = c->capturing ? kMaxSweeps : 60;
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
    constexpr auto kern = k_jacobi_lds<T, NE, FULL>;
    raise_lds_limit<kern>(c->device, kLdsCapWide);
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
        const JacobiLdsArgs<T> ja{g, log, sweeps, uc, s, order, kMaxSweeps, 1, vsync, chk, c->epoch_word(), vc, c->health_word(), ld};
        hipLaunchKernelGGL(kern, dim3(2), dim3(threads), lds, c->stream, ja);
    } else {
        const JacobiLdsArgs<T> ja{g, log, sweeps, uc, s, order, kMaxSweeps, 0, nullptr, nullptr, nullptr, vc, c->health_word(), ld};
        hipLaunchKernelGGL(kern, dim3(1), dim3(threads), lds, c->stream, ja);
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
    const size_t lds_cap = kJacobiLdsCap;
    const int ld = jacobi_pitch<T>(n);  // column pitch in LDS
    const size_t lds = jacobi_lds_bytes<T>(n, ld);
    if (lds > lds_cap || n > 192) jacobi_global<T>(c, g, vwork, uc, s, vc);
    else if (n <= 32) launch_lds<T, 2>(c, g, uc, s, vc, lds, ld);
    else if (n <= 64) launch_lds<T, 4>(c, g, uc, s, vc, lds, ld);
    else if (n <= 128) launch_lds<T, 8>(c, g, uc, s, vc, lds, ld);
    else launch_lds<T, 12>(c, g, uc, s, vc, lds, ld);  // f32 up to n = 192 (the LDS bound is ~200)
}

template void jacobi_svd<double>(rc_context *, Mat<double>, Mat<double>, Mat<double>, double *, Mat<double>);
template void jacobi_svd<float>(rc_context *, Mat<float>, Mat<float>, Mat<float>, float *, Mat<float>);

}  // namespace rc
