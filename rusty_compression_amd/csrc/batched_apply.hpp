// The building blocks of the batched apply (kernels_batched_apply.hip) and of the block-sparse operator built on it
// (kernels_block_operator.hip): element arithmetic for real and interleaved-complex data, the strided operand views, the tile load
// into LDS and the product Out = M[:, :red] In with M in global memory and In in LDS.  The mapping and the summation orders are
// described at the head of kernels_batched_apply.hip; both kernels include this file so that an entry of the operator and a block of
// the apply are summed by the same code.
#pragma once
#include <type_traits>

#include "rc_batched_launch.hpp"
#include "rc_common.hpp"
#include "rc_cplx.hpp"
#include "rc_device.hpp"

namespace rc {

namespace {

constexpr int BA_THREADS = BATCHED_THREADS;
constexpr int BA_WAVES = BA_THREADS / 64;

// element arithmetic shared by the real and the interleaved-complex instances
template <typename E>
struct El {
    using real = E;
    static __device__ __forceinline__ E zero() { return (E)0; }
    static __device__ __forceinline__ E fma(E a, E b, E acc) { return ::fma(a, b, acc); }
    static __device__ __forceinline__ E add(E a, E b) { return a + b; }
    static __device__ __forceinline__ E scale(E s, E v) { return s * v; }
    static __device__ __forceinline__ E shfl_xor(E v, int off) { return __shfl_xor(v, off, 64); }
    static __device__ __forceinline__ E conj(E v) { return v; }
};
template <typename R>
struct El<cplx<R>> {
    using real = R;
    using E = cplx<R>;
    static __device__ __forceinline__ E zero() { return {(R)0, (R)0}; }
    static __device__ __forceinline__ E fma(E a, E b, E acc) {
        acc.re = ::fma(a.re, b.re, acc.re);
        acc.re = ::fma(-a.im, b.im, acc.re);
        acc.im = ::fma(a.re, b.im, acc.im);
        acc.im = ::fma(a.im, b.re, acc.im);
        return acc;
    }
    static __device__ __forceinline__ E add(E a, E b) { return {a.re + b.re, a.im + b.im}; }
    static __device__ __forceinline__ E scale(R s, E v) { return {s * v.re, s * v.im}; }
    static __device__ __forceinline__ E shfl_xor(E v, int off) { return {__shfl_xor(v.re, off, 64), __shfl_xor(v.im, off, 64)}; }
    static __device__ __forceinline__ E conj(E v) { return {v.re, -v.im}; }
};

// a stored factor element widened to the compute type E as it is loaded (rc_*_mixed_*: f32 factors under f64 arithmetic, c32 under c64).
// float -> double is exact and a complex element widens componentwise, so everything downstream sees the bits of a promoted copy; S = E is
// the identity and compiles to nothing
template <typename E, typename S>
__device__ __forceinline__ E ba_widen(S v) {
    if constexpr (std::is_same<E, S>::value) return v;
    else if constexpr (sizeof(E) == sizeof(typename El<E>::real)) return (E)v;
    else return {(typename El<E>::real)v.re, (typename El<E>::real)v.im};
}

// Pins a stored element in its registers at this point of the program (an empty instruction that takes and returns it).  The mixed
// instances load their BA_U (or four) elements under a guard each, pin them all, and widen afterwards: without the pin the compiler sinks
// the conversion into the guarded branch beside its load, where it needs the value at once, so that every load is followed by
// s_waitcnt vmcnt(0) and the loads run one after the other instead of together.  Changes no value.
template <typename S>
__device__ __forceinline__ void ba_pin(S &v) {
    if constexpr (sizeof(S) == sizeof(float)) asm volatile("" : "+v"(v));
    else asm volatile("" : "+v"(v.re), "+v"(v.im));
}

// columns of a tile per scalar type, 16 for real and 8 for complex data: the staged b tile (n x NB) and two intermediates (k x NB)
// fit the LDS cap at n = 512, k = 128 in c64 (8 x (513 + 2 x 129) x 16 B = 96 KiB), and the NB accumulators, the NB values of In and the
// loads in flight of a thread stay in registers (f32 at 32 and c32 at 16 columns took all 256 VGPRs: one wave per SIMD)
template <typename E>
constexpr int ba_nb() { return sizeof(E) == sizeof(typename El<E>::real) ? 16 : 8; }

// strided view of one operand with its batch stride (all in elements of E)
template <typename E>
struct BaView {
    E *p;
    int64_t rs, cs, bs;
};

// S: the type the factors are stored in (E, or the narrower type of the mixed calls); b, y, s and all arithmetic are E
template <typename E, typename S = E>
struct BaArgs {
    BaView<const S> left, mid, right;
    BaView<const E> b;
    BaView<E> y;
    const typename El<E>::real *s;
    int64_t s_stride;
    const int64_t *ranks;
    int count, m, n, k, ncols;  // ncols: nrhs, or n when reconstructing (b.p == nullptr)
};

// dynamic LDS: [Bs: NBT x (n|1), with b only] W0: NBT x (k|1) [W1: NBT x (k|1), with mid only]
template <typename E>
size_t ba_lds_bytes(int n, int k, int nbt, bool has_b, bool has_mid) {
    return ((has_b ? (size_t)nbt * (size_t)(n | 1) : 0) + (size_t)(has_mid ? 2 : 1) * nbt * (size_t)(k | 1)) * sizeof(E);
}

// sum of acc[] over the G lanes of a group (OFF = G / 2 on entry, CNT = the columns a lane still holds).  While a lane holds more
// than one column, a step keeps the lower half of them in the lanes whose bit OFF is clear and the upper half in the others, and
// adds the partner's partial sums of the kept half; a single column is summed by the plain butterfly.  Each sum is a + b of the two
// partners' values, the same bits on both sides.
template <int CNT, int OFF, typename E, int NBT>
__device__ __forceinline__ void ba_reduce(E (&acc)[NBT], int l) {
    if constexpr (OFF >= 1) {
        if constexpr (CNT > 1) {
            constexpr int H = CNT / 2;
            const bool up = (l & OFF) != 0;
#pragma unroll
            for (int i = 0; i < H; ++i) {
                const E send = up ? acc[i] : acc[i + H];
                const E keep = up ? acc[i + H] : acc[i];
                acc[i] = El<E>::add(keep, El<E>::shfl_xor(send, OFF));
            }
            ba_reduce<H, OFF / 2>(acc, l);
        } else {
            acc[0] = El<E>::add(acc[0], El<E>::shfl_xor(acc[0], OFF));
            ba_reduce<1, OFF / 2>(acc, l);
        }
    }
}

// after ba_reduce<NBT, G / 2>: lane l of the group holds the finished columns (l / SH) * CNTF + i, i < CNTF, where CNTF = NBT / G
// columns are left per lane when G < NBT, else one column shared by SH = G / NBT lanes (the first of them stores it)
template <int G, typename E, int NBT, typename Store>
__device__ __forceinline__ void ba_reduce_store(E (&acc)[NBT], int l, int row, bool rok, Store store) {
    ba_reduce<NBT, G / 2>(acc, l);
    constexpr int CNTF = G >= NBT ? 1 : NBT / G, SH = G >= NBT ? G / NBT : 1;
    if (rok && (l % SH) == 0) {
#pragma unroll
        for (int i = 0; i < CNTF; ++i) store(row, (l / SH) * CNTF + i, acc[i]);
    }
}

// store(row, c, sum_{j < red} M[row * rs + j * cs] * In[c * ldin + j]) for row < rows, c < NBT: M in global memory, read once and
// only at j < red; In in LDS, NBT columns of at least red elements, ldin apart.  CJ: every element of M is conjugated as it is loaded (the
// block operator's conj flag; the exact negation of the imaginary part, so the sums are those of the call on a conjugated copy of M).
// S: the type M is stored in; an element is widened to E as it is loaded (before conj); a narrower S also pins its loaded values before widening them (ba_pin), which
// changes when the loads are waited for and no value
template <typename E, int NBT, bool CJ = false, typename S = E, typename Store>
__device__ __forceinline__ void ba_product(const S *__restrict__ M, int64_t rs, int64_t cs, int rows, int red, const E *In, int ldin, Store store, int tid) {
    const int lane = tid & 63, wv = tid >> 6;
    constexpr bool kSame = std::is_same<E, S>::value;
    auto ld = [](S sv) {
        const E v = ba_widen<E>(sv);
        if constexpr (CJ) return El<E>::conj(v);
        else return v;
    };
    if (rs <= cs) {  // rows are the fast index: one thread per row, j ascending
        for (int row = tid; row < rows; row += BA_THREADS) {
            const S *mr = M + (int64_t)row * rs;
            E acc[NBT];
#pragma unroll
            for (int c = 0; c < NBT; ++c) acc[c] = El<E>::zero();
            for (int j = 0; j < red; ++j) {
                const E mv = ld(mr[(int64_t)j * cs]);
#pragma unroll
                for (int c = 0; c < NBT; ++c) acc[c] = El<E>::fma(mv, In[c * ldin + j], acc[c]);
            }
#pragma unroll
            for (int c = 0; c < NBT; ++c) store(row, c, acc[c]);
        }
        return;
    }
    // red is the fast index: G lanes per row (wave-uniform: red is)
    int lg = 0;
    while (lg < 6 && (1 << lg) < red) ++lg;
    const int G = 1 << lg, rpw = 64 >> lg, g = lane >> lg, l = lane & (G - 1);
    auto finish = [&](E(&acc)[NBT], int row, bool rok) {
        switch (lg) {
            case 0: ba_reduce_store<1>(acc, l, row, rok, store); break;
            case 1: ba_reduce_store<2>(acc, l, row, rok, store); break;
            case 2: ba_reduce_store<4>(acc, l, row, rok, store); break;
            case 3: ba_reduce_store<8>(acc, l, row, rok, store); break;
            case 4: ba_reduce_store<16>(acc, l, row, rok, store); break;
            case 5: ba_reduce_store<32>(acc, l, row, rok, store); break;
            default: ba_reduce_store<64>(acc, l, row, rok, store); break;
        }
    };
    // lanes past red or past the last row load nothing and multiply In[c][0] by zero
    if (red <= 64) {  // one j per lane: this lane's In values stay in registers, the loads of BA_U row groups are in flight together
        constexpr int BA_U = 4;  // also for a narrower S (8 against 4: DESIGN.md 7n)
        const bool jok = l < red;
        E in[NBT];
#pragma unroll
        for (int c = 0; c < NBT; ++c) in[c] = In[c * ldin + (jok ? l : 0)];
        for (int rowb = wv * rpw; rowb < rows; rowb += BA_WAVES * rpw * BA_U) {
            // a narrower S is held as stored, pinned once all BA_U loads are issued and widened where it is used (ba_pin); S = E keeps the
            // value as loaded; either way an idle lane multiplies by +0
            typename std::conditional<kSame, E, S>::type mv[BA_U];
#pragma unroll
            for (int u = 0; u < BA_U; ++u) {
                const int row = rowb + u * BA_WAVES * rpw + g;
                if constexpr (kSame) mv[u] = (jok && row < rows) ? ld(M[(int64_t)row * rs + (int64_t)l * cs]) : El<E>::zero();
                else mv[u] = (jok && row < rows) ? M[(int64_t)row * rs + (int64_t)l * cs] : S{};
            }
            if constexpr (!kSame) {
#pragma unroll
                for (int u = 0; u < BA_U; ++u) ba_pin(mv[u]);
            }
#pragma unroll
            for (int u = 0; u < BA_U; ++u) {
                if (rowb + u * BA_WAVES * rpw >= rows) break;  // wave-uniform
                const int row = rowb + u * BA_WAVES * rpw + g;
                E w;
                if constexpr (kSame) w = mv[u];
                else w = (jok && row < rows) ? ld(mv[u]) : El<E>::zero();
                E acc[NBT];
#pragma unroll
                for (int c = 0; c < NBT; ++c) acc[c] = El<E>::fma(w, in[c], El<E>::zero());
                finish(acc, row, row < rows);
            }
        }
        return;
    }
    for (int row0 = wv; row0 < rows; row0 += BA_WAVES) {  // red > 64: G = 64, one row per wave
        const S *mr = M + (int64_t)row0 * rs;
        E acc[NBT];
#pragma unroll
        for (int c = 0; c < NBT; ++c) acc[c] = El<E>::zero();
        if constexpr (kSame) {
#pragma unroll 4
            for (int j0 = 0; j0 < red; j0 += 64) {
                const int j = j0 + l;
                const bool ok = j < red;
                const E mv = ok ? ld(mr[(int64_t)j * cs]) : El<E>::zero();
                const E *ip = In + (ok ? j : 0);
#pragma unroll
                for (int c = 0; c < NBT; ++c) acc[c] = El<E>::fma(mv, ip[c * ldin], acc[c]);
            }
        } else {  // the same terms in the same order, four loads issued and pinned before the first is widened (ba_pin)
            for (int j0 = 0; j0 < red; j0 += 4 * 64) {
                S raw[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int j = j0 + u * 64 + l;
                    raw[u] = j < red ? mr[(int64_t)j * cs] : S{};
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) ba_pin(raw[u]);
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    if (j0 + u * 64 >= red) break;  // wave-uniform
                    const int j = j0 + u * 64 + l;
                    const bool ok = j < red;
                    const E mv = ok ? ld(raw[u]) : El<E>::zero();
                    const E *ip = In + (ok ? j : 0);
#pragma unroll
                    for (int c = 0; c < NBT; ++c) acc[c] = El<E>::fma(mv, ip[c * ldin], acc[c]);
                }
            }
        }
        ba_reduce_store<64>(acc, l, row0, true, store);
    }
}

// T[c * ld + i] = src[i * rs + (c0 + c) * cs] for i < rows, c < nb, zero for nb <= c < NBT; lanes along the fast index of src
// (S: the stored type of src, widened to E)
template <typename E, int NBT, typename S = E>
__device__ __forceinline__ void ba_load_tile(E *T, int ld, const S *__restrict__ src, int64_t rs, int64_t cs, int rows, int c0, int nb, int tid) {
    const int total = rows * NBT;
    if (cs <= rs) {
        for (int idx = tid; idx < total; idx += BA_THREADS) {
            const int c = idx % NBT, i = idx / NBT;
            T[c * ld + i] = c < nb ? ba_widen<E>(src[(int64_t)i * rs + (int64_t)(c0 + c) * cs]) : El<E>::zero();
        }
    } else {
        for (int idx = tid; idx < total; idx += BA_THREADS) {
            const int i = idx % rows, c = idx / rows;
            T[c * ld + i] = c < nb ? ba_widen<E>(src[(int64_t)i * rs + (int64_t)(c0 + c) * cs]) : El<E>::zero();
        }
    }
}

}  // namespace

}  // namespace rc
