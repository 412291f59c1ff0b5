// Shared between the GEMM translation units (kernels_gemm.hip: shape dispatch, split-K policy and the general kernels;
// kernels_gemm_pipe.hip: the software-pipelined f64 main loop of the two big products).
#pragma once
#include "rc_common.hpp"
#include "rc_launch.hpp"

namespace rc {

// The 16x16x4 MFMA of each real scalar and its accumulator fragment (v_mfma_f64_16x16x4_f64, v_mfma_f32_16x16x4_f32: exact f32), shared with the
// batched sketch (kernels_batched_id.hip).  A-operand lane l holds A[l&15][l>>4], B-operand lane l holds B[l>>4][l&15]; C/D: col = l&15,
// row = Acc<T>::row(l, reg).
typedef double double4_t __attribute__((ext_vector_type(4)));
typedef float float4_t __attribute__((ext_vector_type(4)));
typedef double double2_t __attribute__((ext_vector_type(2)));
typedef float float2_t __attribute__((ext_vector_type(2)));

template <typename T> struct Acc;
template <> struct Acc<double> {
    typedef double4_t type;
    typedef double2_t vec2;
    static __device__ inline type mfma(double a, double b, type c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }
    static __device__ inline int row(int lane, int reg) { return (lane >> 4) + 4 * reg; }
};
template <> struct Acc<float> {
    typedef float4_t type;
    typedef float2_t vec2;
    static __device__ inline type mfma(float a, float b, type c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
    static __device__ inline int row(int lane, int reg) { return 4 * (lane >> 4) + reg; }
};

// The LDS chunk images of the batched sketch Omega A, shared by its real kernel (kernels_batched_id.hip) and its complex one (kernels_batched_id_c.hip,
// one image of these pitches per component): BSI_ROWS rows of A beside the matching columns of Omega, column panels of BSI_COLS columns.
constexpr int BSI_ROWS = 32;   // rows of A (= columns of Omega) per LDS chunk
constexpr int BSI_COLS = 64;   // columns of Y per panel
constexpr int BSI_PK = BSI_ROWS + 2;                       // pitch of an image with the reduction index fastest
constexpr int BSI_PA = 80;                                 // pitch of A's image with the column index fastest (16 mod 32, >= BSI_COLS)
constexpr int BSI_A_ELEMS = BSI_ROWS * BSI_PA;             // A's chunk image: the larger of the two layouts
static_assert(BSI_A_ELEMS >= BSI_COLS * BSI_PK && BSI_PA >= BSI_COLS, "A chunk image");
__host__ __device__ constexpr int bsi_po(int l) {          // pitch of Omega's image with the row index fastest (16 mod 32, >= 16 TL)
    return (((l + 15) & ~15) & 16) ? ((l + 15) & ~15) : ((l + 15) & ~15) + 16;
}
__host__ __device__ constexpr int bsi_o_elems(int l) {     // Omega's chunk image: the larger of the two layouts (16 TL rows x BSI_ROWS)
    return BSI_ROWS * bsi_po(l) > ((l + 15) & ~15) * BSI_PK ? BSI_ROWS * bsi_po(l) : ((l + 15) & ~15) * BSI_PK;
}

template <typename T>
struct GemmArgs {
    const T *a, *b;
    T *c;
    int64_t M, N, K;
    int64_t sam, sak;  // A(m, k)
    int64_t sbk, sbn;  // B(k, n)
    int64_t scm, scn;  // C(m, n)
    T alpha, beta;
    int64_t kchunk;    // K range per split
    int splits;
    T *partial;        // [splits][M][N] when splits > 1
    int tiles_m, tiles_n;
};

// Software-pipelined f64 kernel (kernels_gemm_pipe.hip).  Launches the GEMM kernel for an ALREADY split problem (tiles_m,
// tiles_n, kchunk, splits, partial filled in by the caller) if an instantiation for this tile shape exists and the operands
// meet its preconditions (16-byte vector staging, K chunks that are multiples of the K tile); returns false otherwise.
bool gemm_f64p_launch(rc_context *c, const GemmArgs<double> &g, int alay, int blay, int bm, int bn, int bk, int wm, int wn, int orient, bool vec2);
// Whether an instantiation of bm x bn tiles takes a product of 16-byte vector operands however its K is split (whole K tiles, 32-bit
// spans over all of K): gemm_chain asks this of the tile gemm would launch before it cuts that tile up.
bool gemm_f64p_accepts(const GemmArgs<double> &g, int bm, int bn, int bk);

}  // namespace rc
