/* rusty_compression_amd.h -- C ABI of the MI355X-native randomized low-rank
 * compression engine (librusty_compression_amd.so).
 *
 * This is the drop-in boundary for the hot path of rusty-compression v0.1.1
 * (reference at /root/reference).  The reference has no FFI of its own: its
 * arithmetic crosses into Fortran LAPACK inside src/pivoted_qr.rs:138-173 and
 * through ndarray-linalg.  A maintainer swapping the hot path to the GPU binds
 * ONE level higher, at the crate's own trait methods, so every entry point
 * below names the reference interface it replaces (file:line).  The reference
 * side binding (Rust `extern "C"` block + trait impls) is in INTEGRATION.md
 * and bindings/rust/.
 *
 * Conventions
 *  - All matrix arguments are DEVICE memory described by `rc_matrix` (an
 *    ndarray-style strided view: element (i, j) lives at
 *    data[i*row_stride + j*col_stride], strides in elements).  Any layout is
 *    accepted (C order, Fortran order, transposed views); inputs are never
 *    modified (reference: every trait method borrows views and returns owned
 *    arrays).  Outputs are caller-allocated.  "Any layout" holds for outputs as
 *    it does for inputs: a padded view (odd pitch included), a view that starts
 *    at any element offset of its allocation (no alignment beyond the scalar's
 *    own), and a view with both strides non-unit are written like a fresh C-order
 *    array, and no element outside the view is ever written
 *    (tests/test_gpu_output_views.py; overlapping views and zero or negative
 *    strides on outputs are not supported).
 *  - `_f64` / `_f32` select the scalar type (reference macros instantiate
 *    f32/f64/c32/c64; complex is out of scope).
 *  - Index vectors are int64, 0-based, in device memory (reference: usize,
 *    src/qr.rs:36-39).
 *  - Calls are asynchronous on the context's HIP stream unless they return a
 *    host scalar (documented per function); rc_synchronize() waits.
 *  - Every function returns rc_status; rc_last_error_message() explains it.
 *    Status values mirror RustyCompressionError (src/types.rs:11-21).
 *  - One context per host thread per GPU; contexts share nothing.
 */
#ifndef RUSTY_COMPRESSION_AMD_H
#define RUSTY_COMPRESSION_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RC_ABI_VERSION 1

typedef int32_t rc_status;
enum {
    RC_OK = 0,
    RC_LINALG_ERROR = 1,      /* RustyCompressionError::LinalgError      src/types.rs:13-14 */
    RC_COMPRESSION_ERROR = 2, /* RustyCompressionError::CompressionError src/types.rs:15-16 */
    RC_LAYOUT_ERROR = 3,      /* RustyCompressionError::LayoutError      src/types.rs:17-18 */
    RC_PIVOTED_QR_ERROR = 4,  /* RustyCompressionError::PivotedQRError   src/types.rs:19-20 */
    RC_INVALID_ARGUMENT = 5,  /* the reference panics (assert!) on these: src/qr.rs:99, src/permutation.rs:96-99 */
    RC_RUNTIME_ERROR = 6      /* HIP runtime failure (no reference counterpart) */
};

/* ndarray-style strided device view; strides in ELEMENTS. */
typedef struct rc_matrix {
    void *data;
    int64_t rows;
    int64_t cols;
    int64_t row_stride;
    int64_t col_stride;
} rc_matrix;

typedef struct rc_context rc_context;

/* CompressionType (src/lib.rs:82-87) */
enum { RC_COMPRESS_ADAPTIVE = 0, RC_COMPRESS_RANK = 1 };
/* MatrixPermutationMode (src/permutation.rs:7-16) */
enum { RC_PERM_COL = 0, RC_PERM_ROW = 1, RC_PERM_COLINV = 2, RC_PERM_ROWINV = 3 };
/* VectorPermutationMode (src/permutation.rs:19-24) */
enum { RC_VPERM_INV = 0, RC_VPERM_NOINV = 1 };

/* ---------------------------------------------------------------- context -- */
int32_t rc_abi_version(void);
/* stream: a hipStream_t (may be NULL = the device's default stream). */
rc_status rc_create(rc_context **ctx, int32_t device, void *hip_stream);
rc_status rc_destroy(rc_context *ctx);
rc_status rc_set_stream(rc_context *ctx, void *hip_stream);
/* Stream helpers for hosts without HIP bindings: a non-blocking hipStream_t on `device`, to be passed to
 * rc_create / rc_set_stream (one context + stream per independent compression in flight). */
rc_status rc_stream_create(int32_t device, void **hip_stream);
rc_status rc_stream_destroy(int32_t device, void *hip_stream);
rc_status rc_synchronize(rc_context *ctx);
/* Wait for n contexts at once: a completion event is recorded on EVERY context's stream before the first wait.  A host
 * that keeps dozens of independent compressions in flight (one context + stream each) should use this instead of
 * rc_synchronize context by context: stream-by-stream waits returned after max(259 ms, work) on ROCm 7.2 when more
 * than ~28 streams held work ("Completion waits").  No reference counterpart (the reference is synchronous). */
rc_status rc_synchronize_all(rc_context *const *ctxs, int32_t n);
/* Pre-size the internal workspace arena (bytes); optional, it grows on demand. */
rc_status rc_reserve_workspace(rc_context *ctx, size_t bytes);
const char *rc_last_error_message(const rc_context *ctx);

/* Plain device-memory helpers so a host without HIP bindings (the Rust crate)
 * can stage ndarray data: upload -> call -> download. */
rc_status rc_device_malloc(rc_context *ctx, size_t bytes, void **ptr);
rc_status rc_device_free(rc_context *ctx, void *ptr);
rc_status rc_memcpy_h2d(rc_context *ctx, void *dst_dev, const void *src_host, size_t bytes);
rc_status rc_memcpy_d2h(rc_context *ctx, void *dst_host, const void *src_dev, size_t bytes); /* synchronous */

/* hipGraph capture: everything issued on the context's stream between begin and
 * end becomes one replayable graph (launch-bound chains such as the ~130
 * dependent pivot steps of a pivoted QR replay without host launch overhead).
 * Only calls without host synchronisation may be captured, and the context must
 * have run the same call once eagerly before (workspace sizing).  A graph has workspace
 * addresses baked in: while any graph of a context is alive, a workspace the context
 * outgrows is kept allocated instead of freed, so eager calls of any size may be mixed with
 * replays (stream order keeps them apart).  No reference counterpart: the reference is
 * synchronous host code. */
rc_status rc_graph_begin_capture(rc_context *ctx);
rc_status rc_graph_end_capture(rc_context *ctx, void **graph_exec);
rc_status rc_graph_launch(rc_context *ctx, void *graph_exec);
rc_status rc_graph_destroy(rc_context *ctx, void *graph_exec);

/* Options.  RC_OPT_TALL_SKINNY_FAST_PATH (default 1): tall-skinny pivoted QR / QR inside
 * the SVD run as CholeskyQR2 + an LDS-resident pivoted QR of the small factor + a sign fix
 * that restores LAPACK's Householder sign convention; the path certifies itself
 * (positive Cholesky pivots, ||Q1^T Q1 - I|| small) and the call falls back to the plain
 * Householder chain (exact ?geqp3/?orgqr operation order) when the certificate fails.
 * 0 forces the Householder chain.  While a hipGraph is being captured no fallback is
 * possible: failures are OR-ed into a health word instead, which rc_get_health returns
 * and clears (0 = every captured fast path certified itself). */
/* RC_OPT_WIDE_LAZY_QRCP (default 1): pivoted QR of short-wide matrices (m <= 256 << n) keeps the
 * m x m orthogonal factor explicitly and never rewrites the trailing matrix (same ?laqp2
 * pivoting semantics); 0 selects the eager Householder chain. */
/* RC_OPT_WIDE_COOP_QRCP (default 1): the same short-wide pivoted QR as ONE cooperative launch that
 * keeps the whole matrix in registers (one grid barrier per Householder step instead of two kernel
 * launches); certifies itself like the tall-skinny path (bit 4 of the health word = its workgroups
 * could not all become resident in time) and falls back to the lazy scheme; 0 disables it. */
/* Reproducibility.  Every entry point is deterministic: the same call with the same options on the same context state gives the
 * same bits (no atomics on results, fixed split-K reduction order).  Three settings choose between implementations of the same
 * factorization, and bits are promised PER SETTING, not across them: (i) min(RC_OPT_CONCURRENCY_HINT, RC_OPT_KERNEL_SLOTS) decides
 * how far wide products split K (a lone launch, a few kernels in flight, many): results differ by summation order; (ii) a call recorded into a
 * hipGraph cannot read scalars back, so general-shape pivoted QRs run the per-step chain there and the blocked panels eagerly:
 * same pivots on the data-determined prefix, factors equal to rounding (tests: test_captured_pivoted_qr_of_a_blocked_eligible_shape…).
 * The cfg3 pipeline (rc_rsvd_id_*) takes the same path eagerly and captured: its replays equal the eager result bit for bit.
 * (iii) RC_OPT_FUSED_CONSUMERS selects the order and the launches of the two consumers of B in rc_rsvd_id_*; bits are promised per
 * setting like the others (today the two settings agree bit for bit -- tests/test_gpu_fused_consumers.py -- because neither
 * factorization changes its arithmetic, but only the per-setting promise is API).
 * Across RELEASES bits are not promised.  Since the small products of the tall-skinny QR (R2 R1, R2^-1 Q2, Q1[:k, :] W, R2^-1 Vc) are
 * formed inside the kernels next to them, each entry in one ascending order instead of a two-slab GEMM, results move at rounding
 * level wherever the second CholeskyQR pass does not reduce to the identity (first-pass defect above 2.5e-14 in f64, 1e-6 in f32);
 * where it does (well-conditioned sketches, the cfg3 workload) they are the bits of the GEMM order.
 * Environment switches that select between implementations (measurement aids, read once per process) change rounding the same
 * way and are NOT part of the promise: RC_TSQR_FOLD (order of the small factors of the tall-skinny QR), RC_QRCP_CAND_MB (which
 * columns of a blocked panel are updated reflector by reflector and which through the block update: last bits of R12 / Z),
 * RC_GEMM_LANES_TARGET, RC_GEMM_SLOTS_TARGET, RC_GEMM_SMALL_TARGET (split-K counts).
 * Schedules that only change WHEN or WHERE the same arithmetic is issued -- RC_WQ_STAGES, RC_QRCP_OPTIMISTIC, RC_BATCH_OPTIMISTIC,
 * RC_QRCP_KEEP_DIRECT, RC_ID_FUSED -- give identical bits (tested for the staged k_wq_coop and the optimistic blocked QRCP).
 * RC_GEMM_SPREAD changes scheduling only: which workgroup computes an entry of the Gram and shallow products of the tall-skinny
 * chain, never its K slabs or the order of its sum (tests/test_gpu_spread_switch.py compares the two settings bit for bit). */
/* RC_OPT_POWER_ITERATION_FIXED (default 0): rc_sample_range_power_iteration_* performs it_count power steps
 * (Y <- A orth(A^H orth(Y))) as the reference documents; 0 reproduces the reference's behaviour, where a shadowed
 * loop variable leaves exactly one step (src/random_sampling.rs:145-153). */
/* RC_OPT_FORK_BRANCHES (default 0): 1 makes rc_rsvd_id_* run its two independent consumers of B = Q^H A (the SVD and
 * the pivoted-QR / ID branch) side by side on a second stream owned by the context (fork / join with events; captured
 * into the same hipGraph).  Latency of one compression 6.8 -> 5.6 ms; with dozens of such graphs in flight the
 * throughput measured lower (680 vs 913 compressions/s), hence opt-in. */
/* RC_OPT_BLOCKED_QRCP (default 1): pivoted QR of general shapes (neither tall-skinny nor short-wide) runs ?geqp3 the way
 * LAPACK does -- ?laqps panels of 32 steps with the delayed F-matrix update and one MFMA GEMM block update per panel -- with
 * the panel restricted to the candidate columns whose norm can still be the maximum (kernels_qrblk.hip): identical pivoting
 * rule and down-dating formulas, about three passes over the trailing matrix per panel instead of two per step.  Reads one
 * small struct back per panel, so it is not used while a hipGraph is being captured.  0 selects the per-step chain. */
/* RC_OPT_CONCURRENCY_HINT (default 1): how many independent compressions the host keeps in flight on this device (one
 * context + stream each).  What the library sizes its launches for is min(hint, RC_OPT_KERNEL_SLOTS), the compressions
 * whose kernels can really run side by side.  With 1 a wide GEMM (>= 8 output tiles) splits its reduction dimension until
 * every CU has a workgroup (256); with 2..7 a product with >= 32 output tiles splits to 128 workgroups, half the chip, so
 * that a second product can run beside it; with >= 8 the other streams fill the chip and such a product is not split (no
 * partial slabs, no reduction kernel).  Results are deterministic for a given min(hint, slots); different values differ
 * by summation order only. */
/* RC_OPT_KERNEL_SLOTS (default 4): how many kernels of this process the device runs at once.  Packets of one hardware
 * queue run in order, so this is the number of hardware queues the process has; 4 is the HIP runtime's default.  The
 * library does not read the runtime's configuration: a host that runs its process with more queues says so here. */
/* RC_OPT_COOP_PANEL (default 1): the steps of a blocked-QRCP panel run as ONE cooperative launch with the candidate columns
 * resident in registers (one grid barrier per step instead of two kernel boundaries; the candidates are read and written once
 * per panel) whenever the active rows fit (m - j0 <= 4096 in f32, 3072 in f64) and the candidates fit its 512 waves; a launch
 * that cannot run (too many tied candidates, workgroups not co-resident in time) leaves the panel untouched and the step
 * kernels take it.  Same pivot rule; the candidates' norms are down-dated with ?laqp2's formula (their columns are kept up to
 * date, so a norm that loses its accuracy is recomputed on the spot instead of ending the panel).  0 = step kernels only. */
/* RC_OPT_FUSED_CONSUMERS (default 1): rc_rsvd_id_* with both consumers wanted runs the pivoted QR of B = Q^H A (k x n) and the
 * Jacobi SVD of the k x k core of B in ONE launch: the tall QR of B^T first, then one kernel whose first workgroups are the
 * cooperative pivoted QR (one stage over all steps) and whose last two are the Jacobi's producer and consumer, then the tails of
 * both branches: R, the orthogonal factor Q_b of B and the Z of the column ID come out of ONE further launch (they read only the
 * factored matrix, its pivots and tau, and not each other), and the Jacobi writes the left vectors of the core where U = Q U_b
 * reads them.  The two factorizations are independent, and side by side they hold one of the process's kernel slots for the
 * longer of the two instead of two slots for the sum.  Taken for f64, k = 128, shapes the cooperative QR and the tall-skinny path
 * support, RC_OPT_FORK_BRANCHES off and min(RC_OPT_CONCURRENCY_HINT, RC_OPT_KERNEL_SLOTS) < 8; every other call, and 0, run the
 * pivoted-QR / ID branch first and the SVD branch after it.  Certificates keep their meaning (health bits 1, 2, 4, 8, 16). */
enum { RC_OPT_TALL_SKINNY_FAST_PATH = 1, RC_OPT_WIDE_LAZY_QRCP = 2, RC_OPT_WIDE_COOP_QRCP = 3, RC_OPT_POWER_ITERATION_FIXED = 4, RC_OPT_FORK_BRANCHES = 5,
       RC_OPT_BLOCKED_QRCP = 6, RC_OPT_CONCURRENCY_HINT = 7, RC_OPT_COOP_PANEL = 8, RC_OPT_KERNEL_SLOTS = 9, RC_OPT_FUSED_CONSUMERS = 10 };
rc_status rc_set_option(rc_context *ctx, int32_t option, int64_t value);
/* Health word (read and cleared), OR of: 1 non-positive Cholesky pivot, 2 first CholeskyQR pass too far from orthonormal
 * (both: tall-skinny fast path inside a graph, where no fallback is possible), 4 cooperative short-wide QR could not get
 * its workgroups resident, 8 the right-vector workgroup of the Jacobi SVD never saw its producer within the spin bound,
 * 16 a Jacobi SVD used up its sweep budget before converging (eager calls as well: the factors are then accurate to the
 * last sweep's rotation angles only), 32 an index handed to a gather (a permutation entry, a column index) was outside the
 * source: the affected outputs are zero instead of whatever a wild address held, 64 a block id, entry_col or group_row of
 * rc_block_operator_apply_* was out of range: that entry or group was skipped.  0 = every result stands. */
rc_status rc_get_health(rc_context *ctx, int32_t *word);

/* Stage / kernel timers: HIP events recorded on the context's stream around the
 * dominant kernels and pipeline stages (used by bench.py for the roofline line).
 * rc_profile_count / rc_profile_get synchronise the stream. */
rc_status rc_profile_enable(rc_context *ctx, int32_t on);
rc_status rc_profile_reset(rc_context *ctx);
rc_status rc_profile_count(rc_context *ctx, int32_t *n);
rc_status rc_profile_get(rc_context *ctx, int32_t i, char *name, int32_t name_cap, double *total_ms, int64_t *calls);

/* Instantiation of the most recent GEMM launch of this context, spelled as rocprofv3 prints it
 * (e.g. "k_gemm_f64q<1,1,136,256,16,2,4,2,0,0>"): lets bench.py tell whether a committed PMC traffic figure was taken on
 * the kernel that still runs.  Diagnostic, no reference counterpart. */
const char *rc_last_gemm_kernel_name(const rc_context *ctx);

/* ------------------------------------------------------- random_matrix.rs -- */
/* RandomMatrix::random_gaussian (src/random_matrix.rs:21, :120-125): i.i.d. N(0,1), drawn in f64 and cast to T,
 * filled in row-major order.  The reference's rand 0.8 / rand_distr 0.4 ziggurat stream is sequential host code with no
 * pinned version, so it cannot be reproduced sample for sample; parity tests pass Omega explicitly.  The stream of THIS
 * ABI is defined here (and restated in oracle/philox.py, which the GPU kernel is tested against bit for bit):
 *   Philox4x32-10 (Salmon et al., SC'11), key = (seed & 0xffffffff, seed >> 32), counter = (b & 0xffffffff, b >> 32, 0, 0)
 *   for block b -> words w0..w3;  a = w0 << 32 | w1,  b' = w2 << 32 | w3;
 *   u1 = ((a >> 11) + 1) * 2^-53 in (0, 1],  u2 = (b' >> 11) * 2^-53 in [0, 1);
 *   z0 = sqrt(-2 ln u1) cos(2 pi u2),  z1 = sqrt(-2 ln u1) sin(2 pi u2)   (Box-Muller);
 *   number e of the stream (seed, offset) is z_{(offset + e) & 1} of block (offset + e) >> 1;
 *   element (i, j) of out is number i * cols + j;  the f32 variant is the cast of the f64 value. */
rc_status rc_random_gaussian_f64(rc_context *ctx, rc_matrix out, uint64_t seed, uint64_t offset);
rc_status rc_random_gaussian_f32(rc_context *ctx, rc_matrix out, uint64_t seed, uint64_t offset);
/* The raw uint32 words of the same Philox stream (word w = w_{w & 3} of block w >> 2), n words from word_offset into
 * device memory `out`: the integer generator is checkable bit for bit against oracle/philox.py and Random123's
 * known-answer vectors.  No reference counterpart. */
rc_status rc_random_bits_u32(rc_context *ctx, uint32_t *out, int64_t n, uint64_t seed, uint64_t word_offset);

/* --------------------------------------------------------------- types.rs -- */
/* MatMat::matmat for dense matrices (src/types.rs:58-71, :103-121): Y = A X.
 * One GEMM instead of the reference's per-column gemv loop (blanket impl,
 * src/types.rs:145); results differ by summation order only. */
rc_status rc_matmat_f64(rc_context *ctx, rc_matrix a, rc_matrix x, rc_matrix y);
rc_status rc_matmat_f32(rc_context *ctx, rc_matrix a, rc_matrix x, rc_matrix y);
/* ConjMatMat::conj_matmat (src/types.rs:88-101, :123-133): Y = A^H X (ncols(A) x ncols(X)). */
rc_status rc_conj_matmat_f64(rc_context *ctx, rc_matrix a, rc_matrix x, rc_matrix y);
rc_status rc_conj_matmat_f32(rc_context *ctx, rc_matrix a, rc_matrix x, rc_matrix y);
/* ndarray `.dot` on two matrices (all call sites listed in SURVEY.md 2b N9):
 * C = alpha * op(A) op(B) + beta * C, op = transpose when the flag is non-zero.  BLAS semantics: beta = 0 writes C without
 * reading it (NaN or Inf already in C does not propagate); K = 0 gives C = beta * C; a, b and c are any strided views. */
rc_status rc_gemm_f64(rc_context *ctx, int32_t trans_a, int32_t trans_b, double alpha, rc_matrix a, rc_matrix b, double beta, rc_matrix c);
rc_status rc_gemm_f32(rc_context *ctx, int32_t trans_a, int32_t trans_b, float alpha, rc_matrix a, rc_matrix b, float beta, rc_matrix c);
/* RelDiff (src/types.rs:162-196): host scalar out, synchronous. */
rc_status rc_rel_diff_fro_f64(rc_context *ctx, rc_matrix first, rc_matrix second, double *out);
rc_status rc_rel_diff_fro_f32(rc_context *ctx, rc_matrix first, rc_matrix second, float *out);

/* --------------------------------------------------------- permutation.rs -- */
/* invert_permutation_vector (src/permutation.rs:28-38): inverse[perm[i]] = i.  perm and inverse are device arrays of n entries.
 * An input that is no permutation is not an error here: inverse starts at -1 everywhere, an entry outside [0, n) is skipped, and a
 * value that occurs twice leaves one of its positions (which one is not defined).  So every position that no in-range entry names
 * holds -1, and nothing outside inverse[0 .. n) is written.  The call raises no health bit itself: the gather that consumes a -1
 * rejects it (bit 32, rc_get_health), which is how the INV modes below and the to_mat / ID calls report such an input. */
rc_status rc_invert_permutation(rc_context *ctx, const int64_t *perm, int64_t n, int64_t *inverse);
/* ApplyPermutationToMatrix::apply_permutation (src/permutation.rs:84-144).
 * RC_INVALID_ARGUMENT when perm_len mismatches (the reference asserts). */
rc_status rc_apply_permutation_matrix_f64(rc_context *ctx, int32_t mode, rc_matrix in, const int64_t *perm, int64_t perm_len, rc_matrix out);
rc_status rc_apply_permutation_matrix_f32(rc_context *ctx, int32_t mode, rc_matrix in, const int64_t *perm, int64_t perm_len, rc_matrix out);
/* ApplyPermutationToVector::apply_permutation (src/permutation.rs:153-183); vectors are n x 1 views. */
rc_status rc_apply_permutation_vector_f64(rc_context *ctx, int32_t mode, rc_matrix in, const int64_t *perm, int64_t perm_len, rc_matrix out);
rc_status rc_apply_permutation_vector_f32(rc_context *ctx, int32_t mode, rc_matrix in, const int64_t *perm, int64_t perm_len, rc_matrix out);

/* ---------------------------------------------------------- pivoted_qr.rs -- */
/* PivotedQR::pivoted_qr (src/pivoted_qr.rs:25-31, :81-183) = ?geqp3 + ?orgqr:
 *   A P = Q R,  q: m x k,  r: k x n upper trapezoidal,  ind[j] = column of A at position j.
 * k = q.cols = r.rows.  k == min(m, n) reproduces the reference exactly.
 * k <  min(m, n) is the TRUNCATED factorization (stops after k Householder
 * steps): q, r[:k] and ind[:k] equal the full factorization's, ind[k:] lists
 * the remaining columns in the order the swaps left them.
 * Input scale.  The domain and the equivariance statement of the "Input scale" paragraph at rc_column_id_rank_batched_* hold for
 * this call in all four scalar types: with the largest finite real or imaginary part of a within [2^-100, 2^100] (f32 / c32) or
 * [2^-900, 2^900] (f64 / c64) the call factors 2^-e a, e the exponent of that part (taken on the device, no host read), and R takes
 * 2^e back; the result for 2^t A is the result for A with R times 2^t and q, ind unchanged, bit for bit while nothing leaves the
 * normal range.  A zero matrix and one with a non-finite entry are not normalised.  Inside the domain in the same way (the factor
 * that carries the scale in brackets): rc_pivoted_lq_* (l), rc_geqp3_* (R and, for kmax < min(m, n), the trailing block; tau and the
 * reflectors carry none), rc_compute_svd_* (s), rc_column_id_two_sided_* and rc_row_id_two_sided_*, rc_max_col_norm_* (the norm) and
 * rc_rel_diff_fro_* (none: both operands are read times 2^-e, e taken over both).  The calls that take such factors (rc_qr_column_id_*,
 * rc_lq_row_id_*, rc_*_to_mat_*, rc_rank_by_tolerance_*) form no squares of them.
 * NOT inside it -- no input-scale domain is promised yet: rc_sample_range_*, rc_qr_from_range_estimate_*, rc_svd_from_range_estimate_*
 * and rc_rsvd_id_*, their _op_ forms and the row-sharded call (they factor the sketch A Omega and the projection Q^H A on the timed
 * chain without normalising them), and rc_column_id_rank_* with rc_batch_column_id_* (the lone call restores from a and reads C
 * from it, and the batch promises the lone call's bits). */
rc_status rc_pivoted_qr_f64(rc_context *ctx, rc_matrix a, rc_matrix q, rc_matrix r, int64_t *ind);
rc_status rc_pivoted_qr_f32(rc_context *ctx, rc_matrix a, rc_matrix q, rc_matrix r, int64_t *ind);
/* PivotedQR::pivoted_lq (src/pivoted_qr.rs:32-41), LQ::compute_from (src/qr.rs:354-362):
 *   P A = L Q,  l: m x k,  q: k x n,  ind: m. */
rc_status rc_pivoted_lq_f64(rc_context *ctx, rc_matrix a, rc_matrix l, rc_matrix q, int64_t *ind);
rc_status rc_pivoted_lq_f32(rc_context *ctx, rc_matrix a, rc_matrix l, rc_matrix q, int64_t *ind);

/* LAPACK granularity, for a maintainer who swaps only the `$qrf` call (src/pivoted_qr.rs:139-172, ?geqp3), `lax::Lapack::q`
 * (src/pivoted_qr.rs:104-108, ?orgqr / ?ungqr) or the triangular solves of the IDs (src/qr.rs:298, :392, ?trtrs) and keeps the
 * reference's own code around them.  All pointers are DEVICE pointers.
 * rc_geqp3: a (m x n, any strides) is overwritten with LAPACK's output format -- the factorization of A P, columns in pivoted order:
 *   R on and above the diagonal of the first kmax rows, Householder vectors below it in the first kmax columns; jpvt (n, 0-based:
 *   LAPACK's minus one), tau (kmax).  kmax == min(m, n) is ?geqp3; kmax < min(m, n) stops after kmax steps (rows >= kmax of the
 *   columns >= kmax are then unspecified).
 * rc_orgqr: q (m x k) = H_0 ... H_{k-1} [I; 0] from the first k columns of such an a and tau.
 * rc_trsm_upper: T X = B in place (t: k x k upper triangular, b: k x nrhs); no singularity check (?trtrs' INFO is not reproduced). */
rc_status rc_geqp3_f64(rc_context *ctx, rc_matrix a, int64_t kmax, int64_t *jpvt, double *tau);
rc_status rc_geqp3_f32(rc_context *ctx, rc_matrix a, int64_t kmax, int64_t *jpvt, float *tau);
rc_status rc_orgqr_f64(rc_context *ctx, rc_matrix a, const double *tau, int64_t k, rc_matrix q);
rc_status rc_orgqr_f32(rc_context *ctx, rc_matrix a, const float *tau, int64_t k, rc_matrix q);
rc_status rc_trsm_upper_f64(rc_context *ctx, rc_matrix t, rc_matrix b);
rc_status rc_trsm_upper_f32(rc_context *ctx, rc_matrix t, rc_matrix b);

/* ---------------------------------------------------------- compute_svd.rs -- */
/* ComputeSVD::compute_svd (src/compute_svd.rs:18-27) = thin ?gesdd:
 *   u: m x r, s: r (device, descending), vt: r x n, r = min(m, n).
 * Singular vectors are unique up to a sign per pair; S and U diag(S) Vt match gesdd. */
rc_status rc_compute_svd_f64(rc_context *ctx, rc_matrix a, rc_matrix u, double *s, rc_matrix vt);
rc_status rc_compute_svd_f32(rc_context *ctx, rc_matrix a, rc_matrix u, float *s, rc_matrix vt);

/* ------------------------------------------------------------------ qr.rs -- */
/* compress_qr_tolerance / compress_lq_tolerance (src/qr.rs:187-200, :99-112):
 * first i with |d_ii / d_00| < tol on the diagonal of `tri` (R or L).
 * RC_COMPRESSION_ERROR if none, RC_INVALID_ARGUMENT unless 0 <= tol < 1. Synchronous. */
rc_status rc_rank_by_tolerance_f64(rc_context *ctx, rc_matrix tri, double tol, int64_t *rank);
rc_status rc_rank_by_tolerance_f32(rc_context *ctx, rc_matrix tri, double tol, int64_t *rank);
/* QRTraits::to_mat (src/qr.rs:160-166): out = Q (R with COLINV permutation). */
rc_status rc_qr_to_mat_f64(rc_context *ctx, rc_matrix q, rc_matrix r, const int64_t *ind, rc_matrix out);
rc_status rc_qr_to_mat_f32(rc_context *ctx, rc_matrix q, rc_matrix r, const int64_t *ind, rc_matrix out);
/* LQTraits::to_mat (src/qr.rs:73-77): out = (L with ROWINV permutation) Q. */
rc_status rc_lq_to_mat_f64(rc_context *ctx, rc_matrix l, rc_matrix q, const int64_t *ind, rc_matrix out);
rc_status rc_lq_to_mat_f32(rc_context *ctx, rc_matrix l, rc_matrix q, const int64_t *ind, rc_matrix out);
/* QRTraits::column_id (src/qr.rs:270-309): c: m x k, z: k x n (both branches).
 * `ind` (n entries) is the caller's and is checked: an entry outside [0, n) is skipped, a column of z that no in-range entry names is
 * exactly zero, nothing is written outside z or read outside r, and health bit 32 is raised in either case (a duplicated entry leaves
 * such a column; the column it names twice holds the result of one of the two positions).  c = q r[:, :k] does not depend on ind. */
rc_status rc_qr_column_id_f64(rc_context *ctx, rc_matrix q, rc_matrix r, const int64_t *ind, rc_matrix c, rc_matrix z);
rc_status rc_qr_column_id_f32(rc_context *ctx, rc_matrix q, rc_matrix r, const int64_t *ind, rc_matrix c, rc_matrix z);
/* LQTraits::row_id (src/qr.rs:363-403): x: m x k, r_rows: k x n.  `ind` (m entries) is checked like rc_qr_column_id's: rows of x
 * that no in-range entry names are exactly zero, health bit 32. */
rc_status rc_lq_row_id_f64(rc_context *ctx, rc_matrix l, rc_matrix q, const int64_t *ind, rc_matrix x, rc_matrix r_rows);
rc_status rc_lq_row_id_f32(rc_context *ctx, rc_matrix l, rc_matrix q, const int64_t *ind, rc_matrix x, rc_matrix r_rows);
/* QRTraits::compute_from_range_estimate (src/qr.rs:311-323): range m x r', A m x n ->
 * q: m x k, r: k x n, ind: n, with k = min(r', n). */
rc_status rc_qr_from_range_estimate_f64(rc_context *ctx, rc_matrix range, rc_matrix a, rc_matrix q, rc_matrix r, int64_t *ind);
rc_status rc_qr_from_range_estimate_f32(rc_context *ctx, rc_matrix range, rc_matrix a, rc_matrix q, rc_matrix r, int64_t *ind);

/* ----------------------------------------------------------------- svd.rs -- */
/* compress_svd_tolerance (src/svd.rs:87-101) on a device vector of singular values. Synchronous. */
rc_status rc_svd_rank_by_tolerance_f64(rc_context *ctx, const double *s, int64_t len, double tol, int64_t *rank);
rc_status rc_svd_rank_by_tolerance_f32(rc_context *ctx, const float *s, int64_t len, double tol, int64_t *rank);
/* SVDTraits::to_mat (src/svd.rs:42-54): out = U diag(S) Vt. */
rc_status rc_svd_to_mat_f64(rc_context *ctx, rc_matrix u, const double *s, rc_matrix vt, rc_matrix out);
rc_status rc_svd_to_mat_f32(rc_context *ctx, rc_matrix u, const float *s, rc_matrix vt, rc_matrix out);
/* SVDTraits::to_qr (src/svd.rs:150-163): pivoted QR of diag(S) Vt, Q = U Q_b. */
rc_status rc_svd_to_qr_f64(rc_context *ctx, rc_matrix u, const double *s, rc_matrix vt, rc_matrix q, rc_matrix r, int64_t *ind);
rc_status rc_svd_to_qr_f32(rc_context *ctx, rc_matrix u, const float *s, rc_matrix vt, rc_matrix q, rc_matrix r, int64_t *ind);
/* SVDTraits::compute_from_range_estimate (src/svd.rs:171-183): u: m x r', s: r', vt: r' x n. */
rc_status rc_svd_from_range_estimate_f64(rc_context *ctx, rc_matrix range, rc_matrix a, rc_matrix u, double *s, rc_matrix vt);
rc_status rc_svd_from_range_estimate_f32(rc_context *ctx, rc_matrix range, rc_matrix a, rc_matrix u, float *s, rc_matrix vt);

/* ------------------------------- col_interp_decomp.rs / row_interp_decomp.rs -- */
/* ColumnIDTraits::two_sided_id (src/col_interp_decomp.rs:116-125): from C (m x k)
 * computes the row ID of C: c_out: m x k (= row_id.x), x: k x k (= row_id.r), row_ind: m.
 * (r = Z and col_ind are carried over unchanged by the caller.) */
rc_status rc_column_id_two_sided_f64(rc_context *ctx, rc_matrix c, rc_matrix c_out, rc_matrix x, int64_t *row_ind);
rc_status rc_column_id_two_sided_f32(rc_context *ctx, rc_matrix c, rc_matrix c_out, rc_matrix x, int64_t *row_ind);
/* RowIDTraits::two_sided_id (src/row_interp_decomp.rs:120-130): from R (k x n)
 * computes the column ID of R: x: k x k (= col_id.c), r_out: k x n (= col_id.z), col_ind: n. */
rc_status rc_row_id_two_sided_f64(rc_context *ctx, rc_matrix r, rc_matrix x, rc_matrix r_out, int64_t *col_ind);
rc_status rc_row_id_two_sided_f32(rc_context *ctx, rc_matrix r, rc_matrix x, rc_matrix r_out, int64_t *col_ind);

/* ------------------------------------------------------ random_sampling.rs -- */
/* MaxColNorm::max_col_norm (src/random_sampling.rs:184-191). Synchronous, host scalar out. */
rc_status rc_max_col_norm_f64(rc_context *ctx, rc_matrix y, double *out);
rc_status rc_max_col_norm_f32(rc_context *ctx, rc_matrix y, float *out);
/* SampleRange::sample_range_by_rank (src/random_sampling.rs:103-118):
 * q: m x k = first k columns of Q in the pivoted QR of A Omega, Omega: n x (k+p).
 * omega.data == NULL => Omega is generated on the device from (seed, offset 0). */
rc_status rc_sample_range_by_rank_f64(rc_context *ctx, rc_matrix a, int64_t k, int64_t p, rc_matrix omega, uint64_t seed, rc_matrix q);
rc_status rc_sample_range_by_rank_f32(rc_context *ctx, rc_matrix a, int64_t k, int64_t p, rc_matrix omega, uint64_t seed, rc_matrix q);
/* SampleRangePowerIteration::sample_range_power_iteration (src/random_sampling.rs:131-160),
 * INCLUDING its variable-shadowing quirk: for it_count >= 1 exactly one power
 * step survives. */
rc_status rc_sample_range_power_iteration_f64(rc_context *ctx, rc_matrix a, int64_t k, int64_t p, int64_t it_count, rc_matrix omega, uint64_t seed, rc_matrix q);
rc_status rc_sample_range_power_iteration_f32(rc_context *ctx, rc_matrix a, int64_t k, int64_t p, int64_t it_count, rc_matrix omega, uint64_t seed, rc_matrix q);
/* AdaptiveSampling::sample_range_adaptive (src/random_sampling.rs:223-274).
 *   q_cap: m x cap output buffer; on return the basis is its first *rank columns.
 *   omegas: n x (sample_size * blocks) explicit Gaussian blocks consumed left to
 *           right (data == NULL => generated on device from seed).
 *   hist_rank / hist_res (host, hist_cap entries): the residual history
 *           Vec<(usize, f64)>; *hist_len entries are written.
 * Returns RC_COMPRESSION_ERROR if cap columns (or the explicit Omega blocks) are
 * exhausted before the tolerance is met.  Synchronous (the loop condition is a host scalar). */
rc_status rc_sample_range_adaptive_f64(rc_context *ctx, rc_matrix a, double rel_tol, int64_t sample_size, rc_matrix omegas, uint64_t seed, rc_matrix q_cap, int64_t *rank, int64_t *hist_rank, double *hist_res, int64_t hist_cap, int64_t *hist_len);
rc_status rc_sample_range_adaptive_f32(rc_context *ctx, rc_matrix a, double rel_tol, int64_t sample_size, rc_matrix omegas, uint64_t seed, rc_matrix q_cap, int64_t *rank, int64_t *hist_rank, double *hist_res, int64_t hist_cap, int64_t *hist_len);

/* ------------------------------------------------ operators behind callbacks -- */
/* The reference's range finders are implemented for ANY operator, not only for dense arrays:
 *   impl<Op: MatMat> SampleRange for Op            src/random_sampling.rs:102
 *   impl<Op: MatMat + ConjMatMat> SampleRangePowerIteration for Op   :130
 *   impl<Op: MatMat + ConjMatMat> AdaptiveSampling for Op            :222
 *   QRTraits / SVDTraits::compute_from_range_estimate<Op: ConjMatMat>   src/qr.rs:311-323, src/svd.rs:171-183
 * (trait contract: src/types.rs:40-51 nrows / ncols / matvec, :77-81 conj_matvec, :58-71 / :88-101 the derived products).
 * rc_operator is that contract at the C ABI: the extents and the two PRODUCTS (the per-column matvec loop of the blanket impl
 * src/types.rs:145-146 is the host's business -- a host with only a matvec loops over the columns of x inside its callback).
 *   matmat(user, ctx, x, y):       y (rows x s) = A x,    x: cols x s
 *   conj_matmat(user, ctx, x, y):  y (cols x s) = A^H x,  x: rows x s      (may be NULL where only MatMat is required)
 * x and y are strided DEVICE views (any layout; y may be the transposed view of a row-major buffer) owned by the library for the
 * duration of the call.  A callback enqueues its work on the context's stream (rc_get_stream) -- it may call this library's own
 * entry points with the SAME ctx (they nest: the outer call's workspace stays intact) or launch kernels of its own -- and returns
 * RC_OK or a status that the calling entry point then returns (rc_last_error_message names the product).  It must not synchronise
 * unless it has to; it cannot be recorded into a hipGraph (RC_INVALID_ARGUMENT while capturing).
 * The *_op_* entry points below run the same internal steps as their dense twins with the two products replaced by the callbacks:
 * a dense matrix behind callbacks that call rc_matmat / rc_conj_matmat reproduces the dense entry point bit for bit (f64; the f32
 * products pick their tiles by operand layout, so there the agreement is to rounding).  The complex scalar types have the same
 * entry points (rc_*_op_c64 / _c32, declared with the complex instantiations below; rc_rsvd_id_op_* is real-only). */
typedef struct rc_operator rc_operator;
typedef int32_t (*rc_operator_product_fn)(void *user, rc_context *ctx, rc_matrix x, rc_matrix y); /* returns an rc_status */
struct rc_operator {
    int64_t rows;                       /* MatVec::nrows  src/types.rs:44-45 */
    int64_t cols;                       /* MatVec::ncols  src/types.rs:47-48 */
    rc_operator_product_fn matmat;      /* MatMat::matmat          src/types.rs:58-71  */
    rc_operator_product_fn conj_matmat; /* ConjMatMat::conj_matmat src/types.rs:88-101 */
    void *user;
};
/* the hipStream_t the context orders its work on (for a callback's own kernels) */
rc_status rc_get_stream(rc_context *ctx, void **hip_stream);
/* SampleRange for Op (src/random_sampling.rs:102-121) */
rc_status rc_sample_range_by_rank_op_f64(rc_context *ctx, const rc_operator *op, int64_t k, int64_t p, rc_matrix omega, uint64_t seed, rc_matrix q);
rc_status rc_sample_range_by_rank_op_f32(rc_context *ctx, const rc_operator *op, int64_t k, int64_t p, rc_matrix omega, uint64_t seed, rc_matrix q);
/* SampleRangePowerIteration for Op (src/random_sampling.rs:130-163) */
rc_status rc_sample_range_power_iteration_op_f64(rc_context *ctx, const rc_operator *op, int64_t k, int64_t p, int64_t it_count, rc_matrix omega, uint64_t seed, rc_matrix q);
rc_status rc_sample_range_power_iteration_op_f32(rc_context *ctx, const rc_operator *op, int64_t k, int64_t p, int64_t it_count, rc_matrix omega, uint64_t seed, rc_matrix q);
/* AdaptiveSampling for Op (src/random_sampling.rs:222-277) */
rc_status rc_sample_range_adaptive_op_f64(rc_context *ctx, const rc_operator *op, double rel_tol, int64_t sample_size, rc_matrix omegas, uint64_t seed, rc_matrix q_cap, int64_t *rank, int64_t *hist_rank, double *hist_res, int64_t hist_cap, int64_t *hist_len);
rc_status rc_sample_range_adaptive_op_f32(rc_context *ctx, const rc_operator *op, double rel_tol, int64_t sample_size, rc_matrix omegas, uint64_t seed, rc_matrix q_cap, int64_t *rank, int64_t *hist_rank, double *hist_res, int64_t hist_cap, int64_t *hist_len);
/* QRTraits::compute_from_range_estimate<Op: ConjMatMat> (src/qr.rs:311-323) */
rc_status rc_qr_from_range_estimate_op_f64(rc_context *ctx, rc_matrix range, const rc_operator *op, rc_matrix q, rc_matrix r, int64_t *ind);
rc_status rc_qr_from_range_estimate_op_f32(rc_context *ctx, rc_matrix range, const rc_operator *op, rc_matrix q, rc_matrix r, int64_t *ind);
/* SVDTraits::compute_from_range_estimate<Op: ConjMatMat> (src/svd.rs:171-183) */
rc_status rc_svd_from_range_estimate_op_f64(rc_context *ctx, rc_matrix range, const rc_operator *op, rc_matrix u, double *s, rc_matrix vt);
rc_status rc_svd_from_range_estimate_op_f32(rc_context *ctx, rc_matrix range, const rc_operator *op, rc_matrix u, float *s, rc_matrix vt);
/* the fused pipeline below (rc_rsvd_id_*) over an operator; not capturable */
struct rc_rsvd_id_out;
rc_status rc_rsvd_id_op_f64(rc_context *ctx, const rc_operator *op, int64_t k, int64_t p, rc_matrix omega, uint64_t seed, const struct rc_rsvd_id_out *out);
rc_status rc_rsvd_id_op_f32(rc_context *ctx, const rc_operator *op, int64_t k, int64_t p, rc_matrix omega, uint64_t seed, const struct rc_rsvd_id_out *out);

/* ------------------------------------------------ fused pipeline (bench) -- */
/* cfg3 "rSVD + ID" in one call, no host synchronisation inside (capturable in
 * a hipGraph): sample_range_by_rank -> SVD::compute_from_range_estimate ->
 * QR::compute_from_range_estimate -> column_id, sharing B = Q^H A between the
 * two range-estimate consumers (identical results to calling them one by one).
 * Any output with data == NULL is skipped; id outputs all NULL => rSVD only. */
typedef struct rc_rsvd_id_out {
    rc_matrix range_q; /* m x k   */
    rc_matrix u;       /* m x k   */
    void *s;           /* k       */
    rc_matrix vt;      /* k x n   */
    rc_matrix qr_q;    /* m x k   */
    rc_matrix qr_r;    /* k x n   */
    int64_t *qr_ind;   /* n       */
    rc_matrix id_c;    /* m x k   */
    rc_matrix id_z;    /* k x n   */
} rc_rsvd_id_out;
rc_status rc_rsvd_id_f64(rc_context *ctx, rc_matrix a, int64_t k, int64_t p, rc_matrix omega, uint64_t seed, const rc_rsvd_id_out *out);
rc_status rc_rsvd_id_f32(rc_context *ctx, rc_matrix a, int64_t k, int64_t p, rc_matrix omega, uint64_t seed, const rc_rsvd_id_out *out);

/* cfg5 unit of work: rank-k column ID of one dense matrix,
 * QR::compute_from -> compress(RANK(k)) -> column_id
 * (examples/interpolative_decomposition.rs:25-32) with the truncated
 * factorization (see rc_pivoted_qr).  c: m x k, z: k x n, col_ind: n. */
rc_status rc_column_id_rank_f64(rc_context *ctx, rc_matrix a, int64_t k, rc_matrix c, rc_matrix z, int64_t *col_ind);
rc_status rc_column_id_rank_f32(rc_context *ctx, rc_matrix a, int64_t k, rc_matrix c, rc_matrix z, int64_t *col_ind);

/* ------------------------------------------- batches of independent matrices -- */
/* BASELINE.json configs[4]: many same-shaped matrices, rank-k column ID each (the call sequence of
 * examples/interpolative_decomposition.rs:25-32 per matrix), sharded by MATRIX over the GPUs of a node, then ONE exchange
 * step: the gather of the finished factor blocks.  The reference has neither a batch nor a communication layer (it is
 * single-process host code), so these entry points have no file:line counterpart beyond the per-matrix sequence.
 *
 * Packed layout, per matrix i at byte offset i * rc_batch_packed_bytes(m, n, k, sizeof(T)):
 *   C (m x k, C order) | Z (k x n, C order) | pad to 8 bytes | col_ind (n x int64). */
size_t rc_batch_packed_bytes(int64_t m, int64_t n, int64_t k, int32_t elem_size);
/* Contiguous block partition of n_items over `world` ranks (the first n_items % world ranks take one extra item):
 * matrix i of 64 goes to rank i / 8 on 8 GPUs.  Pure host arithmetic. */
rc_status rc_batch_shard_range(int64_t n_items, int32_t world, int32_t rank, int64_t *start, int64_t *count);
/* Rank-k column ID of `count` same-shaped device matrices into the packed device buffer `packed`
 * (count * rc_batch_packed_bytes).  The matrices are spread over the nctx contexts (one HIP stream each, same device) and
 * pipelined (each lane is waited for on its own event, first in, first out; idle lanes take the next matrix); results are identical to count calls of
 * rc_column_id_rank_* on a context with the options of ctxs[0]: shapes the lone call takes off the truncated blocked factorization
 * (tall-skinny, short-wide, k == n, shapes too small for the panels) run the lone call's own routine on their lane.  Which lane a matrix
 * runs on depends on the timing, so the contexts must agree: a context on another device than ctxs[0], or one whose RC_OPT_BLOCKED_QRCP,
 * RC_OPT_COOP_PANEL, RC_OPT_TALL_SKINNY_FAST_PATH, RC_OPT_WIDE_COOP_QRCP or RC_OPT_WIDE_LAZY_QRCP differs from ctxs[0]'s, or whose
 * min(RC_OPT_CONCURRENCY_HINT, RC_OPT_KERNEL_SLOTS) does (it sizes the launches: bits are promised per value), is rejected with
 * RC_INVALID_ARGUMENT (the message names the lane) before anything is launched; the complex twins (rc_batch_column_id_c64 / _c32), whose
 * factorization no option selects, reject a context on another device the same way.  Blocking: returns when every factor is in `packed`.
 * Errors are reported on ctxs[0]; when the call returns an error the contents of every packed slot are undefined. */
rc_status rc_batch_column_id_f64(rc_context *const *ctxs, int32_t nctx, const rc_matrix *mats, int32_t count, int64_t k, void *packed);
rc_status rc_batch_column_id_f32(rc_context *const *ctxs, int32_t nctx, const rc_matrix *mats, int32_t count, int64_t k, void *packed);
/* Many SMALL same-shaped matrices (blocks of a hierarchical matrix / FMM operator) in one stream-ordered call: no host
 * synchronisation inside, capturable between rc_graph_begin_capture and rc_graph_end_capture.  Matrix i is the view `a` with its
 * data moved by i * a_batch_stride elements (0 is legal); c (m x k) and z (k x n) likewise with their own batch strides;
 * col_ind (count x n) and ranks (count) are contiguous; every pointer is a device pointer.  Per matrix the sequence of
 * rc_column_id_rank_*: truncated pivoted QR with ?geqp3's pivots, k clamped to min(m, n), rank r = the first j < k with
 * R_jj == 0 or (tol > 0 and |R_jj / R_00| < tol) (src/qr.rs:187-200 as a ratio), else k -- so tol = 0 is fixed rank k, a
 * matrix of lower exact rank stops at it, an all-zero matrix has rank 0, and where the reference could not compress the rank is k
 * (no per-matrix error).  ranks[i] = r; col_ind[i, :] is the full permutation (pivots first); C[:, j] = A[:, ind[j]] bit for bit
 * and Z = [I | R11^-1 R12] P^T for j < r; columns r..k-1 of C and rows r..k-1 of Z are zero.  Matrix i's bits depend on matrix
 * i alone.  Non-finite input stays inside its matrix's outputs (values unspecified, col_ind still a permutation, 0 <= r <= k).
 * Domain: 1 <= m, n <= 512, 1 <= k <= 128, 0 <= tol < 1, count >= 0 (0: nothing to do); RC_INVALID_ARGUMENT otherwise, for
 * wrong c / z shapes, and for an output batch stride smaller than one output view's span.  Workspace: bounded, not by count.
 * Complex scalars (c64, c32): the same signature, domain, layout, checks and contract with interleaved (re, im) data, strides and
 * batch strides in complex elements; the pivots and the rank rule are on the real partial norms and the real R_jj of ?geqp3's
 * complex Householder QR, and C[:, j] = A[:, ind[j]] bit for bit.
 * Input scale.  Domain: the largest finite modulus of a block lies within [2^-100, 2^100] for f32 / c32 and within [2^-900, 2^900]
 * for f64 / c64 (a zero block is inside it).  Inside it no column norm and no ?larfg norm is taken as an unscaled sum of squares:
 * the working copy is brought to a largest real or imaginary part in [1, 2) by an exact power of two, as ?nrm2's scaling keeps
 * LAPACK's sums inside the range.  Equivariance: the result for 2^e A is the result for A with C, X, s and P (and the sketch Y)
 * multiplied by 2^e and everything else -- ranks, permutations, Z, R, U, Vt, Q -- unchanged, bit for bit while no input, output or
 * working quantity leaves the normal range (an entry more than about 2^63 (f32) or 2^511 (f64) below the block's largest has a
 * subnormal or zero square, as it is below every accuracy of the result).  Outside the domain: values unspecified, but contained in
 * the block's outputs as for non-finite input (permutations still permutations, 0 <= r <= k); a block with a non-finite entry is
 * not normalised.  The same paragraph holds for rc_two_sided_id_rank_batched_*, rc_svd_rank_batched_*,
 * rc_sketch_column_id_rank_batched_* / _complex_batched_* and rc_sketch_range_step_batched_*, which refer to it.
 * The recompressions (every rc_lowrank_recompress_*batched_* entry point, real and complex) are inside it, per operand: each of left,
 * mid, s and right that is present has its largest real or imaginary part in the range above, and so has the sum of their exponents,
 * which is the exponent s_out is written with.  Each operand is loaded times the exact power of two that brings that part to [1, 2);
 * the QRs, the core, the iteration and the rank rule run on the normalised copies and s_out takes the product of the four powers
 * back.  Scaling any operand by 2^e scales s_out by 2^e and leaves u, vt and ranks unchanged, bit for bit under the condition above;
 * so does a set with every operand extreme and a product at unit scale (left and mid times 2^e, s and right times 2^-e).
 * rc_lowrank_residual_batched_* is inside it for err and nrm, which carry 2^e with a and the factors' product (see its Arithmetic
 * paragraph; e is plain arithmetic and carries 2^e exactly).  Still outside, the caller's: the apply and dense entry points, and the
 * intermediate products of the residual's rebuild, diag(s) right and mid (diag(s) right), which are formed as the operands stand
 * and overflow or vanish for a split-scale factor set whose product would be in range. */
rc_status rc_column_id_rank_batched_f64(rc_context *ctx, rc_matrix a, int64_t a_batch_stride, int32_t count, int64_t k, double tol, rc_matrix c, int64_t c_batch_stride, rc_matrix z, int64_t z_batch_stride, int64_t *col_ind, int64_t *ranks);
rc_status rc_column_id_rank_batched_f32(rc_context *ctx, rc_matrix a, int64_t a_batch_stride, int32_t count, int64_t k, double tol, rc_matrix c, int64_t c_batch_stride, rc_matrix z, int64_t z_batch_stride, int64_t *col_ind, int64_t *ranks);
rc_status rc_column_id_rank_batched_c64(rc_context *ctx, rc_matrix a, int64_t a_batch_stride, int32_t count, int64_t k, double tol, rc_matrix c, int64_t c_batch_stride, rc_matrix z, int64_t z_batch_stride, int64_t *col_ind, int64_t *ranks);
rc_status rc_column_id_rank_batched_c32(rc_context *ctx, rc_matrix a, int64_t a_batch_stride, int32_t count, int64_t k, double tol, rc_matrix c, int64_t c_batch_stride, rc_matrix z, int64_t z_batch_stride, int64_t *col_ind, int64_t *ranks);
/* The two-sided ID A ~ C X R of the same batch (ColumnIDTraits::two_sided_id after the column ID, src/col_interp_decomp.rs:116-125)
 * in the same one stream-ordered, capturable call.  Domain, batch layout and checks as rc_column_id_rank_batched_*: k clamped to
 * min(m, n); c (m x k), x (k x k) and r (k x n) each moved by its own batch stride; row_ind (count x m), col_ind (count x n) and
 * ranks (count) contiguous; every pointer a device pointer.  Column side: bit for bit rc_column_id_rank_batched_* on the same
 * input -- ranks[i] = r, col_ind[i, :] the full permutation, r = its Z ([I | R11^-1 R12] P^T on rows < r, rows r..k-1 zero).  Row
 * side: ?geqp3 pivoting of C^T, C = A[:, col_ind[:r]] read bit for bit from a, with tol = 0 and at most r steps; row_ind[i, :] is
 * the full row permutation (pivots first), c[:, :r] = Z2^T with Z2 = [I | R11^-1 R12] P2^T the Z of C^T (so c[row_ind[:r], :r] is
 * exactly the identity), x[:r, :r] = A[row_ind[:r], col_ind[:r]] bit for bit; columns r..k-1 of c and rows and columns r..k-1 of x
 * are zero.  The row side stops early only on an exactly zero pivot; the columns of c from that step on are then zero (ranks[i]
 * still r).  r = 0: row_ind[i, :] is the identity and c, x, r are zero.  Per matrix this is rc_column_id_rank_* at rank r followed
 * by rc_column_id_two_sided_*, except that pivots may differ where the two reduction orders split a near-tie and that X is
 * gathered from A rather than re-formed as L Q; c x r reconstructs A (the reference TwoSidedID's c, x, r, row_ind, col_ind).
 * Matrix i's bits depend on matrix i alone.  Non-finite input stays inside its matrix's outputs (values unspecified, row_ind and
 * col_ind still permutations, 0 <= r <= k).  RC_INVALID_ARGUMENT for an out-of-domain argument, wrong c / x / r shapes, an output
 * batch stride smaller than one output view's span, or a null pointer.  Workspace: bounded, not by count.
 * Complex scalars (c64, c32): the same signature, domain, layout, checks and contract; the row side factors C^H (the conjugate
 * transpose, as rc_column_id_two_sided_c* does through its pivoted LQ of C) and c[:, :r] = Z2^H with Z2 the Z of C^H, so that
 * c[row_ind[:r], :r] is still exactly the identity; x[:r, :r] = A[row_ind[:r], col_ind[:r]] bit for bit (not conjugated).
 * Input scale: the paragraph of rc_column_id_rank_batched_*, sentence for sentence; of the outputs x alone carries the scale. */
rc_status rc_two_sided_id_rank_batched_f64(rc_context *ctx, rc_matrix a, int64_t a_batch_stride, int32_t count, int64_t k, double tol, rc_matrix c, int64_t c_batch_stride, rc_matrix x, int64_t x_batch_stride, rc_matrix r, int64_t r_batch_stride, int64_t *row_ind, int64_t *col_ind, int64_t *ranks);
rc_status rc_two_sided_id_rank_batched_f32(rc_context *ctx, rc_matrix a, int64_t a_batch_stride, int32_t count, int64_t k, double tol, rc_matrix c, int64_t c_batch_stride, rc_matrix x, int64_t x_batch_stride, rc_matrix r, int64_t r_batch_stride, int64_t *row_ind, int64_t *col_ind, int64_t *ranks);
rc_status rc_two_sided_id_rank_batched_c64(rc_context *ctx, rc_matrix a, int64_t a_batch_stride, int32_t count, int64_t k, double tol, rc_matrix c, int64_t c_batch_stride, rc_matrix x, int64_t x_batch_stride, rc_matrix r, int64_t r_batch_stride, int64_t *row_ind, int64_t *col_ind, int64_t *ranks);
rc_status rc_two_sided_id_rank_batched_c32(rc_context *ctx, rc_matrix a, int64_t a_batch_stride, int32_t count, int64_t k, double tol, rc_matrix c, int64_t c_batch_stride, rc_matrix x, int64_t x_batch_stride, rc_matrix r, int64_t r_batch_stride, int64_t *row_ind, int64_t *col_ind, int64_t *ranks);
/* Truncated SVDs of the same kind of batch (SVD::compute_from followed by compress, src/compute_svd.rs:18-27, src/svd.rs:60-101) in
 * one stream-ordered, capturable call.  Batch layout as rc_column_id_rank_batched_*: matrix i is `a` moved by i * a_batch_stride
 * elements (0 is legal); u (m x k) and vt (k x n) each moved by its own batch stride; s (count x p, p = min(m, n)) and ranks (count)
 * contiguous; every pointer a device pointer.  Domain: 1 <= m, n <= 512, min(m, n) <= 128, 1 <= k <= 128 (clamped to p),
 * 0 <= tol < 1, count >= 0 (0: nothing to do); RC_INVALID_ARGUMENT otherwise, for wrong u / vt shapes, an output batch stride
 * smaller than one output view's span, or a null pointer.  Workspace: bounded, not by count.
 * s[i, :] holds all p singular values of matrix i in descending order (the discarded tail is the truncation error).  Rank r = the
 * first j < k with s_j == 0 or (tol > 0 and s_j / s_0 < tol), else k: tol = 0 is compress_svd_rank(k), a matrix of lower exact rank
 * stops at it, an all-zero matrix has rank 0, and where compress_svd_tolerance raises CompressionError the rank is k (no per-matrix
 * error).  ranks[i] = r; u[:, :r], s[:r], vt[:r, :] are the leading singular triplets; columns r..k-1 of u and rows r..k-1 of vt are
 * zero.  Signs: the largest-|.| entry of each kept column of u is positive (the first such on a tie), the matching row of vt follows
 * it (?gesdd leaves them open).  Matrix i's bits depend on matrix i alone: not on count, the neighbours, the input or output
 * strides, or graph replay against an eager call.  Non-finite input stays inside its matrix's outputs (values unspecified,
 * 0 <= r <= k).  A matrix whose Jacobi iteration uses up its sweep budget ORs bit 16 into the health word.  Per matrix: pivoted
 * Householder QR to the p x p factor, one-sided Jacobi on it, U = Q [U_R; 0]; not bit-equal to rc_compute_svd_*, whose QR differs.
 * Complex scalars (c64, c32): the same signature, domain, layout, checks, rank rule, zero tails and health bit with interleaved
 * (re, im) data, strides and batch strides in complex elements; s has the real type (double for c64, float for c32).  u is m x k and
 * vt = V^H (k x n, the conjugate transpose, as in rc_compute_svd_c*), so u[:, :r] diag(s[:r]) vt[:r, :] is the rank-r truncation.
 * Phases replace the sign rule: in each kept column of u, the first (in row order) of its largest-modulus entries is exactly
 * (|u_ic|, 0), the column having been multiplied by that unit phase, and the matching row of vt by its inverse (?gesdd leaves the
 * phase open; with the rule a separated triplet is unique).  conj(A) gives the same s and ranks and the conjugates of u and vt, bit
 * for bit.  Per matrix: complex pivoted Householder QR to the p x p factor R, one-sided complex Jacobi on R^H, U = Q [U_R; 0]; a wide
 * matrix is factored through its transpose.
 * Input scale: the paragraph of rc_column_id_rank_batched_*, sentence for sentence; of the outputs s alone carries the scale. */
rc_status rc_svd_rank_batched_f64(rc_context *ctx, rc_matrix a, int64_t a_batch_stride, int32_t count, int64_t k, double tol, rc_matrix u, int64_t u_batch_stride, double *s, rc_matrix vt, int64_t vt_batch_stride, int64_t *ranks);
rc_status rc_svd_rank_batched_f32(rc_context *ctx, rc_matrix a, int64_t a_batch_stride, int32_t count, int64_t k, double tol, rc_matrix u, int64_t u_batch_stride, float *s, rc_matrix vt, int64_t vt_batch_stride, int64_t *ranks);
rc_status rc_svd_rank_batched_c64(rc_context *ctx, rc_matrix a, int64_t a_batch_stride, int32_t count, int64_t k, double tol, rc_matrix u, int64_t u_batch_stride, double *s, rc_matrix vt, int64_t vt_batch_stride, int64_t *ranks);
rc_status rc_svd_rank_batched_c32(rc_context *ctx, rc_matrix a, int64_t a_batch_stride, int32_t count, int64_t k, double tol, rc_matrix u, int64_t u_batch_stride, float *s, rc_matrix vt, int64_t vt_batch_stride, int64_t *ranks);
/* Apply, or rebuild, every block of such a batch from its factors in one stream-ordered, capturable call that reads the ranks on the
 * device: the reference's Apply::dot (vector and matrix) and to_mat of the column ID (src/col_interp_decomp.rs:63-65, :134-154), the
 * two-sided ID (src/two_sided_interp_decomp.rs:62-65, :159-170) and the SVD (src/svd.rs:42-55) for the outputs of the three batched
 * calls above.  One entry point covers the three factor forms:
 *   left  (m x k)  C of the column ID, C of the two-sided ID, U of the SVD
 *   mid   (k x k)  X of the two-sided ID; mid.data == NULL: none
 *   s              the SVD's singular values: row i = s + i * s_stride, at least k reals (double for f64 / c64, float for f32 / c32); NULL: none
 *   right (k x n)  Z, R, Vt
 *   ranks          count device values; NULL: every rank is k
 *   b     (n x nrhs) the right-hand sides; b.data == NULL: reconstruct (to_mat)
 *   y     (m x nrhs), or m x n when reconstructing
 * Block i of every operand is its view moved by i times its batch stride (0 is legal for the inputs, for example one b shared by all
 * blocks); any row and column strides; y must not overlap an input; every pointer a device pointer.  With r = ranks[i] clamped to
 * [0, k] (k without ranks), per block: W = right_i[:r, :] b_i (W = right_i[:r, :] when reconstructing); with s, W = diag(s_i[:r]) W;
 * with mid, W = mid_i[:r, :r] W; y_i = left_i[:, :r] W; r = 0 gives y_i = 0.  Nothing is conjugated (vt is already V^H).  The
 * transposed apply A^T x is the same call with left = right^T and right = left^T passed as strided views (rows and columns and their
 * strides swapped).  Elements of left, mid, s and right at an index >= r are never read: they may hold anything, NaN included, so the
 * result does not rely on the zero tails the batched calls write.  Block i's bits depend on block i's operands, their row and column
 * strides and the call's shapes alone: not on count, the neighbours, any batch stride, the grid, or graph replay against an eager call
 * (each output element is summed in a fixed order).  Domain: 1 <= m, n <= 512, 1 <= k <= 128, nrhs >= 1, count >= 0 (0: nothing to
 * do).  RC_INVALID_ARGUMENT for an argument outside the domain, inconsistent shapes (left.cols != right.rows, mid not k x k,
 * b.rows != n, y not m x nrhs, or not m x n when reconstructing), a y batch stride smaller than one view's span, a null left, right or
 * y pointer with count > 0, or a null ctx.  No host synchronisation, no workspace: the r x nrhs intermediate never leaves the chip.
 * Complex scalars (c64, c32): the same signature and contract with interleaved (re, im) data, strides and batch strides in complex
 * elements; s has the real type. */
rc_status rc_lowrank_apply_batched_f64(rc_context *ctx, rc_matrix left, int64_t left_batch_stride, rc_matrix mid, int64_t mid_batch_stride, const double *s, int64_t s_stride, rc_matrix right, int64_t right_batch_stride, const int64_t *ranks, int32_t count, rc_matrix b, int64_t b_batch_stride, rc_matrix y, int64_t y_batch_stride);
rc_status rc_lowrank_apply_batched_f32(rc_context *ctx, rc_matrix left, int64_t left_batch_stride, rc_matrix mid, int64_t mid_batch_stride, const float *s, int64_t s_stride, rc_matrix right, int64_t right_batch_stride, const int64_t *ranks, int32_t count, rc_matrix b, int64_t b_batch_stride, rc_matrix y, int64_t y_batch_stride);
rc_status rc_lowrank_apply_batched_c64(rc_context *ctx, rc_matrix left, int64_t left_batch_stride, rc_matrix mid, int64_t mid_batch_stride, const double *s, int64_t s_stride, rc_matrix right, int64_t right_batch_stride, const int64_t *ranks, int32_t count, rc_matrix b, int64_t b_batch_stride, rc_matrix y, int64_t y_batch_stride);
rc_status rc_lowrank_apply_batched_c32(rc_context *ctx, rc_matrix left, int64_t left_batch_stride, rc_matrix mid, int64_t mid_batch_stride, const float *s, int64_t s_stride, rc_matrix right, int64_t right_batch_stride, const int64_t *ranks, int32_t count, rc_matrix b, int64_t b_batch_stride, rc_matrix y, int64_t y_batch_stride);
/* Recompress every factor pair of such a batch to a truncated SVD without forming the m x n blocks, in one stream-ordered, capturable
 * call: rounded addition of low-rank blocks (U1 S1 V1^T + U2 S2 V2^T is the pair [U1 U2] diag(s1, s2) [V1^T; V2^T] of inner width
 * K = k1 + k2), the conversion of a batched column or two-sided ID into an SVD, and re-truncation.  Per block the reference's scheme
 * of SVD::to_qr and compute_from_range_estimate (src/svd.rs:150-163, :171-): factor the thin factors, take the SVD of the small core,
 * multiply back; the rank rule is SVDTraits::compress's (src/svd.rs:60-101).  These two are the real scalars; complex factors go
 * through rc_lowrank_recompress_complex_batched_c64 / _c32 below.
 * Inputs as rc_lowrank_apply_batched_*: left (m x K), mid (K x K; mid.data == NULL: none), s (row i = s + i * s_stride, at least K
 * reals; NULL: none), right (K x n), in_ranks (count device values; NULL: every inner rank is K).  Block i of every operand is its
 * view moved by i times its batch stride (0 is legal for the inputs); any row and column strides; every pointer a device pointer.
 * Outputs as rc_svd_rank_batched_*: u (m x kk) and vt (kk x n) with kk = min(k, K), each moved by its own batch stride; s_out
 * (count x K) and ranks (count) contiguous.  The outputs must not overlap the inputs or one another.
 * Per block, with q = in_ranks[i] clamped to [0, K] and A_i = left[:, :q] mid[:q, :q] diag(s[:q]) right[:q, :] (absent factors omitted):
 *   s_out[i, :q] are the q singular values of A_i in descending order, s_out[i, q:K] is zero;
 *   ranks[i] = r = the first j < min(kk, q) with s_j == 0 or (tol > 0 and s_j / s_0 < tol), else min(kk, q);
 *   u[:, :r], vt[:r, :] are the leading singular vectors, columns r..kk-1 of u and rows r..kk-1 of vt are zero;
 *   signs as rc_svd_rank_batched_*: the first largest-|.| entry of each kept column of u is positive;
 *   q = 0 gives rank 0 and all-zero outputs.
 * Elements of left, mid, s and right at an index >= q are never read: they may hold anything, NaN included.  An exactly zero column
 * of left inside the first q (the zero tails the batched SVD writes, after a concatenation) gives an exactly zero singular value,
 * so at tol = 0 the rank stops at the number of nonzero columns.  Block i's bits depend on block i's operands, their row and column
 * strides and the call's shapes alone: not on count, the neighbours, any batch stride, the grid, or graph replay against an eager
 * call.  Non-finite input stays inside its block's outputs (values unspecified, 0 <= r <= kk).  A block whose Jacobi iteration uses
 * up its sweep budget ORs bit 16 into the health word.  Accuracy: backward stable with respect to the factors, that is errors of a
 * few eps ||left_q||_2 ||mid diag(s)||_2 ||right_q||_2, which cancellation between the factors can make large relative to s_0.
 * Per block: pivoted Householder QR of left[:, :q] and of right[:q, :]^T (q steps each), the q x q core
 * R_L P_L^T mid diag(s) P_R R_R^T summed in a fixed order, one-sided Jacobi on its transpose, U = Q_L [U_c; 0], V = Q_R [V_c; 0]:
 * O((m + n) q^2) work instead of the O(m n min(m, n)) of rebuilding the block, and no limit of 128 on min(m, n).
 * Domain: 1 <= m, n <= 512, 1 <= K <= 128, K <= min(m, n), k >= 1, 0 <= tol < 1, count >= 0 (0: nothing to do).  A pair with
 * K > min(m, n) is cheaper through rc_lowrank_apply_batched_* (to_mat) followed by rc_svd_rank_batched_*.  RC_INVALID_ARGUMENT for an
 * argument outside the domain, inconsistent shapes (left.cols != right.rows, mid not K x K, u not m x kk, vt not kk x n), an output
 * batch stride smaller than one view's span, a null left, right, u, s_out, vt or ranks with count > 0, or a null ctx.  No host
 * synchronisation; workspace bounded by the grid, not by count. */
rc_status rc_lowrank_recompress_batched_f64(rc_context *ctx, rc_matrix left, int64_t left_batch_stride, rc_matrix mid, int64_t mid_batch_stride, const double *s, int64_t s_stride, rc_matrix right, int64_t right_batch_stride, const int64_t *in_ranks, int32_t count, int64_t k, double tol, rc_matrix u, int64_t u_batch_stride, double *s_out, rc_matrix vt, int64_t vt_batch_stride, int64_t *ranks);
rc_status rc_lowrank_recompress_batched_f32(rc_context *ctx, rc_matrix left, int64_t left_batch_stride, rc_matrix mid, int64_t mid_batch_stride, const float *s, int64_t s_stride, rc_matrix right, int64_t right_batch_stride, const int64_t *in_ranks, int32_t count, int64_t k, double tol, rc_matrix u, int64_t u_batch_stride, float *s_out, rc_matrix vt, int64_t vt_batch_stride, int64_t *ranks);
/* The same recompression for factor pairs whose left factor is tall: rc_lowrank_recompress_batched_f64 / _f32's signature argument for
 * argument and its per-block contract sentence for sentence (q, s_out, the rank rule, zero tails, exact zeros, q = 0, NaN containment, health
 * bit 16, no host synchronisation, capturable), with the sign rule taken over all m rows of each kept column of u.  This is the SVD end of
 * rc_sketch_column_id_rank_batched_*: its c (m x kk), z and ranks go in as left, right and in_ranks.
 * Domain: 1 <= m <= 65536, 1 <= n <= 512, 1 <= K <= 128, K <= min(m, n), k >= 1, 0 <= tol < 1, count >= 0; the checks, status codes and
 * messages are the pair's above under the name lowrank_recompress_tall_batched.  These two are the real scalars; complex factors go through
 * rc_lowrank_recompress_tall_complex_batched_c64 / _c32 below (rc_lowrank_recompress_tall_batched_c64 / _c32 do not exist).
 * Per block: left[:, :q] is factored by a flat Householder TSQR inside the one workgroup that owns the block.  Stage 0 is the pivoted QR of
 * rows 0 .. min(m, 512) - 1; every later stage stacks the q x q triangle of the stage before on the next 512 - q rows of left, columns in the
 * pivot order so far, and runs the same q pivoted steps (so an exactly zero column of left stays exactly zero to the end).  The last triangle
 * and the cumulative permutation enter the core; right, the core, the Jacobi iteration, the sort and the rank rule are those of the call above.
 * u is formed by carrying each kept column back through the stages' stored reflectors, chunk of rows by chunk of rows.
 * Bits: as above (operands, their row and column strides and the call's shapes alone); they equal the bits of the truncated factors passed as
 * a call of inner width q, and for m <= 512 every output equals rc_lowrank_recompress_batched_*'s on the same arguments bit for bit.
 * Workspace: a workgroup's slot holds every stage's factored copy, 1 + ceil((m - 512) / (512 - K)) stages of (512 K + 2 K) elements for
 * m > 512, about 90 MiB at m = 65536, K = 128 in f64.  The grid is bounded so that all slots stay at or below 2 GiB (never below one
 * workgroup), so very tall, wide-K blocks run on few workgroups; rc_lowrank_recompress_tall_batched_plan reports the numbers.
 * Wide blocks (a tall right factor) are A^T: call with right^T, mid^T and left^T as strided views (rows and strides swapped, no copy) in the
 * places of left, mid and right, and pass vt^T as u and u^T as vt.  The sign rule then holds on the columns of V. */
rc_status rc_lowrank_recompress_tall_batched_f64(rc_context *ctx, rc_matrix left, int64_t left_batch_stride, rc_matrix mid, int64_t mid_batch_stride, const double *s, int64_t s_stride, rc_matrix right, int64_t right_batch_stride, const int64_t *in_ranks, int32_t count, int64_t k, double tol, rc_matrix u, int64_t u_batch_stride, double *s_out, rc_matrix vt, int64_t vt_batch_stride, int64_t *ranks);
rc_status rc_lowrank_recompress_tall_batched_f32(rc_context *ctx, rc_matrix left, int64_t left_batch_stride, rc_matrix mid, int64_t mid_batch_stride, const float *s, int64_t s_stride, rc_matrix right, int64_t right_batch_stride, const int64_t *in_ranks, int32_t count, int64_t k, double tol, rc_matrix u, int64_t u_batch_stride, float *s_out, rc_matrix vt, int64_t vt_batch_stride, int64_t *ranks);
/* The plan of that call as numbers, host arithmetic only (no context, no device): for blocks of m x n with inner width `inner` and
 * elements of elem_bytes (8: f64, 4: f32), *stages = the stages of a block of full inner rank, *slot_bytes = one workgroup's workspace slot,
 * *grid = what the 2 GiB bound leaves of `resident` workgroups.  RC_INVALID_ARGUMENT outside the call's domain or for a null output. */
rc_status rc_lowrank_recompress_tall_batched_plan(int64_t m, int64_t n, int64_t inner, int32_t elem_bytes, int64_t resident, int64_t *stages, int64_t *slot_bytes, int64_t *grid);
/* The same recompression for factor pairs with both factors tall (the large square blocks at the upper levels of a hierarchical matrix, the
 * pair (P, Q) of a randomized SVD of such a block): rc_lowrank_recompress_tall_batched_f64 / _f32's signature argument for argument, and
 * rc_lowrank_recompress_batched_*'s per-block contract sentence for sentence (q, s_out, the rank rule, zero tails of u and vt, an exactly zero
 * column of left[:, :q] giving an exactly zero singular value, q = 0, elements at an index >= q never read, NaN containment, health bit 16,
 * no host synchronisation, capturable).  The sign rule is the tall call's: the first largest-|.| entry over all m rows of each kept column
 * of u is positive, and vt takes u's signs.
 * Domain: 1 <= m, n <= 65536, 1 <= K <= 128, K <= min(m, n), k >= 1, 0 <= tol < 1, count >= 0; the checks, status codes and messages are the
 * pair's above under the name lowrank_recompress_large_batched.  Real scalars only: rc_lowrank_recompress_large_batched_c64 / _c32 do not
 * exist; complex pairs go to rc_lowrank_recompress_complex_large_batched_c64 / _c32 below.
 * Per block: for n > 512, right[:q, :]^T (n x q) goes through the tall call's flat Householder TSQR as left[:, :q] does: stage 0 the pivoted
 * QR of its rows 0 .. 511, every later stage the q x q triangle on the next 512 - q rows in the pivot order so far; the factor's power-of-two
 * scale is taken over all n columns.  The last triangle and the cumulative permutation enter the core; the core, the Jacobi iteration, the
 * sort and the rank rule are unchanged.  Each kept row of vt is carried back down the right factor's stages and written once, chunk by
 * chunk, with the sign already fixed on u.
 * Bits: a block's bits depend on its operands, their row and column strides and the call's shapes alone, and they equal the bits of the
 * truncated factors passed as a call of inner width q (the stage heights of both sides depend on q, not on K).  For n <= 512 every output
 * equals rc_lowrank_recompress_tall_batched_*'s on the same arguments bit for bit, so for m, n <= 512 it equals
 * rc_lowrank_recompress_batched_*'s too.  No transposition symmetry is promised: the Jacobi iteration runs on the transposed core and the
 * sign rule is on u, so the call on (right^T, mid^T, left^T) need not give the transposed bits.
 * Workspace: a workgroup's slot holds the left factor's stage copies (m > 512), then the right factor's (n > 512), then the rotations where
 * they do not fit in LDS; a side <= 512 follows the tall call's plan, so an n <= 512 call has that plan byte for byte.  The grid is bounded
 * so that all slots stay at or below 2 GiB (never below one workgroup): at m = n = 65536, K = 128 in f64, two sides of 171 stages of
 * 526336 bytes leave 11 workgroups; rc_lowrank_recompress_large_batched_plan reports the numbers. */
rc_status rc_lowrank_recompress_large_batched_f64(rc_context *ctx, rc_matrix left, int64_t left_batch_stride, rc_matrix mid, int64_t mid_batch_stride, const double *s, int64_t s_stride, rc_matrix right, int64_t right_batch_stride, const int64_t *in_ranks, int32_t count, int64_t k, double tol, rc_matrix u, int64_t u_batch_stride, double *s_out, rc_matrix vt, int64_t vt_batch_stride, int64_t *ranks);
rc_status rc_lowrank_recompress_large_batched_f32(rc_context *ctx, rc_matrix left, int64_t left_batch_stride, rc_matrix mid, int64_t mid_batch_stride, const float *s, int64_t s_stride, rc_matrix right, int64_t right_batch_stride, const int64_t *in_ranks, int32_t count, int64_t k, double tol, rc_matrix u, int64_t u_batch_stride, float *s_out, rc_matrix vt, int64_t vt_batch_stride, int64_t *ranks);
/* The plan of that call as numbers, host arithmetic only (no context, no device): as rc_lowrank_recompress_tall_batched_plan, with the
 * stages of a block of full inner rank on each side (1 for a side <= 512).  RC_INVALID_ARGUMENT outside the call's domain or for a null
 * output. */
rc_status rc_lowrank_recompress_large_batched_plan(int64_t m, int64_t n, int64_t inner, int32_t elem_bytes, int64_t resident, int64_t *stages_left, int64_t *stages_right, int64_t *slot_bytes, int64_t *grid);
/* The same call for complex factors (c64, c32): rc_lowrank_recompress_batched_f64's signature argument for argument and its contract, domain,
 * checks and error messages, with interleaved (re, im) data and every stride and batch stride in complex elements.  s, s_out and tol have the
 * real type of the data (double for c64, float for c32): s scales the columns of mid by real numbers, and singular values are real.
 * A_i = left[:, :q] mid[:q, :q] diag(s[:q]) right[:q, :] with nothing conjugated, as in rc_lowrank_apply_batched_c* and
 * rc_lowrank_residual_batched_c*; vt = V^H (so A_i ~ u diag(s_out) vt, again with nothing conjugated).  Phases as rc_svd_rank_batched_c*:
 * in each kept column of u the first entry of largest modulus is real and positive with imaginary part exactly 0, and the matching row of
 * vt carries the conjugate phase.  Conjugating every complex input gives the conjugates of u and vt and the same s_out and ranks, bit for
 * bit; inputs whose imaginary parts are all zero give u and vt with imaginary parts exactly zero.  Per block: complex pivoted Householder QR
 * of left[:, :q] and of the plain transpose right[:q, :]^T, the core R_L P_L^T mid diag(s) P_R R_R^T in complex FMAs of a fixed order,
 * one-sided Jacobi on its conjugate transpose with the rotation tests evaluated in f64, U = Q_L [U_c; 0], vt = (Q_R [conj(V_c); 0])^T.
 * The name: the stem is rc_lowrank_recompress_complex_batched_, not rc_lowrank_recompress_batched_ with a c64 / c32 suffix as the other
 * families spell their complex members, because the real pair was published as "real scalars only" and callers (and the ABI test of that
 * pair) rely on rc_lowrank_recompress_batched_c64 / _c32 not existing: a build that has this complex call is told apart by its own symbol. */
rc_status rc_lowrank_recompress_complex_batched_c64(rc_context *ctx, rc_matrix left, int64_t left_batch_stride, rc_matrix mid, int64_t mid_batch_stride, const double *s, int64_t s_stride, rc_matrix right, int64_t right_batch_stride, const int64_t *in_ranks, int32_t count, int64_t k, double tol, rc_matrix u, int64_t u_batch_stride, double *s_out, rc_matrix vt, int64_t vt_batch_stride, int64_t *ranks);
rc_status rc_lowrank_recompress_complex_batched_c32(rc_context *ctx, rc_matrix left, int64_t left_batch_stride, rc_matrix mid, int64_t mid_batch_stride, const float *s, int64_t s_stride, rc_matrix right, int64_t right_batch_stride, const int64_t *in_ranks, int32_t count, int64_t k, float tol, rc_matrix u, int64_t u_batch_stride, float *s_out, rc_matrix vt, int64_t vt_batch_stride, int64_t *ranks);
/* The complex recompression for factor pairs whose left factor is tall: rc_lowrank_recompress_complex_batched_c64 / _c32's signature argument for
 * argument (interleaved (re, im) data, strides in complex elements, real s, s_out and tol, float tol for c32) and its per-block contract sentence
 * for sentence (q, s_out, the rank rule, zero tails, exact zeros, q = 0, NaN containment, health bit 16, conjugation and zero-imaginary-part
 * symmetry, vt = V^H with nothing conjugated in the product), with the phase rule taken over all m rows of each kept column of u: the first
 * entry of largest modulus is real and positive with imaginary part exactly 0, whichever 512-row stage holds it.  This is the SVD end of
 * rc_sketch_column_id_rank_complex_batched_*: its c (m x kk), z and ranks go in as left, right and in_ranks.
 * Domain: 1 <= m <= 65536, 1 <= n <= 512, 1 <= K <= 128, K <= min(m, n), k >= 1, 0 <= tol < 1, count >= 0; the checks, status codes and
 * messages are the shared ones under the name lowrank_recompress_tall_complex_batched.
 * Per block: rc_lowrank_recompress_tall_batched_*'s staged Householder TSQR of left[:, :q] (stages of 512 rows, each later stage the q x q
 * triangle so far on the next 512 - q rows, pivoted in every stage, complex taus) and its backward pass through the stored reflectors; right,
 * the core, the Jacobi iteration, the sort and the rank rule are rc_lowrank_recompress_complex_batched_*'s.
 * Bits: the operands, their row and column strides and the call's shapes alone; those of the truncated factors passed as a call of inner width
 * q; and for m <= 512 every output equals rc_lowrank_recompress_complex_batched_*'s on the same arguments bit for bit.
 * Workspace: a slot holds 1 + ceil((m - 512) / (512 - K)) stages of (512 K + 2 K) complex elements for m > 512: 173 MiB at m = 65536, K = 128
 * in c64 (11 workgroups under the 2 GiB bound), 87 MiB in c32 (23).  Such blocks are served, slowly; the plan query below reports the numbers.
 * Wide blocks are A^T: since vt = V^H and nothing in the product is conjugated, A^T = vt^T diag(s_out) u^T is again of this form, so call with
 * right^T, mid^T and left^T as strided views in the places of left, mid and right and pass vt^T as u and u^T as vt: plain transposes of all
 * three factors, nothing conjugated.  The phase rule then holds on the columns of vt^T.
 * The name: rc_lowrank_recompress_tall_batched_c64 / _c32 stay absent for the reason given at rc_lowrank_recompress_complex_batched_*. */
rc_status rc_lowrank_recompress_tall_complex_batched_c64(rc_context *ctx, rc_matrix left, int64_t left_batch_stride, rc_matrix mid, int64_t mid_batch_stride, const double *s, int64_t s_stride, rc_matrix right, int64_t right_batch_stride, const int64_t *in_ranks, int32_t count, int64_t k, double tol, rc_matrix u, int64_t u_batch_stride, double *s_out, rc_matrix vt, int64_t vt_batch_stride, int64_t *ranks);
rc_status rc_lowrank_recompress_tall_complex_batched_c32(rc_context *ctx, rc_matrix left, int64_t left_batch_stride, rc_matrix mid, int64_t mid_batch_stride, const float *s, int64_t s_stride, rc_matrix right, int64_t right_batch_stride, const int64_t *in_ranks, int32_t count, int64_t k, float tol, rc_matrix u, int64_t u_batch_stride, float *s_out, rc_matrix vt, int64_t vt_batch_stride, int64_t *ranks);
/* The plan of that call as numbers, host arithmetic only (no context, no device): as rc_lowrank_recompress_tall_batched_plan with real_bytes
 * the size of the real type (8: c64, 4: c32); *slot_bytes counts complex elements of 2 * real_bytes.  RC_INVALID_ARGUMENT outside the call's
 * domain, for another real_bytes, resident < 1 or a null output. */
rc_status rc_lowrank_recompress_tall_complex_batched_plan(int64_t m, int64_t n, int64_t inner, int32_t real_bytes, int64_t resident, int64_t *stages, int64_t *slot_bytes, int64_t *grid);
/* The complex recompression for factor pairs with both factors tall (the large square blocks at the upper levels of a hierarchical matrix):
 * rc_lowrank_recompress_tall_complex_batched_c64 / _c32's signature argument for argument (interleaved (re, im) data, strides in complex elements,
 * real s, s_out and tol, float tol for c32) and its per-block contract sentence for sentence: A_i = left[:, :q] mid[:q, :q] diag(s[:q])
 * right[:q, :] with nothing conjugated, vt = V^H, the rank rule, s_out zero past q, u and vt zero past the rank, an exactly zero column of
 * left[:, :q] giving an exactly zero singular value, q = 0 reading no input, elements at an index >= q never read, NaN
 * containment, health bit 16, conjugation and zero-imaginary-part symmetry, no host synchronisation, capturable.  The phase rule is taken over
 * all m rows of each kept column of u: the first entry of largest modulus is exactly (|x|, 0), whichever stage holds it; the matching row of
 * vt carries the conjugate phase over all n columns.
 * Domain: 1 <= m, n <= 65536, 1 <= K <= 128, K <= min(m, n), k >= 1, 0 <= tol < 1, count >= 0; the checks, status codes and messages are the
 * shared ones under the name lowrank_recompress_complex_large_batched.
 * Per block: for n > 512 the plain transpose right[:q, :]^T (n x q) goes through the tall call's staged Householder TSQR as left[:, :q] does
 * (stage 0 the pivoted QR of its rows 0 .. 511, every later stage the q x q triangle on the next 512 - q rows in the pivot order so far,
 * complex taus); the last triangle and the cumulative permutation enter the core; the core, the Jacobi iteration, the sort and the rank rule
 * are unchanged.  Each kept row of vt is carried back down the right factor's stages and written once, chunk by chunk, times the conjugate of
 * the phase fixed on u.
 * Zero rows of right: for n > 512 an exactly zero row of right[:q, :] is an exactly zero singular value too (a zero row of the right
 * factor's R; where that R has fewer nonzero rows than the left factor's, the iteration runs on the core itself instead of its conjugate
 * transpose, in which those rows are untouched zero columns).  Not promised: for n <= 512 the call is
 * rc_lowrank_recompress_tall_complex_batched_* bit for bit, which makes no such promise and can return inaccurate singular values for a
 * zero row of right under a nonzero column of left; nor, for any n, a core whose nonzero columns are dependent for another reason (zero
 * columns of left and zero rows of right at different indices with no mid, or equal rows of right), where the singular values that
 * should vanish come out as rounding of sigma and the others can lose accuracy.  Cut left and right at the same indices, as the batched calls' zero tails are.
 * Bits: the operands, their row and column strides and the call's shapes alone; those of the truncated factors passed as a call of inner width
 * q (the stage heights of both sides depend on q, not on K); and for n <= 512 every output equals
 * rc_lowrank_recompress_tall_complex_batched_*'s on the same arguments bit for bit.  No transposition symmetry is promised.
 * Workspace: a workgroup's slot holds the left factor's stage copies (m > 512), then the right factor's (n > 512), then the core and the
 * rotations where they do not fit in LDS; an n <= 512 call has the tall complex call's plan byte for byte.  The grid is bounded so that all
 * slots stay at or below 2 GiB (never below one workgroup): at m = n = 65536, K = 128 in c64, two sides of 171 stages of 1052672 bytes leave
 * 5 workgroups; the plan query below reports the numbers.
 * The name: "complex" stands before "large", unlike rc_lowrank_recompress_tall_complex_batched_*.  The real pair was published as "real
 * scalars only" with both spellings a twin might have taken, the real stem with a c64 / c32 suffix and ..._large_complex_batched_*, named as
 * absent, and callers (and the ABI test of that pair) rely on that: neither is declared or exported, and a build that has this call is told
 * apart by its own symbol. */
rc_status rc_lowrank_recompress_complex_large_batched_c64(rc_context *ctx, rc_matrix left, int64_t left_batch_stride, rc_matrix mid, int64_t mid_batch_stride, const double *s, int64_t s_stride, rc_matrix right, int64_t right_batch_stride, const int64_t *in_ranks, int32_t count, int64_t k, double tol, rc_matrix u, int64_t u_batch_stride, double *s_out, rc_matrix vt, int64_t vt_batch_stride, int64_t *ranks);
rc_status rc_lowrank_recompress_complex_large_batched_c32(rc_context *ctx, rc_matrix left, int64_t left_batch_stride, rc_matrix mid, int64_t mid_batch_stride, const float *s, int64_t s_stride, rc_matrix right, int64_t right_batch_stride, const int64_t *in_ranks, int32_t count, int64_t k, float tol, rc_matrix u, int64_t u_batch_stride, float *s_out, rc_matrix vt, int64_t vt_batch_stride, int64_t *ranks);
/* The plan of that call as numbers, host arithmetic only (no context, no device): as rc_lowrank_recompress_large_batched_plan with real_bytes
 * the size of the real type (8: c64, 4: c32); *slot_bytes counts complex elements of 2 * real_bytes.  RC_INVALID_ARGUMENT outside the call's
 * domain, for another real_bytes, resident < 1 or a null output. */
rc_status rc_lowrank_recompress_complex_large_batched_plan(int64_t m, int64_t n, int64_t inner, int32_t real_bytes, int64_t resident, int64_t *stages_left, int64_t *stages_right, int64_t *slot_bytes, int64_t *grid);
/* The one-pass randomized column ID of every block of a batch, in one stream-ordered, capturable call: the sketch Y_i = omega_i a_i (l x n) of each
 * tall block a_i (m x n) is formed while a_i streams through the chip once, and the column ID of the small Y_i gives the pivots and Z; C is gathered
 * from a_i.  Per block this replaces the reference's randomized sequence: the projection of sample_range_by_rank (src/random_sampling.rs), then
 * QR::compute_from_range_estimate followed by column_id() (src/qr.rs:311-323): with omega = Q^H of a range estimate it is that sequence, with a
 * Gaussian omega (rc_random_gaussian_*) it is the one-pass randomized ID.  The pivoted QR runs on l rows instead of m, so m is not bounded by what
 * one workgroup holds.  Real scalars; complex blocks go to rc_sketch_column_id_rank_complex_batched_c64 / _c32 below.
 * The batch layout is rc_column_id_rank_batched_*'s: block i of every operand is its view moved by i times its batch stride; any row and column
 * strides; every pointer a device pointer.  a is m x n; omega is l x m (omega_batch_stride = 0 shares one test matrix over the batch, the usual
 * case; a_batch_stride = 0 is legal too); y is l x n and receives the sketch when y.data is not NULL (y.data == NULL: not written, the other
 * fields are then ignored); c is m x kk and z is kk x n with kk = min(k, l, n); col_ind (count x n) and ranks (count) are contiguous.  The outputs
 * must not overlap the inputs or one another.
 * Per block, with Y_i the sketch as this call computes it (and writes it to y):
 *   col_ind, ranks and z are what rc_column_id_rank_batched_* returns for the matrix Y_i with the same k and tol, bit for bit: pivots by ?geqp3's
 *     rule on Y_i, r = the first j < kk with R_jj == 0 or (tol > 0 and |R_jj / R_00| < tol), else kk, z = [I | R11^-1 R12] P^T with rows r..kk-1 zero;
 *   c[:, j] = a[:, col_ind[j]] bit for bit for j < r, columns r..kk-1 of c are zero, so a_i ~ c z to the accuracy of the sketch.
 * An element of Y_i is summed in ascending order of the row index of a, in chunks that depend on (l, m, n) alone, by v_mfma_f64_16x16x4_f64 /
 * v_mfma_f32_16x16x4_f32 (exact f32); nothing is split across workgroups or added by atomics.  The outputs do not depend on whether y is
 * requested; block i's bits depend on block i's a and omega alone: not on count, the position in the batch, the neighbours, any batch, row or
 * column stride, the grid, or graph replay against an eager call.  Non-finite input stays inside its block's outputs (values unspecified, col_ind
 * still a permutation, 0 <= r <= kk).
 * Domain: 1 <= n <= 512, 1 <= l <= 128, 1 <= m <= 65536, 1 <= k <= 128, 0 <= tol < 1, count >= 0 (0: nothing to do).  RC_INVALID_ARGUMENT for an
 * argument outside the domain, omega.cols != a.rows, a wrong y, c or z shape, an output batch stride smaller than one view's span when count > 1,
 * a null a, omega, c, z, col_ind or ranks with count > 0, or a null ctx (rejected before a device is touched).  No host synchronisation;
 * workspace bounded by the grid, not by count.
 * Input scale: the paragraph of rc_column_id_rank_batched_*, sentence for sentence, with a the block that carries the scale (omega of
 * order one): the power of two is taken from the sketch Y_i, and y and c carry the scale. */
rc_status rc_sketch_column_id_rank_batched_f64(rc_context *ctx, rc_matrix a, int64_t a_batch_stride, rc_matrix omega, int64_t omega_batch_stride, int32_t count, int64_t k, double tol, rc_matrix y, int64_t y_batch_stride, rc_matrix c, int64_t c_batch_stride, rc_matrix z, int64_t z_batch_stride, int64_t *col_ind, int64_t *ranks);
rc_status rc_sketch_column_id_rank_batched_f32(rc_context *ctx, rc_matrix a, int64_t a_batch_stride, rc_matrix omega, int64_t omega_batch_stride, int32_t count, int64_t k, double tol, rc_matrix y, int64_t y_batch_stride, rc_matrix c, int64_t c_batch_stride, rc_matrix z, int64_t z_batch_stride, int64_t *col_ind, int64_t *ranks);
/* One range step of a power iteration on every tall block of a batch, in one stream-ordered, capturable call (the two products of one
 * round of sample_range_power_iteration, src/random_sampling.rs:131-158, with the orthonormalisation between them).  Per block a_i (m x n)
 * and test matrix omega_i (l x m): the sketch Y_i = omega_i a_i (l x n), formed exactly as rc_sketch_column_id_rank_batched_* forms it (y,
 * when requested, equals that call's y bit for bit); q_i (l x n), an orthonormal basis of Y_i's rows from a column-pivoted Householder QR of
 * Y_i^T: rows 0 .. r-1 are orthonormal and span the rows of Y_i, rows r .. l-1 are exactly zero, where ranks[i] = r is the first step
 * whose R_jj is exactly zero or not finite (else l; there is no tolerance here, truncation belongs to the call that ends the chain); and
 * the projection p_i = a_i q_i^T (m x l), whose columns r .. l-1 are exactly zero.  a streams through the chip twice.  To continue a power
 * iteration, orthonormalise p with rc_lowrank_recompress_tall_batched_* (right = I, k = l, tol = 0, in_ranks = ranks) and pass u^T as the
 * next omega; rc_lowrank_recompress_tall_batched_*(left = p, right = q, in_ranks = ranks) turns the pair into a truncated SVD of a ~ p q.
 * Domain: 1 <= n <= 512, 1 <= m <= 65536, 1 <= l <= min(128, m, n), count >= 0.  Any row and column strides on every view; batch
 * strides of 0 are legal for a and omega (one omega shared by all blocks); y.data == NULL: the sketch is not written, and the other outputs
 * do not depend on that.  Outputs must not overlap inputs or one another.  Block i's bits depend on block i's a and omega and the
 * call's shapes alone.  Non-finite input stays inside its block's outputs, with 0 <= ranks[i] <= l.  RC_INVALID_ARGUMENT for an argument
 * outside the domain, omega.cols != a.rows, a wrong y, q or p shape, an output batch stride smaller than one view's span when count > 1, a
 * null a, omega, q, p or ranks with count > 0, or a null ctx (rejected before a device is touched).  No host synchronisation; workspace
 * bounded by the grid, not by count.  Real scalars; complex blocks go to rc_sketch_range_step_complex_batched_c64 / _c32 below.
 * Input scale: the paragraph of rc_column_id_rank_batched_*, sentence for sentence, with a the block that carries the scale; y and p
 * carry it, q and ranks do not.  A chain that hands p to rc_lowrank_recompress_tall_batched_f64 / _f32 keeps the equivariance: that call
 * loads left and right times exact powers of two (u is unchanged and s carries 2^e when p does). */
rc_status rc_sketch_range_step_batched_f64(rc_context *ctx, rc_matrix a, int64_t a_batch_stride, rc_matrix omega, int64_t omega_batch_stride, int32_t count, rc_matrix y, int64_t y_batch_stride, rc_matrix q, int64_t q_batch_stride, rc_matrix p, int64_t p_batch_stride, int64_t *ranks);
rc_status rc_sketch_range_step_batched_f32(rc_context *ctx, rc_matrix a, int64_t a_batch_stride, rc_matrix omega, int64_t omega_batch_stride, int32_t count, rc_matrix y, int64_t y_batch_stride, rc_matrix q, int64_t q_batch_stride, rc_matrix p, int64_t p_batch_stride, int64_t *ranks);
/* The sketch alone, for blocks of any width: per block Y_i = omega_i a_i (l x n) and nothing else, in one stream-ordered, capturable call.
 * This is the product the two calls above form inside their launch, without the factorization that bounds their n by what one workgroup
 * holds: the front end of a randomized SVD of wide or large square blocks (rc_lowrank_recompress_large_batched_* is its back end), and, on
 * transposed views, its projection.
 * a is m x n, omega is l x m, y is l x n.  The batch layout is rc_sketch_column_id_rank_batched_*'s: block i of every operand is its view
 * moved by i times its batch stride; any row and column strides on every view; batch stride 0 is legal for a and omega (one omega shared by
 * all blocks, the usual case); every pointer a device pointer.  The output must not overlap the inputs.
 * Bits: an element of Y_i is rc_sketch_column_id_rank_batched_*'s chain exactly: v_mfma_f64_16x16x4_f64 / v_mfma_f32_16x16x4_f32 (exact
 * f32) over ascending rows of a, from zero, in chunks of 32 rows, four rows per instruction.  So
 *   (i)  for n <= 512, y equals the y of rc_sketch_column_id_rank_batched_* (and of rc_sketch_range_step_batched_*) bit for bit;
 *   (ii) for any n, column j of y depends on column j of a, on omega and on m alone: not on n, on which 64-column panel or work unit holds
 *        the column, on the grid, on count, the position in the batch, the neighbours, any stride, or graph replay against an eager call.
 * From (i) and transposed views one call computes P = a Q^T: pass a' = a^T (n x m, the strides swapped), omega' = Q (l x n) and
 * y' = p^T (l x m, a transposed view of the m x l output).  For n <= 512 that p equals rc_sketch_range_step_batched_*'s p bit for bit,
 * given the same q.  Non-finite input stays inside its block, and inside the columns of y whose columns of a hold it when omega is finite.
 * Work is split over (block, 64-column panel) units on a persistent grid, so a few large blocks fill the chip; nothing is split along m and
 * nothing is added by atomics.
 * Domain: 1 <= m, n <= 65536, 1 <= l <= 128, count >= 0 (0: nothing to do).  RC_INVALID_ARGUMENT for an argument outside the domain,
 * omega.cols != a.rows, a wrong y shape, a y batch stride smaller than one view's span when count > 1, a null a, omega or y with count > 0,
 * or a null ctx (rejected before a device is touched).  No host synchronisation, no workspace.  Real scalars only:
 * rc_sketch_product_batched_c64 / _c32 do not exist. */
rc_status rc_sketch_product_batched_f64(rc_context *ctx, rc_matrix a, int64_t a_batch_stride, rc_matrix omega, int64_t omega_batch_stride, int32_t count, rc_matrix y, int64_t y_batch_stride);
rc_status rc_sketch_product_batched_f32(rc_context *ctx, rc_matrix a, int64_t a_batch_stride, rc_matrix omega, int64_t omega_batch_stride, int32_t count, rc_matrix y, int64_t y_batch_stride);
/* The complex twin of rc_sketch_column_id_rank_batched_*: the one-pass randomized column ID of every complex tall block of a batch, in one
 * stream-ordered, capturable call: the sketch Y_i = omega_i a_i (l x n) of each block a_i (m x n) is formed while a_i streams through the chip once,
 * and the column ID of the small Y_i gives the pivots and Z; C is gathered from a_i.  Nothing is conjugated: a caller who wants Q^H a passes
 * omega = Q^H (with that omega this is sample_range_by_rank's projection, then QR::compute_from_range_estimate + column_id(), src/qr.rs:311-323,
 * for the reference's c64 / c32 scalars).  The pivoted QR runs on l rows instead of m, so m is not bounded by what one workgroup holds.
 * Data are interleaved (re, im): _c64 is std::complex<double>, _c32 std::complex<float>; every stride and batch stride is in complex elements and an
 * element need only be aligned as its real type.  The batch layout is the real call's: block i of every operand is its view moved by i times its
 * batch stride; any row and column strides; every pointer a device pointer.  a is m x n; omega is l x m (omega_batch_stride = 0 shares one test
 * matrix over the batch, the usual case; a_batch_stride = 0 is legal too); y is l x n and receives the sketch when y.data is not NULL (y.data ==
 * NULL: not written, the other fields are then ignored); c is m x kk and z is kk x n with kk = min(k, l, n); col_ind (count x n) and ranks (count)
 * are contiguous int64.  The outputs must not overlap the inputs or one another.
 * Per block, with Y_i the sketch as this call computes it (and writes it to y):
 *   col_ind, ranks and z are what rc_column_id_rank_batched_c64 / _c32 returns for the matrix Y_i with the same k and tol, bit for bit: pivots on the
 *     real partial norms of ?geqp3's complex Householder QR of Y_i, r = the first j < kk with the real R_jj == 0 or (tol > 0 and |R_jj / R_00| < tol),
 *     else kk, z = [I | R11^-1 R12] P^T with rows r..kk-1 zero;
 *   c[:, j] = a[:, col_ind[j]] bit for bit for j < r, columns r..kk-1 of c are zero, so a_i ~ c z to the accuracy of the sketch.
 * The sketch runs on v_mfma_f64_16x16x4_f64 / v_mfma_f32_16x16x4_f32 with the real and imaginary parts as separate real operands.  Each of Re Y and
 * Im Y is one accumulator chain per element, from zero over the ascending rows of a, four rows per instruction; within a four-row step Re takes
 * MFMA(Om_re, A_re) then MFMA(-Om_im, A_im), Im takes MFMA(Om_re, A_im) then MFMA(Om_im, A_re) (the negation is a sign flip in a register);
 * nothing is split across workgroups or added by atomics.  The outputs do not depend on whether y is requested; block i's bits depend on block i's
 * a and omega alone: not on count, the position in the batch, the neighbours, any batch, row or column stride, where the working copy lives, the
 * grid, or graph replay against an eager call.  Two properties follow from that order:
 *   conjugation: conjugating both a and omega gives the same col_ind and ranks and the elementwise conjugate of y, c and z, bit for bit, except
 *     that a component that cancels to exactly zero is +0 either way;
 *   zero imaginary parts: with every imaginary part of a and omega +0, Re y has the bits of rc_sketch_column_id_rank_batched_f64 / _f32's y on the
 *     real parts and Im y is zero.
 * Non-finite input stays inside its block's outputs (values unspecified, col_ind still a permutation, 0 <= r <= kk).
 * Domain: 1 <= n <= 512, 1 <= l <= 128, 1 <= m <= 65536, 1 <= k <= 128, 0 <= tol < 1, count >= 0 (0: nothing to do).  RC_INVALID_ARGUMENT for an
 * argument outside the domain, omega.cols != a.rows, a wrong y, c or z shape, an output batch stride smaller than one view's span when count > 1,
 * a null a, omega, c, z, col_ind or ranks with count > 0, or a null ctx (rejected before a device is touched).  No host synchronisation;
 * workspace bounded by the grid, not by count.
 * The name: the stem is rc_sketch_column_id_rank_complex_batched_, as rc_lowrank_recompress_complex_batched_ is spelled, because the real pair was
 * published as "real scalars only" and callers (and the ABI test of that pair) rely on rc_sketch_column_id_rank_batched_c64 / _c32 not existing.
 * Input scale: the paragraph of rc_column_id_rank_batched_*, sentence for sentence, as for the real pair. */
rc_status rc_sketch_column_id_rank_complex_batched_c64(rc_context *ctx, rc_matrix a, int64_t a_batch_stride, rc_matrix omega, int64_t omega_batch_stride, int32_t count, int64_t k, double tol, rc_matrix y, int64_t y_batch_stride, rc_matrix c, int64_t c_batch_stride, rc_matrix z, int64_t z_batch_stride, int64_t *col_ind, int64_t *ranks);
rc_status rc_sketch_column_id_rank_complex_batched_c32(rc_context *ctx, rc_matrix a, int64_t a_batch_stride, rc_matrix omega, int64_t omega_batch_stride, int32_t count, int64_t k, double tol, rc_matrix y, int64_t y_batch_stride, rc_matrix c, int64_t c_batch_stride, rc_matrix z, int64_t z_batch_stride, int64_t *col_ind, int64_t *ranks);
/* The complex twin of rc_sketch_range_step_batched_*: one range step of a power iteration on every complex tall block of a batch, in one
 * stream-ordered, capturable call (the two products of one round of sample_range_power_iteration, src/random_sampling.rs:128-168, for the
 * reference's c64 / c32 scalars, with the orthonormalisation between them).  The arguments are the real call's, one for one, with a trailing
 * p_conj; data are interleaved (re, im), every stride and batch stride is in complex elements, and the batch layout is that of
 * rc_sketch_column_id_rank_complex_batched_*.  Per block a_i (m x n) and test matrix omega_i (l x m):
 *   y = omega_i a_i (l x n), nothing conjugated, formed exactly as rc_sketch_column_id_rank_complex_batched_* forms it (y, when requested, is
 *     that call's y bit for bit; y.data == NULL: not written, and the other outputs do not depend on that);
 *   q (l x n) has orthonormal rows, q q^H = I on its first r rows, which span the rows of y: y = (y q^H) q.  It comes from the column-pivoted
 *     complex Householder QR of the plain transpose y^T with ?geqp3's conventions (real R_jj): row c of q is (H_0 .. H_c e_c)^T, transposed and
 *     not conjugated (the QR of y^H would give the same q); rows r .. l-1 are exactly zero;
 *   ranks[i] = r is the first step whose real R_jj is exactly zero or not finite, else l (there is no tolerance here: truncation belongs to the
 *     call that ends the chain);
 *   p (m x l) = a_i q^H when p_conj == 0, so a_i ~ p q with nothing conjugated; columns r .. l-1 are exactly zero.  When p_conj != 0, p
 *     receives the elementwise conjugate of that: the same bits with the sign of every imaginary part flipped at the store.
 * Why p_conj: the next test matrix of a power iteration is U^H, U an orthonormal basis of p's columns, and no call here conjugates.  The tall
 * complex recompression is conjugation-symmetric bit for bit, so orthonormalising conj(p) gives conj(U), whose plain transpose, a strided
 * view, is U^H: no caller has to conjugate anything and no existing signature changes.  The recipe:
 *   a round: this call with p_conj = 1, then rc_lowrank_recompress_tall_complex_batched_*(left = p, right = I, k = l, tol = 0, in_ranks =
 *     ranks), then u^T (swap u's row and column strides) as the next omega;
 *   the SVD end: this call with p_conj = 0, then rc_lowrank_recompress_tall_complex_batched_*(left = p, right = q, in_ranks = ranks), a
 *     truncated SVD of a ~ p q; the ID end: rc_sketch_column_id_rank_complex_batched_* with the last round's u^T as omega.
 * Both products run on the MFMA in the sketched ID's order: an element of y is one accumulator chain pair (Re, Im) from zero over the ascending
 * rows of a_i, an element of p one such pair over the ascending columns of a_i with conj(q) as the left operand.  a streams through the chip
 * twice when l <= 64; above that each of the two products takes a second pass over a.  Block i's bits depend on block i's a and omega and on
 * (l, m, n, p_conj) alone.  Conjugating both a and omega gives the same ranks and the conjugates of y, q and p, bit for bit up to the sign of
 * exact zeros; with every imaginary part of a and omega +0, Re y has the bits of rc_sketch_range_step_batched_*'s y on the real parts and the
 * imaginary parts of y, q and p are exactly zero (q and p need not equal the real call's bits).  Non-finite input stays inside its block's
 * outputs, with 0 <= ranks[i] <= l.
 * Input scale: the paragraph of rc_column_id_rank_batched_* applies to this call (the working copy of y^T is brought to [1, 2) by an exact
 * power of two before the QR): y and p carry 2^e, q and ranks do not.  The complex recompressions normalise their operands as the real
 * ones do, so the chains built on this call with them are equivariant in the same way.
 * Domain: 1 <= n <= 512, 1 <= m <= 65536, 1 <= l <= min(128, m, n), count >= 0; batch strides of 0 are legal for a and omega.  Outputs must not
 * overlap inputs or one another.  RC_INVALID_ARGUMENT as for the real call, under the name sketch_range_step_complex_batched; a null ctx is
 * rejected before a device is touched.  No host synchronisation; workspace bounded by the grid, not by count.
 * The name: the _complex_batched_ stem of the family; rc_sketch_range_step_batched_c64 / _c32 stay absent, and callers tell builds apart by that. */
rc_status rc_sketch_range_step_complex_batched_c64(rc_context *ctx, rc_matrix a, int64_t a_batch_stride, rc_matrix omega, int64_t omega_batch_stride, int32_t count, rc_matrix y, int64_t y_batch_stride, rc_matrix q, int64_t q_batch_stride, rc_matrix p, int64_t p_batch_stride, int64_t *ranks, int32_t p_conj);
rc_status rc_sketch_range_step_complex_batched_c32(rc_context *ctx, rc_matrix a, int64_t a_batch_stride, rc_matrix omega, int64_t omega_batch_stride, int32_t count, rc_matrix y, int64_t y_batch_stride, rc_matrix q, int64_t q_batch_stride, rc_matrix p, int64_t p_batch_stride, int64_t *ranks, int32_t p_conj);
/* The certificate of such a batch: the Frobenius norm of what a low-rank factorization leaves of its block, in one stream-ordered, capturable call
 * that reads the ranks on the device: per block the reference's rel_diff_fro(x.to_mat(), a) (src/lib.rs) without the m x n temporary of to_mat, on
 * the domain of the sketched column ID, so the output of every batched compressor above is accepted.  The _c64 / _c32 forms take interleaved
 * (re, im) views with strides and batch strides in complex elements; s, err and nrm stay of the real type and nothing is conjugated, as in
 * rc_lowrank_apply_batched_c* (vt is already V^H, the two-sided c already Z2^H).
 * Operands.  The factor operands are exactly those of rc_lowrank_apply_batched_*: left (m x K), mid (K x K; mid.data == NULL: none), s (row i =
 * s + i * s_stride, at least K reals; NULL: none), right (K x n), ranks (count device values; NULL: every rank is K).  a is m x n.  Block i of
 * every operand is its view moved by i times its batch stride; a batch stride of 0 is legal for every input; any row and column strides; every
 * pointer a device pointer.
 * Per block (absent factors omitted), with r = ranks[i] clamped to [0, K] and Ah_i = left_i[:, :r] mid_i[:r, :r] diag(s_i[:r]) right_i[:r, :]:
 *   err[i] = ||a_i - Ah_i||_F;
 *   nrm[i] = ||a_i||_F; nrm == NULL: not written;
 *   e_i = a_i - Ah_i (m x n) when e.data != NULL; e.data == NULL: not written, the other fields of e are then ignored.
 * err and nrm are contiguous and of the real type of the call; e must not overlap any input.
 * Reads.  Elements of left, mid, s and right at an index >= r are never read: they may hold anything, NaN included, so the result does not rely
 * on the zero tails the batched calls write.
 * Arithmetic.  An element of Ah is the sum over ascending l, from zero, of left[i, l] W[l, j], four terms per v_mfma_f64_16x16x4_f64 /
 * v_mfma_f32_16x16x4_f32 (exact f32, no reduced precision).  W = right itself when there is neither mid nor s; otherwise
 * W = mid[:r, :r] (diag(s[:r]) right[:r, :]) with diag(s) right rounded once per element and the mid product summed in ascending inner index by
 * plain FMAs.  The residual element is a - Ah, one rounding.  Squares of e and of a are accumulated in f64 for both types, in a fixed order that
 * depends on (m, n) alone, and the root is rounded to the output type.  Scaling, f64 / c64: the three accumulators of LAPACK 3.10's ?lassq.  A
 * component of magnitude in [2^-511, 2^486) is squared as it stands, a larger one times 2^-538, a smaller one times 2^537; the three sums run
 * apart in the same fixed order and are combined once per block, so neither err nor nrm overflows or vanishes while the norm itself is a normal
 * number, and a block with every component in the middle range keeps the bits of the single sum.  A block that straddles a threshold is summed
 * in another grouping than its scaled copy: err and nrm of 2^e a are 2^e times those of a to rounding, not bit for bit.  f32 / c32: the single f64
 * sum, which the square of an f32 component (2^-298 .. 2^256) cannot leave.  e is unaffected.
 * Complex arithmetic.  The same MFMAs on the real and imaginary parts as separate real operands: per element each of Re Ah and Im Ah is one
 * accumulator chain from zero over ascending l, four terms per instruction, and within a step of four the Re chain takes the products
 * Re(left) Re(W), then (-Im(left)) Im(W), the Im chain Re(left) Im(W), then Im(left) Re(W); the negation is exact.  diag(s) right is one rounding
 * per component; the mid product is summed over ascending p from zero by plain FMAs, the four real products of a term in the order
 * re += Re(mid) Re(W0), re += (-Im(mid)) Im(W0), im += Re(mid) Im(W0), im += Im(mid) Re(W0).  Each component of e is one rounding; the squares of
 * Re e, Im e (Re a, Im a) enter the f64 sums element by element, re before im.  Hence: conjugating every complex operand leaves err and nrm
 * bit for bit and conjugates e bit for bit (up to the sign of an exactly cancelled zero); operands whose imaginary parts are all +0 give Re e equal
 * to the real call's e on the real parts and Im e = 0; the exact zeros of a column ID's kept columns hold as in the real call.
 * Consequences.  With r = 0, err[i] and nrm[i] are the same bits and e_i = a_i bit for bit.  For column-ID factors (no mid, no s) column
 * col_ind[j], j < r, of e is exactly zero: a unit column of z rebuilds the column of c exactly.  Block i's bits depend on block i's operands
 * and the call's shapes alone: not on count, the position in the batch, the neighbours, any batch, row or column stride, the grid, whether e or
 * nrm is requested, or graph replay against an eager call.  Non-finite input stays inside its block's err, nrm and e.
 * Domain: 1 <= m <= 65536, 1 <= n <= 512, 1 <= K <= 128, count >= 0 (0: nothing to do).  RC_INVALID_ARGUMENT for an argument outside the domain,
 * inconsistent shapes (left.rows != a.rows, left.cols != right.rows, right.cols != a.cols, mid not K x K, e not m x n), an e batch stride smaller
 * than one view's span when count > 1, a null a, left, right or err with count > 0, or a null ctx (rejected before a device is touched).  No host
 * synchronisation; workspace bounded by the grid, not by count. */
rc_status rc_lowrank_residual_batched_f64(rc_context *ctx, rc_matrix a, int64_t a_batch_stride, rc_matrix left, int64_t left_batch_stride, rc_matrix mid, int64_t mid_batch_stride, const double *s, int64_t s_stride, rc_matrix right, int64_t right_batch_stride, const int64_t *ranks, int32_t count, rc_matrix e, int64_t e_batch_stride, double *err, double *nrm);
rc_status rc_lowrank_residual_batched_f32(rc_context *ctx, rc_matrix a, int64_t a_batch_stride, rc_matrix left, int64_t left_batch_stride, rc_matrix mid, int64_t mid_batch_stride, const float *s, int64_t s_stride, rc_matrix right, int64_t right_batch_stride, const int64_t *ranks, int32_t count, rc_matrix e, int64_t e_batch_stride, float *err, float *nrm);
rc_status rc_lowrank_residual_batched_c64(rc_context *ctx, rc_matrix a, int64_t a_batch_stride, rc_matrix left, int64_t left_batch_stride, rc_matrix mid, int64_t mid_batch_stride, const double *s, int64_t s_stride, rc_matrix right, int64_t right_batch_stride, const int64_t *ranks, int32_t count, rc_matrix e, int64_t e_batch_stride, double *err, double *nrm);
rc_status rc_lowrank_residual_batched_c32(rc_context *ctx, rc_matrix a, int64_t a_batch_stride, rc_matrix left, int64_t left_batch_stride, rc_matrix mid, int64_t mid_batch_stride, const float *s, int64_t s_stride, rc_matrix right, int64_t right_batch_stride, const int64_t *ranks, int32_t count, rc_matrix e, int64_t e_batch_stride, float *err, float *nrm);
/* Apply the block-sparse operator such a batch describes, y = H x, in one stream-ordered, capturable call: the blocks of H are the low-rank
 * factors of a batch (the operands of rc_lowrank_apply_batched_*, unchanged) and, optionally, a batch of dense near-field blocks of the same
 * m x n shape, placed by a block-CSR pattern that lives on the device.  It is what the reference's MatMat / ConjMatMat (src/types.rs:40-101)
 * are for a hierarchical (BLR, H-matrix, FMM) operator whose blocks the batched calls above compressed; the gather of x, the apply and the
 * scatter-add into y happen in one launch, without atomics on y and without a workspace.
 * Layout.  Block ids are unified: id < count is low-rank block id (left, mid, s, right and ranks exactly as in rc_lowrank_apply_batched_*,
 * each view moved by id times its batch stride, 0 legal); count <= id < count + dense_count is block id - count of dense (m x n, moved by
 * dense_batch_stride; dense.data == NULL: there are none and dense_count is ignored).  Group g owns rows group_row[g] .. group_row[g] + m - 1
 * of y and consists of the entries group_ptr[g] .. group_ptr[g + 1] - 1, in that order; entry e contributes block entry_block[e] applied to
 * rows entry_col[e] .. entry_col[e] + n - 1 of x.  group_ptr (groups + 1 values, non-decreasing, indexing entry_block and entry_col, whose
 * length is not passed: that they cover group_ptr[groups] entries is the caller's contract), group_row (groups), entry_block and entry_col are
 * device int64 arrays.  x is N x nrhs and y is M x nrhs with any strides; y must not overlap an input.  A block may appear in several
 * entries and groups, and the x ranges of entries may overlap freely.  The row ranges of two groups must not overlap: if they do, which
 * group's values those rows hold is unspecified and nothing else is affected.  Rows of y that belong to no group are not touched.
 * Arithmetic.  Per group and column of x: acc starts at +0; every entry adds its contribution in list order, one rounding per add; the
 * group's rows of y receive acc, or y_old + acc (one more rounding) when accumulate != 0.  An empty group writes zeros, or leaves y_old when
 * accumulating.  The contribution of a low-rank entry is, bit for bit, what rc_lowrank_apply_batched_* writes for that block with
 * b = x[entry_col : entry_col + n, :]: r = ranks[id] clamped to [0, K], nothing at an index >= r is read, r = 0 contributes nothing.  The
 * contribution of a dense entry is sum_j D[i, j] x[col + j, c] in the summation order of the apply's last product at inner extent n, so for
 * n <= 128 it equals the low-rank contribution of left = D, right = I_n bit for bit.
 * conj != 0 (complex types; ignored for f64 / f32): every element of left, mid, right and dense is conjugated as it is loaded; s is real and
 * x is untouched.  With the transposed views (left = right^T, right = left^T, mid^T, dense^T as strided views) and the pattern grouped by
 * column instead of by row this is A^H x.  (mid and s together do not transpose into this chain: (L M diag(s) R)^T = R^T diag(s) M^T L^T.)
 * Bits.  The bits of a group's rows depend on its entries' operands in order, the rows of x they read, which stride of each view is the
 * smaller, and the block shape: not on groups, the group's position, the other groups, nrhs or the column tile (column c of a 17-column x
 * equals the same column applied alone), any batch stride, the grid, or graph replay against an eager call.  Non-finite values stay inside the
 * groups that reference them.
 * Indices are checked on the device: an entry whose block id is outside [0, count + dense_count) or whose entry_col is outside [0, N - n] is
 * skipped, a group whose group_row is outside [0, M - m] (or whose group_ptr pair starts below 0) writes nothing, and either case ORs bit 64
 * into the health word; every other group is unaffected.
 * Domain: 1 <= m, n <= 512, 1 <= K <= 128, nrhs >= 1, count, dense_count, groups >= 0 (groups == 0: nothing to do).  m, n (and K) are those of
 * left and right when count > 0 or left.data != NULL, else those of dense.  RC_INVALID_ARGUMENT for an argument outside the domain,
 * inconsistent shapes (left.cols != right.rows, mid not K x K, dense not m x n, x.cols != y.cols), neither a low-rank nor a dense batch with
 * groups > 0, a null left or right with count > 0, a null index array, x or y with groups > 0, or a null ctx (rejected before a device is
 * touched).  No host synchronisation, no workspace: a work unit is (group, tile of columns), its m x tile accumulator stays on the chip and y
 * is written once.  Parallelism is therefore groups x tiles: an operator with fewer block rows than the device holds workgroups does not fill
 * it at nrhs = 1 (splitting a group would need a workspace that grows with the entry count).
 * Complex scalars (c64, c32): interleaved (re, im) data, strides and batch strides in complex elements; s has the real type. */
rc_status rc_block_operator_apply_f64(rc_context *ctx, rc_matrix left, int64_t left_batch_stride, rc_matrix mid, int64_t mid_batch_stride, const double *s, int64_t s_stride, rc_matrix right, int64_t right_batch_stride, const int64_t *ranks, int32_t count, rc_matrix dense, int64_t dense_batch_stride, int32_t dense_count, const int64_t *group_ptr, const int64_t *group_row, int32_t groups, const int64_t *entry_block, const int64_t *entry_col, rc_matrix x, rc_matrix y, int32_t accumulate, int32_t conj);
rc_status rc_block_operator_apply_f32(rc_context *ctx, rc_matrix left, int64_t left_batch_stride, rc_matrix mid, int64_t mid_batch_stride, const float *s, int64_t s_stride, rc_matrix right, int64_t right_batch_stride, const int64_t *ranks, int32_t count, rc_matrix dense, int64_t dense_batch_stride, int32_t dense_count, const int64_t *group_ptr, const int64_t *group_row, int32_t groups, const int64_t *entry_block, const int64_t *entry_col, rc_matrix x, rc_matrix y, int32_t accumulate, int32_t conj);
rc_status rc_block_operator_apply_c64(rc_context *ctx, rc_matrix left, int64_t left_batch_stride, rc_matrix mid, int64_t mid_batch_stride, const double *s, int64_t s_stride, rc_matrix right, int64_t right_batch_stride, const int64_t *ranks, int32_t count, rc_matrix dense, int64_t dense_batch_stride, int32_t dense_count, const int64_t *group_ptr, const int64_t *group_row, int32_t groups, const int64_t *entry_block, const int64_t *entry_col, rc_matrix x, rc_matrix y, int32_t accumulate, int32_t conj);
rc_status rc_block_operator_apply_c32(rc_context *ctx, rc_matrix left, int64_t left_batch_stride, rc_matrix mid, int64_t mid_batch_stride, const float *s, int64_t s_stride, rc_matrix right, int64_t right_batch_stride, const int64_t *ranks, int32_t count, rc_matrix dense, int64_t dense_batch_stride, int32_t dense_count, const int64_t *group_ptr, const int64_t *group_row, int32_t groups, const int64_t *entry_block, const int64_t *entry_col, rc_matrix x, rc_matrix y, int32_t accumulate, int32_t conj);
/* Mixed-precision storage of a compressed batch: the factors in f32 (c32 for complex blocks), everything else in f64 (c64).  Factors that were
 * produced to a tolerance of 1e-6 carry no more than 24 bits of information; storing them in the narrow type halves the footprint of the compressed
 * operator and the bytes its matvec moves, while the vectors, the accumulation and the dense near-field blocks keep full precision.  Below, S is
 * the storage type and T the compute type: (T, S) = (f64, f32) for the _f64 calls and (c64, c32) for the _c64 calls.
 *
 * rc_lowrank_apply_mixed_batched_f64 / _c64 take the arguments of rc_lowrank_apply_batched_f64 / _c64, with left, mid and right views of S data
 * (their strides and batch strides count elements of S); s stays double, b and y are T, ranks is unchanged.
 * rc_block_operator_apply_mixed_f64 / _c64 take the arguments of rc_block_operator_apply_f64 / _c64, with left, mid and right of S; dense, x, y
 * are T and s double: near-field blocks stay in full precision.
 * Contract.  Every stored element is widened exactly to T as it is loaded (f32 -> f64 is exact; a complex element widens componentwise, and conj
 * is applied after widening); everything else is the twin's arithmetic in the twin's order.  The result is, bit for bit, what
 * rc_lowrank_apply_batched_T / rc_block_operator_apply_T writes for the same call on promoted copies of the factors (rc_promote_batched_*).
 * Hence every clause of the twins carries over unchanged: nothing at an index >= r is read; block i's (a group's) bits do not depend on count, the
 * neighbours, any batch stride, the column tile, the grid, or graph replay against an eager call; the accumulate and conj flags; health bit 64
 * for an out-of-range index; the domains 1 <= m, n <= 512, 1 <= K <= 128, nrhs >= 1; the argument checks, their status codes and messages.
 * Consequence.  Switching a batch from T to S storage changes the result only through the rounding of the stored factors: elementwise by at most
 * q u32 (1 + 2 u32) E, where q is the number of demoted factors in the chain (2, or 3 with mid), u32 = 2^-24 and
 * E = |left| |mid| diag(|s|) |right| |b| taken to the rank ((1 + u)^q - 1 <= q u (1 + 2 u) for q <= 3), provided no factor element overflowed or
 * fell into the f32 subnormal range when it was demoted. */
rc_status rc_lowrank_apply_mixed_batched_f64(rc_context *ctx, rc_matrix left, int64_t left_batch_stride, rc_matrix mid, int64_t mid_batch_stride, const double *s, int64_t s_stride, rc_matrix right, int64_t right_batch_stride, const int64_t *ranks, int32_t count, rc_matrix b, int64_t b_batch_stride, rc_matrix y, int64_t y_batch_stride);
rc_status rc_lowrank_apply_mixed_batched_c64(rc_context *ctx, rc_matrix left, int64_t left_batch_stride, rc_matrix mid, int64_t mid_batch_stride, const double *s, int64_t s_stride, rc_matrix right, int64_t right_batch_stride, const int64_t *ranks, int32_t count, rc_matrix b, int64_t b_batch_stride, rc_matrix y, int64_t y_batch_stride);
rc_status rc_block_operator_apply_mixed_f64(rc_context *ctx, rc_matrix left, int64_t left_batch_stride, rc_matrix mid, int64_t mid_batch_stride, const double *s, int64_t s_stride, rc_matrix right, int64_t right_batch_stride, const int64_t *ranks, int32_t count, rc_matrix dense, int64_t dense_batch_stride, int32_t dense_count, const int64_t *group_ptr, const int64_t *group_row, int32_t groups, const int64_t *entry_block, const int64_t *entry_col, rc_matrix x, rc_matrix y, int32_t accumulate, int32_t conj);
rc_status rc_block_operator_apply_mixed_c64(rc_context *ctx, rc_matrix left, int64_t left_batch_stride, rc_matrix mid, int64_t mid_batch_stride, const double *s, int64_t s_stride, rc_matrix right, int64_t right_batch_stride, const int64_t *ranks, int32_t count, rc_matrix dense, int64_t dense_batch_stride, int32_t dense_count, const int64_t *group_ptr, const int64_t *group_row, int32_t groups, const int64_t *entry_block, const int64_t *entry_col, rc_matrix x, rc_matrix y, int32_t accumulate, int32_t conj);
/* Strided batched conversion between the two types, so that a C, C++ or Rust host can move a factor batch in one stream-ordered, capturable
 * call: rc_demote_batched_f64 / _c64 convert T -> S (src is f64 / c64, dst f32 / c32), rc_promote_batched_f32 / _c32 convert S -> T (src is
 * f32 / c32, dst f64 / c64).  Block i is src moved by i * src_batch_stride and dst moved by i * dst_batch_stride, each in elements of its own
 * type; src and dst have the same rows x cols and any row and column strides; dst must not overlap src.  Demotion is IEEE round-to-nearest-even
 * per (real or imaginary) component, the bits of NumPy's astype(float32): results that are f32 subnormals, +-0, and finite values beyond the f32
 * range, which become +-inf, included; NaN stays NaN (payload unspecified).  overflow may be NULL; otherwise it holds count device int64 values and
 * overflow[i] receives the number of finite source elements of block i whose image is not finite (a complex element is finite when both parts
 * are); the call writes the value, it does not add to it, and the value is deterministic.  Promotion is exact.  Domain: 1 <= rows, cols <= 65536
 * (the tall c of the sketched ID included), count >= 0 (0: nothing to do).  RC_INVALID_ARGUMENT for an argument outside the domain, dst not of
 * src's shape, a dst batch stride smaller than one view's span when count > 1, a null src or dst with count > 0, or a null ctx.  No host
 * synchronisation, no workspace. */
rc_status rc_demote_batched_f64(rc_context *ctx, rc_matrix src, int64_t src_batch_stride, int32_t count, rc_matrix dst, int64_t dst_batch_stride, int64_t *overflow);
rc_status rc_demote_batched_c64(rc_context *ctx, rc_matrix src, int64_t src_batch_stride, int32_t count, rc_matrix dst, int64_t dst_batch_stride, int64_t *overflow);
rc_status rc_promote_batched_f32(rc_context *ctx, rc_matrix src, int64_t src_batch_stride, int32_t count, rc_matrix dst, int64_t dst_batch_stride);
rc_status rc_promote_batched_c32(rc_context *ctx, rc_matrix src, int64_t src_batch_stride, int32_t count, rc_matrix dst, int64_t dst_batch_stride);
/* Reserved: the _f32 members of the three stems above (every _f64 entry point of this header has an _f32 one).  They would be f32 arithmetic over
 * 16-bit storage, which this library does not build: each returns RC_INVALID_ARGUMENT for every call (and for a null ctx), with a message
 * that names the _f64 and _c64 calls, and touches no operand. */
rc_status rc_lowrank_apply_mixed_batched_f32(rc_context *ctx, rc_matrix left, int64_t left_batch_stride, rc_matrix mid, int64_t mid_batch_stride, const float *s, int64_t s_stride, rc_matrix right, int64_t right_batch_stride, const int64_t *ranks, int32_t count, rc_matrix b, int64_t b_batch_stride, rc_matrix y, int64_t y_batch_stride);
rc_status rc_block_operator_apply_mixed_f32(rc_context *ctx, rc_matrix left, int64_t left_batch_stride, rc_matrix mid, int64_t mid_batch_stride, const float *s, int64_t s_stride, rc_matrix right, int64_t right_batch_stride, const int64_t *ranks, int32_t count, rc_matrix dense, int64_t dense_batch_stride, int32_t dense_count, const int64_t *group_ptr, const int64_t *group_row, int32_t groups, const int64_t *entry_block, const int64_t *entry_col, rc_matrix x, rc_matrix y, int32_t accumulate, int32_t conj);
rc_status rc_demote_batched_f32(rc_context *ctx, rc_matrix src, int64_t src_batch_stride, int32_t count, rc_matrix dst, int64_t dst_batch_stride, int64_t *overflow);

/* The gather over RCCL (xGMI inside a node).  One process per GPU: rank 0 calls rc_comm_unique_id and hands the 128
 * bytes to the other ranks by whatever means the host has (MPI, a file, torch.distributed), every rank calls
 * rc_comm_init, then rc_comm_gather moves bytes_per_rank bytes from every rank's `send` into
 * recv[rank * bytes_per_rank ...] on `root` (grouped ncclSend / ncclRecv on the context's stream, asynchronous:
 * rc_synchronize(ctx) completes it).  librccl is opened at run time; RC_RUNTIME_ERROR if it is not available. */
typedef struct rc_comm rc_comm;
rc_status rc_comm_unique_id(void *id128);
rc_status rc_comm_init(rc_comm **comm, int32_t world, int32_t rank, const void *id128, int32_t device);
rc_status rc_comm_gather(rc_comm *comm, rc_context *ctx, const void *send, void *recv, size_t bytes_per_rank, int32_t root);
rc_status rc_comm_destroy(rc_comm *comm);
const char *rc_comm_last_error_message(const rc_comm *comm);
/* The two collectives of the row-sharded single-matrix path below (all ranks end with the same bits):
 *   rc_comm_all_gather      recv[r * bytes_per_rank ...] = rank r's send (send may be the rank's own block of recv)
 *   rc_comm_all_reduce_sum  buf[i] = sum over the ranks, in place; elem_size 8 = double, 4 = float
 * ordered on the context's stream (ncclAllGather / ncclAllReduce: asynchronous).  rc_comm_world reports the extent. */
rc_status rc_comm_all_gather(rc_comm *comm, rc_context *ctx, const void *send, void *recv, size_t bytes_per_rank);
rc_status rc_comm_all_reduce_sum(rc_comm *comm, rc_context *ctx, void *buf, size_t count, int32_t elem_size);
rc_status rc_comm_world(const rc_comm *comm, int32_t *world, int32_t *rank);
/* A communicator over the HOST's own communication layer (MPI, gloo, a test harness) instead of RCCL: the library stages
 * the (small) buffers of the two collectives above through host memory, waits for the stream and calls back.  Both
 * callbacks work on host pointers, return 0 on success, and must leave the same bytes on every rank.
 * rc_comm_gather is not available on such a communicator. */
typedef int32_t (*rc_host_all_gather_fn)(void *user, const void *send, void *recv, size_t bytes_per_rank);
typedef int32_t (*rc_host_all_reduce_sum_fn)(void *user, void *buf, size_t count, int32_t elem_size);
rc_status rc_comm_init_host(rc_comm **comm, int32_t world, int32_t rank, int32_t device, rc_host_all_gather_fn all_gather,
                            rc_host_all_reduce_sum_fn all_reduce_sum, void *user);

/* ----------------------------------------- one matrix sharded by rows over the GPUs -- */
/* The cfg3 pipeline (sample_range_by_rank -> SVD / QR::compute_from_range_estimate -> column_id, src/random_sampling.rs:103-118,
 * src/svd.rs:171-183, src/qr.rs:311-323, :270-309) for ONE matrix A = [A_0; ...; A_{W-1}] whose row block a_local
 * (m_r x n, m_r >= k + p) lives on this rank; the reference is single-process, so there is no file:line for the split.
 * Local: the sketch Y_r = A_r Omega (Omega = the Philox stream of `seed`, identical on every rank), its pivoted QR, every
 * product with A.  Exchanged: the l x l factor of every rank (all-gather; the pivoted QR of the stack gives THE pivoted
 * QR of Y, TSQR) and the k x n projection B (all-reduce).  out: range_q, u, qr_q, id_c have m_r rows (this rank's rows
 * of the global factors); s, vt, qr_r, qr_ind, id_z are replicated bit-identically.  "NULL = skipped" as in rc_rsvd_id.
 * comm == NULL: one rank.  Blocking where the transport is (host communicators); not capturable. */
rc_status rc_rsvd_id_row_sharded_f64(rc_comm *comm, rc_context *ctx, rc_matrix a_local, int64_t k, int64_t p, uint64_t seed, const rc_rsvd_id_out *out);
rc_status rc_rsvd_id_row_sharded_f32(rc_comm *comm, rc_context *ctx, rc_matrix a_local, int64_t k, int64_t p, uint64_t seed, const rc_rsvd_id_out *out);

/* ------------------------------------------------------------- complex scalars (c32 / c64) -- */
/* The reference instantiates every trait for f32, f64, c32 and c64 (macros at src/qr.rs:408-416, src/pivoted_qr.rs:187-190,
 * src/svd.rs:188-191, src/random_sampling.rs:123-126, :165-168, :277-280, src/types.rs:198-204).  Complex matrices are
 * interleaved (re, im) pairs -- the layout of ndarray's Complex<T> and of numpy complex arrays -- described by the same
 * rc_matrix (strides in complex elements).  Same semantics as the real entry points with A^H wherever they have A^T:
 * conj_matmat is A^H X (src/types.rs:128-132), Q has orthonormal columns in the complex inner product, singular values
 * and norms are real (float / double arguments below), R has a real diagonal (?geqp3), permutation indices as before.
 * rc_gemm_*: trans = 0 none, 1 transpose, 2 conjugate transpose; complex alpha / beta with the real entry points' BLAS contract
 * (beta = 0 never reads C, K = 0 gives C = beta * C).  rc_random_gaussian_*: element (i, j) takes normals
 * 2 (offset + i cols + j) (real part) and the next one (imaginary part) of the Philox stream, the order the reference
 * draws them in (src/random_matrix.rs:136-143).  rc_rsvd_id_c* / rc_batch_column_id_c* are compositions of the calls below with
 * the real entry points' members, layout and "null = skipped" rule (B = Q^H A formed once; not the tuned real hot path);
 * rc_svd_rank_by_tolerance_c* forwards to the real call (singular values are real). */
typedef struct rc_complex32 { float re, im; } rc_complex32;
typedef struct rc_complex64 { double re, im; } rc_complex64;
rc_status rc_random_gaussian_c64(rc_context *ctx, rc_matrix out, uint64_t seed, uint64_t offset);
rc_status rc_matmat_c64(rc_context *ctx, rc_matrix a, rc_matrix x, rc_matrix y);
rc_status rc_conj_matmat_c64(rc_context *ctx, rc_matrix a, rc_matrix x, rc_matrix y);
rc_status rc_gemm_c64(rc_context *ctx, int32_t trans_a, int32_t trans_b, rc_complex64 alpha, rc_matrix a, rc_matrix b, rc_complex64 beta, rc_matrix c);
rc_status rc_rel_diff_fro_c64(rc_context *ctx, rc_matrix first, rc_matrix second, double *out);
rc_status rc_apply_permutation_matrix_c64(rc_context *ctx, int32_t mode, rc_matrix in, const int64_t *perm, int64_t perm_len, rc_matrix out);
rc_status rc_apply_permutation_vector_c64(rc_context *ctx, int32_t mode, rc_matrix in, const int64_t *perm, int64_t perm_len, rc_matrix out);
rc_status rc_pivoted_qr_c64(rc_context *ctx, rc_matrix a, rc_matrix q, rc_matrix r, int64_t *ind);
rc_status rc_pivoted_lq_c64(rc_context *ctx, rc_matrix a, rc_matrix l, rc_matrix q, int64_t *ind);
rc_status rc_geqp3_c64(rc_context *ctx, rc_matrix a, int64_t kmax, int64_t *jpvt, rc_complex64 *tau);   /* ?geqp3, LAPACK format (see rc_geqp3_f64) */
rc_status rc_orgqr_c64(rc_context *ctx, rc_matrix a, const rc_complex64 *tau, int64_t k, rc_matrix q);   /* ?ungqr */
rc_status rc_trsm_upper_c64(rc_context *ctx, rc_matrix t, rc_matrix b);
rc_status rc_compute_svd_c64(rc_context *ctx, rc_matrix a, rc_matrix u, double *s, rc_matrix vt);
rc_status rc_rank_by_tolerance_c64(rc_context *ctx, rc_matrix tri, double tol, int64_t *rank);
rc_status rc_qr_to_mat_c64(rc_context *ctx, rc_matrix q, rc_matrix r, const int64_t *ind, rc_matrix out);
rc_status rc_lq_to_mat_c64(rc_context *ctx, rc_matrix l, rc_matrix q, const int64_t *ind, rc_matrix out);
rc_status rc_qr_column_id_c64(rc_context *ctx, rc_matrix q, rc_matrix r, const int64_t *ind, rc_matrix c, rc_matrix z);
rc_status rc_lq_row_id_c64(rc_context *ctx, rc_matrix l, rc_matrix q, const int64_t *ind, rc_matrix x, rc_matrix r_rows);
rc_status rc_qr_from_range_estimate_c64(rc_context *ctx, rc_matrix range, rc_matrix a, rc_matrix q, rc_matrix r, int64_t *ind);
rc_status rc_svd_to_mat_c64(rc_context *ctx, rc_matrix u, const double *s, rc_matrix vt, rc_matrix out);
rc_status rc_svd_to_qr_c64(rc_context *ctx, rc_matrix u, const double *s, rc_matrix vt, rc_matrix q, rc_matrix r, int64_t *ind);
rc_status rc_svd_from_range_estimate_c64(rc_context *ctx, rc_matrix range, rc_matrix a, rc_matrix u, double *s, rc_matrix vt);
rc_status rc_column_id_two_sided_c64(rc_context *ctx, rc_matrix c, rc_matrix c_out, rc_matrix x, int64_t *row_ind);
rc_status rc_row_id_two_sided_c64(rc_context *ctx, rc_matrix r, rc_matrix x, rc_matrix r_out, int64_t *col_ind);
rc_status rc_max_col_norm_c64(rc_context *ctx, rc_matrix y, double *out);
rc_status rc_sample_range_by_rank_c64(rc_context *ctx, rc_matrix a, int64_t k, int64_t p, rc_matrix omega, uint64_t seed, rc_matrix q);
/* the operator-callback entry points (rc_operator, above) for c64: views are interleaved complex, strides in complex elements */
rc_status rc_sample_range_by_rank_op_c64(rc_context *ctx, const rc_operator *op, int64_t k, int64_t p, rc_matrix omega, uint64_t seed, rc_matrix q);
rc_status rc_sample_range_power_iteration_op_c64(rc_context *ctx, const rc_operator *op, int64_t k, int64_t p, int64_t it_count, rc_matrix omega, uint64_t seed, rc_matrix q);
rc_status rc_sample_range_adaptive_op_c64(rc_context *ctx, const rc_operator *op, double rel_tol, int64_t sample_size, rc_matrix omegas, uint64_t seed, rc_matrix q_cap, int64_t *rank, int64_t *hist_rank, double *hist_res, int64_t hist_cap, int64_t *hist_len);
rc_status rc_qr_from_range_estimate_op_c64(rc_context *ctx, rc_matrix range, const rc_operator *op, rc_matrix q, rc_matrix r, int64_t *ind);
rc_status rc_svd_from_range_estimate_op_c64(rc_context *ctx, rc_matrix range, const rc_operator *op, rc_matrix u, double *s, rc_matrix vt);
rc_status rc_sample_range_power_iteration_c64(rc_context *ctx, rc_matrix a, int64_t k, int64_t p, int64_t it_count, rc_matrix omega, uint64_t seed, rc_matrix q);
rc_status rc_sample_range_adaptive_c64(rc_context *ctx, rc_matrix a, double rel_tol, int64_t sample_size, rc_matrix omegas, uint64_t seed, rc_matrix q_cap, int64_t *rank, int64_t *hist_rank, double *hist_res, int64_t hist_cap, int64_t *hist_len);
rc_status rc_column_id_rank_c64(rc_context *ctx, rc_matrix a, int64_t k, rc_matrix c, rc_matrix z, int64_t *col_ind);
rc_status rc_svd_rank_by_tolerance_c64(rc_context *ctx, const double *s, int64_t len, double tol, int64_t *rank);
rc_status rc_rsvd_id_c64(rc_context *ctx, rc_matrix a, int64_t k, int64_t p, rc_matrix omega, uint64_t seed, const rc_rsvd_id_out *out);
rc_status rc_batch_column_id_c64(rc_context *const *ctxs, int32_t nctx, const rc_matrix *mats, int32_t count, int64_t k, void *packed);
rc_status rc_random_gaussian_c32(rc_context *ctx, rc_matrix out, uint64_t seed, uint64_t offset);
rc_status rc_matmat_c32(rc_context *ctx, rc_matrix a, rc_matrix x, rc_matrix y);
rc_status rc_conj_matmat_c32(rc_context *ctx, rc_matrix a, rc_matrix x, rc_matrix y);
rc_status rc_gemm_c32(rc_context *ctx, int32_t trans_a, int32_t trans_b, rc_complex32 alpha, rc_matrix a, rc_matrix b, rc_complex32 beta, rc_matrix c);
rc_status rc_rel_diff_fro_c32(rc_context *ctx, rc_matrix first, rc_matrix second, float *out);
rc_status rc_apply_permutation_matrix_c32(rc_context *ctx, int32_t mode, rc_matrix in, const int64_t *perm, int64_t perm_len, rc_matrix out);
rc_status rc_apply_permutation_vector_c32(rc_context *ctx, int32_t mode, rc_matrix in, const int64_t *perm, int64_t perm_len, rc_matrix out);
rc_status rc_pivoted_qr_c32(rc_context *ctx, rc_matrix a, rc_matrix q, rc_matrix r, int64_t *ind);
rc_status rc_pivoted_lq_c32(rc_context *ctx, rc_matrix a, rc_matrix l, rc_matrix q, int64_t *ind);
rc_status rc_geqp3_c32(rc_context *ctx, rc_matrix a, int64_t kmax, int64_t *jpvt, rc_complex32 *tau);   /* ?geqp3, LAPACK format (see rc_geqp3_f64) */
rc_status rc_orgqr_c32(rc_context *ctx, rc_matrix a, const rc_complex32 *tau, int64_t k, rc_matrix q);   /* ?ungqr */
rc_status rc_trsm_upper_c32(rc_context *ctx, rc_matrix t, rc_matrix b);
rc_status rc_compute_svd_c32(rc_context *ctx, rc_matrix a, rc_matrix u, float *s, rc_matrix vt);
rc_status rc_rank_by_tolerance_c32(rc_context *ctx, rc_matrix tri, double tol, int64_t *rank);
rc_status rc_qr_to_mat_c32(rc_context *ctx, rc_matrix q, rc_matrix r, const int64_t *ind, rc_matrix out);
rc_status rc_lq_to_mat_c32(rc_context *ctx, rc_matrix l, rc_matrix q, const int64_t *ind, rc_matrix out);
rc_status rc_qr_column_id_c32(rc_context *ctx, rc_matrix q, rc_matrix r, const int64_t *ind, rc_matrix c, rc_matrix z);
rc_status rc_lq_row_id_c32(rc_context *ctx, rc_matrix l, rc_matrix q, const int64_t *ind, rc_matrix x, rc_matrix r_rows);
rc_status rc_qr_from_range_estimate_c32(rc_context *ctx, rc_matrix range, rc_matrix a, rc_matrix q, rc_matrix r, int64_t *ind);
rc_status rc_svd_to_mat_c32(rc_context *ctx, rc_matrix u, const float *s, rc_matrix vt, rc_matrix out);
rc_status rc_svd_to_qr_c32(rc_context *ctx, rc_matrix u, const float *s, rc_matrix vt, rc_matrix q, rc_matrix r, int64_t *ind);
rc_status rc_svd_from_range_estimate_c32(rc_context *ctx, rc_matrix range, rc_matrix a, rc_matrix u, float *s, rc_matrix vt);
rc_status rc_column_id_two_sided_c32(rc_context *ctx, rc_matrix c, rc_matrix c_out, rc_matrix x, int64_t *row_ind);
rc_status rc_row_id_two_sided_c32(rc_context *ctx, rc_matrix r, rc_matrix x, rc_matrix r_out, int64_t *col_ind);
rc_status rc_max_col_norm_c32(rc_context *ctx, rc_matrix y, float *out);
rc_status rc_sample_range_by_rank_c32(rc_context *ctx, rc_matrix a, int64_t k, int64_t p, rc_matrix omega, uint64_t seed, rc_matrix q);
rc_status rc_sample_range_by_rank_op_c32(rc_context *ctx, const rc_operator *op, int64_t k, int64_t p, rc_matrix omega, uint64_t seed, rc_matrix q);
rc_status rc_sample_range_power_iteration_op_c32(rc_context *ctx, const rc_operator *op, int64_t k, int64_t p, int64_t it_count, rc_matrix omega, uint64_t seed, rc_matrix q);
rc_status rc_sample_range_adaptive_op_c32(rc_context *ctx, const rc_operator *op, double rel_tol, int64_t sample_size, rc_matrix omegas, uint64_t seed, rc_matrix q_cap, int64_t *rank, int64_t *hist_rank, double *hist_res, int64_t hist_cap, int64_t *hist_len);
rc_status rc_qr_from_range_estimate_op_c32(rc_context *ctx, rc_matrix range, const rc_operator *op, rc_matrix q, rc_matrix r, int64_t *ind);
rc_status rc_svd_from_range_estimate_op_c32(rc_context *ctx, rc_matrix range, const rc_operator *op, rc_matrix u, float *s, rc_matrix vt);
rc_status rc_sample_range_power_iteration_c32(rc_context *ctx, rc_matrix a, int64_t k, int64_t p, int64_t it_count, rc_matrix omega, uint64_t seed, rc_matrix q);
rc_status rc_sample_range_adaptive_c32(rc_context *ctx, rc_matrix a, double rel_tol, int64_t sample_size, rc_matrix omegas, uint64_t seed, rc_matrix q_cap, int64_t *rank, int64_t *hist_rank, double *hist_res, int64_t hist_cap, int64_t *hist_len);
rc_status rc_column_id_rank_c32(rc_context *ctx, rc_matrix a, int64_t k, rc_matrix c, rc_matrix z, int64_t *col_ind);
rc_status rc_svd_rank_by_tolerance_c32(rc_context *ctx, const float *s, int64_t len, double tol, int64_t *rank);
rc_status rc_rsvd_id_c32(rc_context *ctx, rc_matrix a, int64_t k, int64_t p, rc_matrix omega, uint64_t seed, const rc_rsvd_id_out *out);
rc_status rc_batch_column_id_c32(rc_context *const *ctxs, int32_t nctx, const rc_matrix *mats, int32_t count, int64_t k, void *packed);

#ifdef __cplusplus
}
#endif
#endif /* RUSTY_COMPRESSION_AMD_H */
