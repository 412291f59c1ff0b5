"""rusty_compression_amd -- MI355X-native randomized low-rank compression.

Host-side mirror of the public surface of the Rust crate `rusty-compression`
v0.1.1 (reference src/lib.rs:90-102) over the C ABI of
librusty_compression_amd.so (include/rusty_compression_amd.h).  Only the hot
path is here: Gaussian sketch -> column-pivoted QR (+ permutation) -> small SVD /
column, row and two-sided interpolative decompositions.
"""
from ._lib import (CompressionError, Context, HipRuntimeError, LayoutError, LinalgError, PivotedQRError,  # noqa: F401
                   RustyCompressionError, default_context)
from .batch import column_id_rank_batched, svd_rank_batched, svd_rank_batched_complex, two_sided_id_rank_batched  # noqa: F401
from .batch import column_id_apply_batched, lowrank_apply_batched, svd_apply_batched, two_sided_id_apply_batched  # noqa: F401
from .batch import column_id_to_svd_batched, lowrank_recompress_batched, svd_add_batched, two_sided_id_to_svd_batched  # noqa: F401
from .batch import (column_id_to_svd_batched_complex, lowrank_recompress_batched_complex, svd_add_batched_complex,  # noqa: F401
                    two_sided_id_to_svd_batched_complex)
from .batch import column_id_to_svd_tall_batched, lowrank_recompress_tall_batched, sketch_svd_rank_batched, svd_add_tall_batched  # noqa: F401
from .batch import lowrank_recompress_large_batched, svd_add_large_batched  # noqa: F401
from .batch import lowrank_recompress_large_batched_complex, svd_add_large_batched_complex  # noqa: F401
from .batch import sketch_product_batched, sketch_range_step_large_batched, sketch_svd_rank_large_batched  # noqa: F401
from .batch import (column_id_to_svd_tall_batched_complex, lowrank_recompress_tall_batched_complex, sketch_svd_rank_batched_complex,  # noqa: F401
                    svd_add_tall_batched_complex)
from .batch import sketch_column_id_rank_batched  # noqa: F401
from .batch import sketch_column_id_rank_batched_complex  # noqa: F401
from .batch import (sketch_column_id_rank_power_batched, sketch_power_omega_batched, sketch_range_step_batched,  # noqa: F401
                    sketch_svd_rank_power_batched)
from .batch import (sketch_column_id_rank_power_batched_complex, sketch_power_omega_batched_complex,  # noqa: F401
                    sketch_range_step_batched_complex, sketch_svd_rank_power_batched_complex)
from .batch import block_csr, block_operator_apply  # noqa: F401
from .batch import block_operator_apply_mixed, demote_batched, lowrank_apply_batched_mixed, promote_batched  # noqa: F401
from .batch import column_id_residual_batched, lowrank_residual_batched, svd_residual_batched, two_sided_id_residual_batched  # noqa: F401
from .batch import (column_id_residual_batched_complex, lowrank_residual_batched_complex, svd_residual_batched_complex,  # noqa: F401
                    two_sided_id_residual_batched_complex)
from .col_interp_decomp import ColumnID  # noqa: F401
from .operator import BlockLowRankOperator, DenseOperator, LowRankOperator, MixedBlockLowRankOperator, Operator  # noqa: F401
from .permutation import (MatrixPermutationMode, VectorPermutationMode, apply_permutation,  # noqa: F401
                          invert_permutation_vector)
from .qr import LQ, QR, pivoted_lq, pivoted_qr  # noqa: F401
from .random_matrix import (Rng, random_approximate_low_rank_matrix, random_bits_u32, random_gaussian,  # noqa: F401
                            random_orthogonal_matrix)
from .random_sampling import (max_col_norm, sample_range_adaptive, sample_range_by_rank,  # noqa: F401
                              sample_range_power_iteration)
from .row_interp_decomp import RowID  # noqa: F401
from .svd import SVD, compute_svd  # noqa: F401
from .lapack import geqp3, orgqr, trsm_upper  # noqa: F401
from .two_sided_interp_decomp import TwoSidedID  # noqa: F401
from .types import CompressionType, conj_matmat, dot, matmat, rel_diff_fro, rel_diff_l2  # noqa: F401

__all__ = [
    "QR", "LQ", "SVD", "ColumnID", "RowID", "TwoSidedID", "CompressionType", "Rng",
    "MatrixPermutationMode", "VectorPermutationMode", "apply_permutation", "invert_permutation_vector",
    "random_gaussian", "random_bits_u32", "random_orthogonal_matrix", "random_approximate_low_rank_matrix",
    "sample_range_by_rank", "sample_range_power_iteration", "sample_range_adaptive", "max_col_norm",
    "matmat", "conj_matmat", "dot", "rel_diff_fro", "rel_diff_l2", "pivoted_qr", "pivoted_lq", "compute_svd", "column_id_rank_batched", "two_sided_id_rank_batched", "svd_rank_batched", "svd_rank_batched_complex", "lowrank_apply_batched", "column_id_apply_batched", "two_sided_id_apply_batched", "svd_apply_batched", "lowrank_recompress_batched", "column_id_to_svd_batched", "two_sided_id_to_svd_batched", "svd_add_batched", "lowrank_recompress_batched_complex", "column_id_to_svd_batched_complex", "two_sided_id_to_svd_batched_complex", "svd_add_batched_complex", "lowrank_recompress_tall_batched", "column_id_to_svd_tall_batched", "svd_add_tall_batched", "lowrank_recompress_large_batched", "svd_add_large_batched", "lowrank_recompress_large_batched_complex", "svd_add_large_batched_complex", "sketch_svd_rank_batched", "lowrank_recompress_tall_batched_complex", "column_id_to_svd_tall_batched_complex", "svd_add_tall_batched_complex", "sketch_svd_rank_batched_complex", "sketch_column_id_rank_batched", "sketch_column_id_rank_batched_complex", "lowrank_residual_batched", "column_id_residual_batched", "two_sided_id_residual_batched", "svd_residual_batched", "lowrank_residual_batched_complex", "column_id_residual_batched_complex", "two_sided_id_residual_batched_complex", "svd_residual_batched_complex", "geqp3", "orgqr", "trsm_upper",
    "RustyCompressionError", "LinalgError", "CompressionError", "LayoutError", "PivotedQRError", "HipRuntimeError",
    "Context", "default_context", "Operator", "DenseOperator", "LowRankOperator", "BlockLowRankOperator",
    "block_csr", "block_operator_apply",
    "sketch_range_step_batched", "sketch_power_omega_batched", "sketch_column_id_rank_power_batched", "sketch_svd_rank_power_batched",
    "sketch_range_step_batched_complex", "sketch_power_omega_batched_complex", "sketch_column_id_rank_power_batched_complex",
    "sketch_svd_rank_power_batched_complex",
    "sketch_product_batched", "sketch_range_step_large_batched", "sketch_svd_rank_large_batched",
    "lowrank_apply_batched_mixed", "block_operator_apply_mixed", "demote_batched", "promote_batched", "MixedBlockLowRankOperator",
]
