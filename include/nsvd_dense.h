/*
 * nsvd_dense.h - C ABI of libnsvd_dense.so: the two-sided DENSE operator on index batches, both halves of an SVD step
 * on a stored matrix. A library of its own beside libnsvd_hip.so (built by the same Makefile from
 * csrc/kernel_apply_pair.hip alone; it shares headers with libnsvd_hip.so and no symbol): include/nsvd.h, its ctypes
 * table and libnsvd_hip.so's exports stay exactly the 102 entry points of ABI 6, and this file, _lib.DENSE_SIGNATURES
 * and libnsvd_dense.so's exports are held to the same three-way agreement (tests/test_dense_pair_oracle.py).
 * Conventions (device pointers, caller-owned workspace, `stream`, return codes) are nsvd.h's.
 *
 * out_x[i][l] = scale_g * sum_k A[rows[i]][cols[k]] g[k][l]   (B1, L)   "A g"
 * out_y[k][l] = scale_f * sum_i A[rows[i]][cols[k]] f[i][l]   (B2, L)   "A^T f"
 * - nsvd_kernel_apply's two-sided counterpart for a RECTANGULAR, non-symmetric matrix: the (Tg, Tadjf) producer of
 * NestedLoRALossFunctionSVD(f, Tg, g, Tadjf) (methods/nestedlora.py:100-156) when the operator is a matrix the caller
 * holds. A: (N1, lda) row-major float32, 16-byte aligned, lda >= N2 rounded up to 64 and lda % 4 == 0 (rows are read in
 * whole 64-float chunks; the column padding and any rows beyond N1 may hold anything finite) - nsvd_kernel_apply's
 * contract for K; no transposed copy is needed or made. rows (B1), cols (B2): int64 indices drawn with replacement
 * (duplicates are ordinary terms of the sums); g: (B2, L), f: (B1, L), out_x: (B1, L), out_y: (B2, L) float32 row-major.
 * rows[i] outside [0, N1): out_x[i] is a zero row and row i of f contributes nothing to out_y. cols[k] outside [0, N2):
 * out_y[k] is a zero row and row k of g contributes nothing to out_x. Any N1, N2, B1, B2, L >= 1. Every 64 x 64 block of
 * the gathered rows is brought on chip once per 64 heads and feeds both contractions on the fp32 MFMA; partial copies in
 * the workspace (at most 32 of either product) are added in a fixed order: no atomics, bit-reproducible, independent of
 * the stream. NSVD_EINVAL: a null pointer, a non-positive size, a bad lda or alignment, a workspace too small or not
 * 256-byte aligned; a refused call launches nothing and writes nothing. No allocation, no synchronisation. Index
 * arithmetic into A is 64-bit. Restated in float64 by tests/_dense_pair_oracle.py.
 * nsvd_kernel_apply_pair_partition (host only): row_groups runs of 64-row tiles of the batch (= partial copies of
 * A[rows, :]^T f) and col_groups runs of columns of A (= partial copies of out_x).
 */
#ifndef NSVD_DENSE_H
#define NSVD_DENSE_H
#include "nsvd.h"

#ifdef __cplusplus
extern "C" {
#endif

size_t nsvd_kernel_apply_pair_workspace_bytes(int N1, int N2, int B1, int B2, int L);
int nsvd_kernel_apply_pair_partition(int N1, int N2, int B1, int B2, int L, int* row_groups, int* col_groups);
int nsvd_kernel_apply_pair(const float* A, size_t lda, int N1, int N2, const long long* rows, int B1,
                           const long long* cols, int B2, const float* g, const float* f, int L, float scale_g,
                           float scale_f, float* out_x, float* out_y, void* ws, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* NSVD_DENSE_H */
