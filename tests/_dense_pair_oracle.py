"""Float64 restatement of nsvd_kernel_apply_pair (csrc/kernel_apply_pair.hip), numpy:

    out_x[i] = scale_g * sum_k A[rows[i]][cols[k]] g[k],        out_y[k] = scale_f * sum_i A[rows[i]][cols[k]] f[i]

with the rule for indices out of range: such a row (column) of the gathered block is zero - its output row is zero and
its row of f (of g) contributes nothing to the other product."""
import numpy as np


def gathered_block(A, N1, N2, rows, cols):
    """A[rows][:, cols] as float64 (B1, B2), rows outside [0, N1) and columns outside [0, N2) zeroed"""
    A = np.asarray(A, dtype=np.float64)
    rows, cols = np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64)
    okr, okc = (rows >= 0) & (rows < N1), (cols >= 0) & (cols < N2)
    blk = A[np.where(okr, rows, 0)][:, np.where(okc, cols, 0)]
    return blk * okr[:, None] * okc[None, :]


def dense_apply_pair(A, N1, N2, rows, cols, g, f, scale_g, scale_f):
    blk = gathered_block(A, N1, N2, rows, cols)
    return scale_g * (blk @ np.asarray(g, dtype=np.float64)), scale_f * (blk.T @ np.asarray(f, dtype=np.float64))
