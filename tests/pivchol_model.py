"""The numpy restatement of the diagonal-pivoted Cholesky contract (include/gsi_hip.h: gsi_op_pivoted_cholesky;
csrc/pchol_state.hpp).  Not a test module.

  d_i = A(i, i).  Before step j: trace_j = sum of max(d_i, 0); p = the lowest index attaining max d_i; stop, tested in this
  order, with reason 4 (non-finite), 3 (d_p is not > 0), 2 (trace_j <= tol trace_0), 1 (j == K).
  Step j: r = sqrt(d_p); s_i = 0, then for c = 0 .. j - 1 ascending s_i = s_i + L[i, c] L[p, c]; L[i, j] = (A(i, p) - s_i) / r;
  d_i = d_i - L[i, j] L[i, j]; then d_p = 0.

The loop over c is a Python loop of vector operations over the rows, so every product and every sum is rounded on its own
(numpy fuses nothing), and np.sqrt and the division are correctly rounded: the model's L is the contract's L bit for bit.
The trace is summed by np.sum (pairwise): the contract leaves its order free, and only the comparison with tol sees it.
"""
import numpy as np


def matrix_source(A):
    """(column, diag) of a dense symmetric matrix."""
    A = np.asarray(A, dtype=np.float64)
    return (lambda p: A[:, p]), np.diag(A).copy()


def table_source(table):
    """(column, diag) of the implicit grid covariance A(i, j) = table[|x_i - x_j|, |y_i - y_j|], i = (i // ny, i % ny)."""
    table = np.asarray(table, dtype=np.float64)
    nx, ny = table.shape
    ix, iy = np.divmod(np.arange(nx * ny), ny)
    return (lambda p: table[np.abs(ix - ix[p]), np.abs(iy - iy[p])]), np.full(nx * ny, table[0, 0])


def pivchol(column, diag, K, tol=0.0):
    """Returns a dict: L (n x K, Fortran order, zeros from column rank on), piv (rank entries), rank, reason, trace0, trace,
    dmax, d (the diagonal of A - L L' as the recurrence leaves it), gaps (per step: the relative gap between the two
    largest d, (d_1 - d_2) / d_1; empty for n = 1)."""
    d = np.array(diag, dtype=np.float64)
    n = d.size
    L = np.zeros((n, K), order="F")
    piv, gaps = [], []
    trace0 = trace = float(np.maximum(d, 0.0).sum())
    j = 0
    while True:
        trace = float(np.maximum(d, 0.0).sum())
        p = int(np.argmax(d)) if np.isfinite(d).all() else -1
        dmax = float(d[p]) if p >= 0 else float("nan")
        if p < 0 or not np.isfinite(trace):
            reason = 4
            break
        if not dmax > 0.0:
            reason = 3
            break
        if trace <= tol * trace0:
            reason = 2
            break
        if j == K:
            reason = 1
            break
        if n > 1:
            top = np.partition(d, n - 2)[n - 2:]
            gaps.append(float((top[1] - top[0]) / top[1]))
        r = np.sqrt(d[p])
        s = np.zeros(n)
        for c in range(j):
            s = s + L[:, c] * L[p, c]
        l = (column(p) - s) / r
        L[:, j] = l
        d = d - l * l
        d[p] = 0.0
        piv.append(p)
        j += 1
    return {"L": L, "piv": np.array(piv, dtype=np.int64), "rank": j, "reason": reason, "trace0": trace0, "trace": trace,
            "dmax": dmax, "d": d, "gaps": np.array(gaps)}


def diag_from_factor(diagA, L, piv):
    """The d that the contract's recurrence leaves, recomputed from a factor: d = diag(A), then for every column j in order
    d = d - L[:, j] L[:, j] and d[piv[j]] = 0.  Bit for bit the library's d where diagA is what it read."""
    d = np.array(diagA, dtype=np.float64)
    for j, p in enumerate(piv):
        l = L[:, j]
        d = d - l * l
        d[p] = 0.0
    return d
