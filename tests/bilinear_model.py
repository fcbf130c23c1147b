"""numpy restatement of the bilinear reduction of the likelihood gradient (csrc/bilinear_terms.hip,
csrc/bilinear_terms_host.hpp), with the same products and the same order of additions, so the results
agree bit for bit:

  V = Y + dd .* R         d = dd[i] R[i, c] rounded, then v = Y[i, c] + d          (dd None: V = Y)
  p = L[i, a] V[i, c]     rounded on its own
  per chunk of CHUNK = 2048 rows: s = 0.0, then s = s + p in ascending row order
  the result: total = 0.0, then total = total + s in ascending chunk order

numpy's `cumsum` adds strictly one element at a time in index order (its `sum` adds pairwise: it is NOT used here)."""
import numpy as np

CHUNK = 2048
MAX_G = 16


def _ordered_sum(P):
    """Column sums of P (rows x outputs) in the order above."""
    n = P.shape[0]
    parts = [np.cumsum(np.vstack([np.zeros((1, P.shape[1])), P[r0:min(n, r0 + CHUNK)]]), axis=0)[-1] for r0 in range(0, n, CHUNK)]
    return np.cumsum(np.vstack([np.zeros((1, P.shape[1]))] + parts), axis=0)[-1]


def terms(L, Y, R=None, dd=None, g=0):
    """(gram (g x g), t (b - g)) of the header's gsi_mat_bilinear."""
    L, Y = np.asarray(L, dtype=np.float64), np.asarray(Y, dtype=np.float64)
    n, b = L.shape
    assert 0 <= g <= min(b, MAX_G)
    V = Y
    if dd is not None:
        d = np.asarray(dd, dtype=np.float64)[:, None] * np.asarray(R, dtype=np.float64)
        V = Y + d
    gram = np.zeros((g, g))
    for c in range(g):
        gram[:, c] = _ordered_sum(L[:, :g] * V[:, c:c + 1])
    t = _ordered_sum(L[:, g:] * V[:, g:]) if b > g else np.zeros(0)
    return gram, t
