"""A numpy model of a randsvd panel factored as two column halves, at a small size.

The panel is Y = S (c T) with S the n x N centred samples and T (N x l) = [T1 | T2], split at l1.  The left half
Y1 = S (c T1) is factored on its own, P1 Y1 = L1 U11.  The first l1 rows of U come from its pivot rows,
[U11 | U12] = c L11^-1 S[perm1(0:l1)] T, and with C1 = c T1 U11^-1 (so that L1 = (P1 S) C1) the right half's Schur complement
is S (c T2 - C1 U12) on all rows, in S's row order: an update of N x (l - l1) coefficients instead of n x (l - l1) numbers.
Its rows are brought into the left half's pivoted order, the rows below l1 are factored, and that factorization's
interchanges are applied to the rows of L1 below l1.  The result is the L and the interchanges of lu(Y).

This model follows those steps with scipy's dgetrf and compares with dgetrf of the whole panel: the same interchanges, and
the same L to

    |L_halves - L_whole|max  <=  l eps max_i |S[i, :]| max_j |C[:, j]|          (|L|max = 1 under partial pivoting),

C = c T U^-1 the coefficients of L = (P S) C.  Reasoning: an entry of L is a row of P S times a column of C, and either route
computes it with an error of a few eps times the product of those norms per operation on it; it takes part in at most l
elimination steps.  The interchanges can only agree where no step's choice hangs on that error, so the seeds are chosen such
that the whole factorization's smallest relative gap between its two largest pivot candidates, min_j (1 - max_{i>j} |L_ij|),
is above 1000 times the bound, and the test asserts that margin before it compares.
"""
import numpy as np
import pytest
import scipy.linalg as sla

N_ROWS, N_SAMPLES, L, L1 = 2000, 96, 40, 24
MARGIN = 1000.0


def _samples(n, N, decay, seed):
    rng = np.random.default_rng(seed)
    S = rng.standard_normal((n, N)) * (np.arange(1, N + 1, dtype=float) ** -decay)
    return S - S.mean(axis=1, keepdims=True)


def _at(piv, n):
    """(P X)[i] = X[at[i]] for LAPACK's 0-based interchanges."""
    at = np.arange(n)
    for j, r in enumerate(piv):
        at[[j, r]] = at[[r, j]]
    return at


def _unit_lower(lu):
    L = np.tril(lu, -1)
    k = lu.shape[1]
    L[np.arange(k), np.arange(k)] = 1.0
    return L


def _lu_in_halves(S, T, c, l1):
    n, l = S.shape[0], T.shape[1]
    T1, T2 = T[:, :l1], T[:, l1:]
    lu1, piv1 = sla.lu_factor(c * (S @ T1), check_finite=False)
    L1 = _unit_lower(lu1)
    at1 = _at(piv1, n)
    U1 = c * sla.solve_triangular(L1[:l1], S[at1[:l1]] @ T, lower=True, unit_diagonal=True)     # [U11 | U12]
    U11, U12 = np.triu(U1[:, :l1]), U1[:, l1:]
    C1 = c * sla.solve_triangular(U11, T1.T, trans="T", lower=False).T                          # C1 U11 = c T1
    X = S @ (c * T2 - C1 @ U12)                                                                  # in S's row order
    X = X[at1]
    X[:l1] = 0.0
    lu2, piv2 = sla.lu_factor(X[l1:], check_finite=False)
    at2 = _at(piv2, n - l1)
    Lh = np.zeros((n, l))
    Lh[:l1, :l1] = L1[:l1]
    Lh[l1:, :l1] = L1[l1:][at2]
    Lh[l1:, l1:] = _unit_lower(lu2)
    return Lh, np.concatenate([piv1, piv2 + l1])


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_two_halves_give_the_interchanges_and_the_L_of_the_whole_panel(seed):
    n, N, l, l1 = N_ROWS, N_SAMPLES, L, L1
    S = _samples(n, N, 0.75, seed)
    T = np.random.default_rng(100 + seed).standard_normal((N, l))
    c = 1.0 / (N - 1)
    lu, piv = sla.lu_factor(c * (S @ T), check_finite=False)
    Lw = _unit_lower(lu)
    U = np.triu(lu[:l])
    C = c * sla.solve_triangular(U, T.T, trans="T", lower=False).T
    bound = l * np.finfo(float).eps * np.max(np.linalg.norm(S, axis=1)) * np.max(np.linalg.norm(C, axis=0))
    below = np.abs(np.tril(Lw, -1))
    gap = np.min(1.0 - below.max(axis=0))
    print(f"\nseed {seed}: bound {bound:.2e}, smallest pivot gap {gap:.2e}")
    assert gap >= MARGIN * bound, (gap, bound)
    Lh, pivh = _lu_in_halves(S, T, c, l1)
    err = np.max(np.abs(Lh - Lw))
    print(f"seed {seed}: |L_halves - L_whole|max {err:.2e}")
    assert np.array_equal(pivh, piv), (pivh, piv)
    assert err <= bound, (err, bound)
