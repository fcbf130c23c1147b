"""A numpy model of randsvd's power steps in sample space, at a small size.

For a LowRankCovMatrix A = c S S' (c = 1/(N-1), S the n x N centred samples) the range finder factors panels Y = c S T.
With P Y = L U (LAPACK's interchanges, Julia's F.L), L = (P S) C for C = c T U^-1, so

    S'L = G C + S[mv]' ((S[perm(mv)] - S[mv]) C),    G = S'S, mv = the rows the interchanges move (at most 2 l),

which is what Backend::lowrank_power_step forms instead of the n x l product S'L.  The backend re-forms U from the pivot
rows, U = L11^-1 (P Y)[0:l], and declines when (P S) C misses the L of the factorization by more than 1e-8 on the pivot rows
or a sample of the others.  This model follows those steps with scipy's dgetrf and checks the identity to rounding where
the spectrum is the bench's (decay 0.75), and that the check flags the steep one (decay 2.5) at the first factorization.
"""
import numpy as np
import pytest
import scipy.linalg as sla

CHECK_MAX = 1e-8


def _samples(n, N, decay, seed=0):
    rng = np.random.default_rng(seed)
    S = rng.standard_normal((n, N)) * (np.arange(1, N + 1, dtype=float) ** -decay)
    return S - S.mean(axis=1, keepdims=True)            # centred over the samples, as the synthetic operator


def _perm(piv):
    """(P S)[i] = S[perm[i]] for LAPACK's 0-based interchanges; returns perm restricted to the moved rows."""
    perm = {}
    for j, r in enumerate(piv):
        if r != j:
            a, b = perm.get(j, j), perm.get(int(r), int(r))
            perm[j], perm[int(r)] = b, a
    return {i: p for i, p in perm.items() if i != p}


def _power_step(S, G, T, c, rng_rows=256):
    """One LU of Y = c S T and T_next from coefficients; returns (T_next, S'L, check value)."""
    n, l = S.shape[0], T.shape[1]
    Y = c * (S @ T)
    lu, piv = sla.lu_factor(Y, check_finite=False)
    L = np.tril(lu, -1)
    L[np.arange(l), np.arange(l)] = 1.0
    perm = _perm(piv)
    at = np.arange(n)
    for i, p in perm.items():
        at[i] = p
    mv = np.array(sorted(perm), dtype=np.int64)
    # U from the pivot rows: U = L11^-1 (P Y)[0:l] = c L11^-1 S[perm(0:l)] T
    U = c * sla.solve_triangular(L[:l], S[at[:l]] @ T, lower=True, unit_diagonal=True)
    C = c * sla.solve_triangular(U, T.T, trans="T", lower=False).T          # c T U^-1
    rows = np.concatenate([np.arange(l), l + np.random.default_rng(1).integers(0, n - l, rng_rows)])
    check = np.max(np.abs(S[at[rows]] @ C - L[rows]))
    T_next = G @ C + S[mv].T @ ((S[at[mv]] - S[mv]) @ C)
    return T_next, S.T @ L, check


@pytest.mark.parametrize("decay", [0.75])
def test_sample_space_power_step_matches_the_direct_product(decay):
    n, N, l, q = 20000, 256, 48, 2
    S = _samples(n, N, decay)
    G = S.T @ S
    c = 1.0 / (N - 1)
    Om = np.random.default_rng(7).standard_normal((n, l))
    T = S.T @ Om
    for k in range(2 * q):
        T_next, T_direct, check = _power_step(S, G, T, c)
        err = np.max(np.abs(T_next - T_direct)) / np.max(np.abs(T_direct))
        assert check <= CHECK_MAX, (k, check)
        assert err <= 1e-12, (k, err)
        T = T_direct                                     # the direct path's panel: each step compared on its own


def test_check_flags_a_steep_spectrum_at_the_first_factorization():
    n, N, l = 20000, 256, 48
    S = _samples(n, N, 2.5)
    G = S.T @ S
    c = 1.0 / (N - 1)
    T = S.T @ np.random.default_rng(7).standard_normal((n, l))
    _, _, check = _power_step(S, G, T, c)
    assert check > CHECK_MAX, check
