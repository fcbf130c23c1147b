"""The algebra of two changes to the sample-space tail, in numpy: no GPU.

1. The series of chol(I + E).  With Phi(A) = striu(A) + diag(A) / 2 the upper triangular factor of I + E and its inverse are
       R = I + R1 + R2 + O(|E|^3),  R1 = Phi(E),  R2 = -Phi(R1'R1);      X = R^-1 = I - R1 + R1 R1 - R2 + O(|E|^3)
   (cq_series_kernel, cholqr.hip).  The kernel's gate is |E|_F <= 6e-6: the dropped terms are O(|E|_2^3) <= |E|_F^3 = 2.2e-16.
   Held here against np.linalg.cholesky and its inverse, entry by entry, within 4 l eps at every norm up to the gate.  First
   order alone (R = I + R1, X = I - R1) leaves |E|^2 / 8 on a diagonal entry and |E|^2 / 2 beside it: at |E|_F = 1e-7 that is
   1e-15 to 5e-15, over 4 l eps where l is 1 or 2, and at 5.9e-6 it is 8.7e-12 at l = 32 -- second order is needed.
2. The fork identity.  Z = S B1 M with B1 = B0 XW1, so the rows that are formed beside the small SVD can start from B0:
   (S B0)(XW1 M) = (S B1) M to rounding on a graded case; one step earlier, from P0 = G A0 through X1, it is not (cond(R1)).
"""
import numpy as np
import pytest

EPS = np.finfo(np.float64).eps


def phi(A):
    return np.triu(A, 1) + 0.5 * np.diag(np.diag(A))


def series(G, order=2):
    l = G.shape[0]
    E = G - np.eye(l)
    R1 = phi(E)
    R2 = -phi(R1.T @ R1) if order >= 2 else np.zeros_like(E)
    Q = R1 @ R1 if order >= 2 else np.zeros_like(E)
    return np.eye(l) + R1 + R2, np.eye(l) - R1 + Q - R2


def sym_noise(l, norm, seed):
    rng = np.random.default_rng(seed)
    E = rng.standard_normal((l, l))
    E = E + E.T
    return E * (norm / np.linalg.norm(E))


def reference(G):
    R = np.linalg.cholesky(G).T
    return R, np.linalg.inv(R)


@pytest.mark.parametrize("norm", [1e-14, 1e-7, 3.8e-6, 5.9e-6, 6e-6])
@pytest.mark.parametrize("l", [1, 2, 31, 32, 33, 320])
def test_second_order_series_is_the_cholesky_factor(l, norm):
    G = np.eye(l) + sym_noise(l, norm, l)
    R, X = series(G)
    Rc, Xc = reference(G)
    er, ex = np.max(np.abs(R - Rc)), np.max(np.abs(X - Xc))
    back = np.max(np.abs(R.T @ R - G))
    print(f"\nl = {l}, |E|_F = {norm:.1e}: |R - chol| {er:.2e}, |X - inv| {ex:.2e}, |R'R - G| {back:.2e} (bar {4 * l * EPS:.2e})")
    assert er <= 4 * l * EPS and ex <= 4 * l * EPS and back <= 4 * l * EPS
    assert np.all(np.tril(R, -1) == 0.0) and np.all(np.tril(X, -1) == 0.0)


def _one_pair(l, norm):
    E = np.zeros((l, l))
    if l == 1:
        E[0, 0] = norm
    else:
        E[0, 1] = E[1, 0] = norm / np.sqrt(2.0)
    return np.eye(l) + E


@pytest.mark.parametrize("l, norm", [(1, 1e-7), (2, 1e-7), (32, 5.9e-6)])
def test_first_order_alone_misses_the_bar(l, norm):
    G = _one_pair(l, norm)
    Rc, Xc = reference(G)
    R1, X1 = series(G, order=1)
    R2, X2 = series(G, order=2)
    e1 = max(np.max(np.abs(R1 - Rc)), np.max(np.abs(X1 - Xc)))
    e2 = max(np.max(np.abs(R2 - Rc)), np.max(np.abs(X2 - Xc)))
    print(f"\nl = {l}, |E|_F = {norm:.1e}: first order {e1:.2e}, second order {e2:.2e} (bar {4 * l * EPS:.2e})")
    assert e1 > 4 * l * EPS
    assert e2 <= 4 * l * EPS


def test_fork_identity_on_a_graded_case():
    # the tail's chain in numpy: n = 1500, N_s = 96, l = 40, K = 32, decay 0.75, one power step's worth of grading in T
    rng = np.random.default_rng(3)
    n, Ns, l, K = 1500, 96, 40, 32
    S = rng.standard_normal((n, Ns)) * (np.arange(1, Ns + 1) ** -0.75)
    S -= S.mean(axis=1, keepdims=True)
    c = 1.0 / (Ns - 1)
    G = S.T @ S
    Lp = np.linalg.qr(c * S @ (S.T @ rng.standard_normal((n, l))))[0]        # a panel like the last LU's L
    T = S.T @ Lp
    A0 = c * T

    def chol_inv(M):
        Rr = np.linalg.cholesky(M).T
        return Rr, np.linalg.inv(Rr)

    P0 = G @ A0
    R1, X1 = chol_inv(A0.T @ P0)
    A1 = A0 @ X1
    P = G @ A1
    R2, X2 = chol_inv(A1.T @ P)
    B0 = c * P
    RW1, XW1 = chol_inv(B0.T @ (G @ B0))
    B1 = B0 @ XW1
    RW2, XW2 = chol_inv(B1.T @ (G @ B1))
    U, sv, _ = np.linalg.svd(RW2 @ RW1 @ X2)
    M = (XW2 @ (U * np.sqrt(sv)))[:, :K]
    Sl, B0l, B1l, XW1l, Ml = (a.astype(np.longdouble) for a in (S, B0, B1, XW1, M))
    Zref = Sl @ (B1l @ Ml)                                                     # what the direct product computes
    scale = np.sqrt(sv[0])

    def dist(Z):
        return float(np.max(np.linalg.norm((Z.astype(np.longdouble) - Zref).astype(np.float64), axis=0))) / scale

    direct = dist(S @ (B1 @ M))
    late = dist((S @ B1) @ M)
    early = dist((S @ B0) @ (XW1 @ M))
    before_b0 = dist((S @ P0) @ (c * (X1 @ (XW1 @ M))))
    print(f"\nmax column distance / sqrt(sigma_1): direct {direct:.2e}, (S B1) M {late:.2e}, (S B0)(XW1 M) {early:.2e}, "
          f"forked before B0 {before_b0:.2e}; cond(R1) {np.linalg.cond(R1):.1e}")
    # the project's bar between the tail's legs is 1e-12 sqrt(sigma_1); rounding of these sums is a few eps sqrt(N_s)
    assert direct <= 1e-13 and late <= 1e-13 and early <= 1e-13
    assert early <= 4 * max(late, direct)
    assert before_b0 > 10 * early                                              # why the fork is not placed before B0
