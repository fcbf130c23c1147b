"""numpy models of the exact posterior variance of linear inversion and kriging.  Not a test module.

`rowdot_acc`: the row pass of csrc/posterior_exact.hip and csrc/posterior_exact_host.hpp -- a loop over the columns, every
product and every sum an IEEE double operation of its own, starting from acc.  The kernel must return these bits.

`restatement`: the whole direct algorithm of `gsi_op_posterior_variance` in float64 on dense matrices
(`numpy.linalg.cholesky`, triangular solves, sums of squares).  Its error against `reference` is what the bar of the tests is
built from.

`reference`: the universal-kriging variance in `np.longdouble` from the dense C, H, D and X."""
import numpy as np

from posterior_cases import LD, chol_ld, solve_ld


def rowdot_acc(A, B, acc):
    """acc + the row sums of A .* B, added column by column in ascending order (a new array)."""
    out = np.array(acc, dtype=np.float64).reshape(-1).copy()
    for c in range(A.shape[1]):
        prod = A[:, c] * B[:, c]          # one rounding
        out = out + prod                  # one rounding
    return out


def _forward_sub(Lo, B):
    """Lo^-1 B for a lower triangular Lo, in the precision of the operands."""
    X = np.array(B, dtype=Lo.dtype)
    for j in range(Lo.shape[0]):
        X[j] = X[j] / Lo[j, j]
        X[j + 1:] -= Lo[j + 1:, j][:, None] * X[j][None, :]
    return X


def restatement(Cm, H, d, X):
    """v (n) in float64: M = H C H' + D = L L', t_i = L^-1 g_i, W_d = L^-1 Phi, S = W_d'W_d = Ls Ls', u_i = row i of
    G L^-T W_d, v_i = C_00 - |t_i|^2 + |Ls^-1 (x_i - u_i)|^2."""
    G = Cm @ H.T                                             # n x nobs
    M = H @ G + np.diag(d)
    Lo = np.linalg.cholesky(0.5 * (M + M.T))
    Tt = _forward_sub(Lo, G.T)                               # nobs x n: column i is t_i
    v = Cm[0, 0] - np.sum(Tt * Tt, axis=0)
    if X.shape[1]:
        Wd = _forward_sub(Lo, H @ X)
        Ls = np.linalg.cholesky(Wd.T @ Wd)
        U = Tt.T @ Wd
        z = _forward_sub(Ls, (X - U).T)
        v = v + np.sum(z * z, axis=0)
    return v


def reference(Cm, H, d, X):
    """The same variance in np.longdouble, from the defining formula:
    v_i = C_ii - g_i'M^-1 g_i + (x_i - Phi'M^-1 g_i)'(Phi'M^-1 Phi)^-1 (x_i - Phi'M^-1 g_i)."""
    Cl, Hl, Xl = Cm.astype(LD), H.astype(LD), X.astype(LD)
    G = Cl @ Hl.T
    M = Hl @ G + np.diag(np.asarray(d, dtype=LD))
    Lo = chol_ld(0.5 * (M + M.T))
    Tt = _forward_sub(Lo, G.T)
    v = np.diag(Cl) - np.sum(Tt * Tt, axis=0)
    if X.shape[1]:
        Phi = Hl @ Xl
        MPhi = solve_ld(M, Phi)
        R = Xl - G @ MPhi                                    # n x p: rows x_i - Phi'M^-1 g_i
        Z = solve_ld(Phi.T @ MPhi, R.T)
        v = v + np.sum(R.T * Z, axis=0)
    return v
