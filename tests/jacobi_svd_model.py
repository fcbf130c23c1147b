"""The block Jacobi SVD of csrc/jacobi_svd.hip restated in numpy: its dispatch, its order of column pairs, its rotation.

Four pieces, used by tests/test_jacobi_svd_model.py (CPU) and tests/test_jacobi_svd_gpu.py:

  dispatch(l, forced_w)   what svd_small / svd_small_impl choose for a width: columns per block, LDS stride, blocks, the
                          register-resident instantiation, activity-driven sweeps or plain ones, dynamic LDS bytes.
  hashed_ints / graded    deterministic inputs without an RNG stream: a splitmix-style hash of (i, j, seed) reduced to the
                          integers -8 .. 8, columns scaled by powers of two over `span_bits` binades.  Every entry is an exact
                          dyadic number; exact_sum (math.fsum) is a checksum of a regenerated input.
  svd_ref(W)              singular values by one-sided Jacobi in numpy.longdouble on W itself (no QR first), tolerance
                          sqrt(l) eps_longdouble, each round of the circle tournament as one vectorised step.
  svd_model(R, svd_w)     the kernel's scheme in float64: the same tournament of blocks (rr_pair), the first block round
                          sweeping all pairs of the 2 W resident columns and the later ones the cross pairs only
                          (q = W + (p + r) mod W), the same zero padding columns, rotation test c^2 > tol^2 (a b) and
                          Rutishauser rotation -- with exact sqrt and division where the device uses v_rsq_f64 / v_rcp_f64
                          plus Newton steps, and numpy's summation order.  Not bit-exact with the device and never compared
                          with it: it shows that the order visits every column pair once per inner sweep, and that a float64
                          implementation of this scheme meets the bound the GPU tests assert with room to spare.  The pairs
                          of one (block round, inner round) are disjoint, so they are rotated as one vectorised step; that is
                          the order of the device (workgroups and quarter waves of a round run side by side).
                          The model runs full sweeps until one rotates nothing (the device's plain loop); the sparse sweeps
                          of the activity-driven form are a subset of these visits chosen by csrc/jacobi_sched.hpp, which
                          tests/host/jacobi_sched_main.cpp checks on its own.  `active_after` holds, sweep by sweep, what the
                          device's look (4 tol) would have found.
"""
import functools
import math

import numpy as np

EPS = float(np.finfo(np.float64).eps)
SVD_THREADS = 256
SVD_SCHED_INTS = 4096
LDS_REQUEST = 160 * 1024 - 64           # hipFuncAttributeMaxDynamicSharedMemorySize asked for by svd_small_impl


def rr_pair(n, r, q):
    """Pair q of round r of the circle tournament on n (even) players (jacobi_sched.hpp)."""
    if q == 0:
        return n - 1, r % (n - 1)
    return (r + q) % (n - 1), (r - q) % (n - 1)


def dispatch(l, forced_w=0):
    """What svd_small chooses for width l (forced_w: the GSI_SVD_W knob)."""
    if forced_w == 16 and l <= 600:
        w = 16
    elif forced_w == 8 and l <= 1200:
        w = 8
    elif forced_w == 4 and l <= 2500:
        w = 4
    elif forced_w == 2:
        w = 2
    elif l <= 600:
        w = 16
    elif l <= 1200:
        w = 8
    elif l <= 2500:
        w = 4
    else:
        w = 2
    lp = l
    while lp % 32 != 16:
        lp += 1
    nblk = max(2, -(-l // w))
    nblk += nblk & 1
    npairs = nblk * (nblk + 1) // 2
    ni = l // 16 if (l % 16 == 0 and l // 16 in (10, 16, 20)) else 0
    activity = (w == 16 and nblk > 2 and 4 * npairs <= SVD_SCHED_INTS)
    return {"svd_w": w, "lp": lp, "nblk": nblk, "ni": ni, "activity": activity,
            # the cross-only block rounds keep column p in registers (jacobi_cross_rounds): they exist when nblk > 2
            "resident": ni > 0 and nblk > 2 and w <= SVD_THREADS // 16,
            # the first sweep after which the activity-driven form looks at the flags
            "first_look": (1 if l < 128 else 4) if activity else 0,
            "inner_sweeps": 2 if nblk == 2 else 1,
            "lds_bytes": 2 * w * lp * 8 + 16}


# ---- inputs ------------------------------------------------------------------------------------------------------------
def hashed_ints(n, l, seed=0):
    """n x l integers in [-8, 8] from a splitmix64-style hash of (row, column, seed), as float64."""
    i = np.arange(n, dtype=np.uint64)[:, None]
    j = np.arange(l, dtype=np.uint64)[None, :]
    with np.errstate(over="ignore"):
        x = (i * np.uint64(0x9E3779B97F4A7C15) + j * np.uint64(0xD1B54A32D192ED03)
             + np.uint64(seed + 1) * np.uint64(0x8CB92BA72F3D8DD7))
        x ^= x >> np.uint64(30)
        x *= np.uint64(0xBF58476D1CE4E5B9)
        x ^= x >> np.uint64(27)
        x *= np.uint64(0x94D049BB133111EB)
        x ^= x >> np.uint64(31)
    return (x % np.uint64(17)).astype(np.int64).astype(np.float64) - 8.0


def graded(n, l, seed=0, span_bits=40):
    """hashed_ints with column j scaled by 2^-((7919 j) mod (span_bits + 1)): column norms spread over span_bits binades in
    no particular order, every entry an exact dyadic number."""
    e = -((7919 * np.arange(l)) % (span_bits + 1))
    return np.asfortranarray(hashed_ints(n, l, seed) * np.ldexp(1.0, e)[None, :])


def exact_sum(W):
    """The correctly rounded sum of all entries (math.fsum): independent of the order of summation, so it serves as a
    checksum of a regenerated input."""
    return math.fsum(np.asarray(W, dtype=np.float64).ravel(order="K").tolist())


def kappa_normalised(W):
    """kappa_2 of W with its columns scaled to unit norm: what the relative accuracy of one-sided Jacobi depends on
    (Demmel and Veselic, "Jacobi's method is more accurate than QR", SIAM J. Matrix Anal. Appl. 13, 1992)."""
    s = np.linalg.svd(W / np.linalg.norm(W, axis=0), compute_uv=False)
    return float(s[0] / s[-1])


def relative_bound(W):
    """l eps kappa_2(W_n): the bound on |S_i - ref_i| / ref_i the graded tests assert (constant 1)."""
    return W.shape[1] * EPS * kappa_normalised(W)


# ---- the rotation, vectorised over disjoint pairs --------------------------------------------------------------------
def _rotate_step(X, P, Q, tol2):
    """Rows P[k], Q[k] of X (columns of the matrix, stored as rows) are rotated where c^2 > tol2 a b; the pairs are disjoint.
    Returns the number of rotations."""
    xp, xq = X[P], X[Q]
    a = (xp * xp).sum(axis=1)
    b = (xq * xq).sum(axis=1)
    c = (xp * xq).sum(axis=1)
    m = (a > 0) & (b > 0) & (c * c > tol2 * (a * b))
    if not m.any():
        return 0
    a, b, c, xp, xq = a[m], b[m], c[m], xp[m], xq[m]
    d, e = b - a, 2 * c
    r = np.sqrt(d * d + e * e)
    t = np.copysign(np.abs(e), d * e) / (np.abs(d) + r)
    cs = 1 / np.sqrt(1 + t * t)
    sn = cs * t
    X[P[m]] = cs[:, None] * xp - sn[:, None] * xq
    X[Q[m]] = sn[:, None] * xp + cs[:, None] * xq
    return int(m.sum())


# ---- the long-double reference ------------------------------------------------------------------------------------------
def svd_ref(W, max_sweeps=60):
    """Singular values of W, descending, as numpy.longdouble: Hestenes Jacobi on the columns of W in long double."""
    W = np.asarray(W)
    l = W.shape[1]
    X = np.ascontiguousarray(W.T.astype(np.longdouble))
    if l == 1:
        return np.sqrt((X * X).sum(axis=1))
    X = X[np.argsort(-(X * X).sum(axis=1), kind="stable")]        # largest first (de Rijk): fewer sweeps, same limit
    ne = l + (l & 1)
    steps = []
    for r in range(ne - 1):
        pq = [rr_pair(ne, r, q) for q in range(ne // 2)]
        pq = [(min(p, q), max(p, q)) for p, q in pq if p < l and q < l]
        steps.append((np.array([p for p, _ in pq]), np.array([q for _, q in pq])))
    tol = np.sqrt(np.longdouble(l)) * np.finfo(np.longdouble).eps
    tol2 = tol * tol
    for _ in range(max_sweeps):
        if sum(_rotate_step(X, P, Q, tol2) for P, Q in steps) == 0:
            break
    else:
        raise RuntimeError("svd_ref: no convergence")
    return np.sort(np.sqrt((X * X).sum(axis=1)))[::-1]


# ---- the triangular factor the device hands to the Jacobi kernel --------------------------------------------------------
def cholqr2_R(W):
    """R = R2 R1 of CholeskyQR2 in float64: G = W'W, R1 = chol(G), T = W R1^-1, R2 = chol(T'T)."""
    R1 = np.linalg.cholesky(W.T @ W).T
    T = W @ np.linalg.inv(R1)
    R2 = np.linalg.cholesky(T.T @ T).T
    return R2 @ R1


def device_R(W):
    """The factor of the route svd_tall takes for the shape: CholeskyQR2 for n >= 2 l (l <= 1024), Householder below."""
    n, l = W.shape
    if n >= 2 * l and l <= 1024:
        return cholqr2_R(W)
    return np.linalg.qr(W, mode="r")


# ---- the kernel's scheme --------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def sweep_steps(l, w):
    """One inner sweep of the device as a list of steps; a step is (P, Q): the disjoint column pairs (global indices < l)
    that one inner round of one block round rotates.  Pairs with a padding column (index >= l) are left out: the device
    skips them by its a > 0 && b > 0 test."""
    nblk = max(2, -(-l // w))
    nblk += nblk & 1
    steps = []
    for br in range(max(nblk - 1, 1)):
        bps = [(0, 1)] if nblk == 2 else [rr_pair(nblk, br, x) for x in range(nblk // 2)]
        all_pairs = (br == 0)                                   # cross_only = 0 in the first block round only
        for ir in range(2 * w - 1 if all_pairs else w):
            P, Q = [], []
            for ba, bb in bps:
                for k in range(w):
                    if all_pairs:
                        p, q = rr_pair(2 * w, ir, k)
                    else:
                        p, q = k, w + (k + ir) % w
                    gp = ba * w + p if p < w else bb * w + p - w
                    gq = ba * w + q if q < w else bb * w + q - w
                    if gp < l and gq < l:
                        P.append(gp)
                        Q.append(gq)
            if P:
                steps.append((np.array(P), np.array(Q)))
    return steps


def visit_counts(l, w):
    """l x l symmetric matrix: how often one inner sweep visits each column pair."""
    V = np.zeros((l, l), dtype=np.int64)
    for P, Q in sweep_steps(l, w):
        assert len(set(P.tolist()) | set(Q.tolist())) == 2 * len(P), "a step's pairs are not disjoint"
        np.add.at(V, (P, Q), 1)
        np.add.at(V, (Q, P), 1)
    return V


def finish(X, tie_rule=True):
    """jacobi_norms_kernel + jacobi_finish_kernel: (S, U) with S[rank(c)] = |column c|, rank by descending norm, equal norms
    lower column first; a zero column gives a zero column of U.  Slots nobody writes stay NaN (tie_rule=False: the wrong
    variant that ranks equal norms equally)."""
    l = X.shape[0]
    norms = np.sqrt((X * X).sum(axis=1))
    S = np.full(l, np.nan)
    U = np.full((l, l), np.nan)
    for c in range(l):
        before = norms > norms[c]
        if tie_rule:
            before |= (norms == norms[c]) & (np.arange(l) < c)
        rank = int(before.sum())
        S[rank] = norms[c]
        U[:, rank] = X[c] * (1.0 / norms[c] if norms[c] > 0 else 0.0)
    return S, U


def svd_model(R, svd_w, max_sweeps=40, tol_scale=1.0, skip_block=None, tie_rule=True):
    """(S, U, info) of the l x l factor R by the kernel's scheme in float64 (module docstring).  info: "sweeps" as the device
    counts them (the one that rotates nothing included), "rotations" per sweep, "active_after" per sweep (a column pair above
    the look's threshold 4 tol is left), "converged".  tol_scale != 1, skip_block (the columns of that block are never rotated;
    -1: the last block) and tie_rule=False are deliberately WRONG variants for tests/test_jacobi_svd_model.py."""
    R = np.asarray(R, dtype=np.float64)
    l = R.shape[0]
    X = np.ascontiguousarray(R.T)
    tol = np.sqrt(float(l)) * EPS * tol_scale
    tol2 = tol * tol
    steps = sweep_steps(l, svd_w)
    if skip_block is not None:
        b = (l - 1) // svd_w if skip_block < 0 else skip_block
        keep = [(P // svd_w != b) & (Q // svd_w != b) for P, Q in steps]
        steps = [(P[k], Q[k]) for (P, Q), k in zip(steps, keep) if k.any()]
    nblk = max(2, -(-l // svd_w))
    inner = 2 if nblk + (nblk & 1) == 2 else 1
    info = {"sweeps": 0, "rotations": [], "active_after": [], "converged": False}
    for _ in range(max_sweeps):
        rot = 0
        for _ in range(inner):
            rot += sum(_rotate_step(X, P, Q, tol2) for P, Q in steps)
        info["sweeps"] += 1
        info["rotations"].append(rot)
        G = X @ X.T
        dg = np.diag(G)
        C2 = np.triu(G * G, 1)
        info["active_after"].append(bool((C2 > 16.0 * tol2 * np.outer(dg, dg)).any()))
        if rot == 0:
            info["converged"] = True
            break
    S, U = finish(X, tie_rule)
    return S, U, info
