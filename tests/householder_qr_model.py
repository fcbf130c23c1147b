"""A numpy restatement of the Householder tier (csrc/panel_qr.hip and the Householder branch of HipBackend::qr_thinQ) as
it is blocked, with switches that plant one defect each.  tests/test_householder_qr_model.py runs the table of
tests/householder_qr_cases.py through it: the unperturbed model passes every case, every defect fails a named set of cases.
That is how a reader knows that the table sees what it claims -- it stands in for perturbed device builds.

What is restated:
  * 16-column panels (QR_NB); per column j one sweep (qr_step_kernel) that applies reflector j - 1 to the live panel columns
    through the coefficients tw and accumulates sigma = |x|^2 and d_k = x . a_k for column j, then qr_house_kernel: beta, tau,
    row j of R and the next tw from d_k;
  * 256-row workgroups, rows_per_thread = ceil(m / 262144) sweeps of 256 rows each, one partial sum per workgroup, and the
    16-way fixed-order sum of the partials (p = g, g + 16, ...);
  * copyV (unit lower trapezoid), G = V'V, buildT (dlarft, forward columnwise), applyT with T' in the factorization and T in
    forming Q, and Q formed from the last panel first;
  * the range guard of the backend: max|Y| outside [2^-400, 2^400] -> factor 2^-e Y, scale R back.
The products that the device runs through its contraction kernel are plain matmuls here; sums are numpy's, so the model
agrees with the device to rounding, not bit for bit.

DEFECTS (the argument `defect`):
  no_second_trip   the 16-way partial sum stops after its first trip: workgroups 16, 17, ... are never added
  one_sweep        the rr loop of qr_step_kernel stops after one sweep: rows 256 .. 256 rpt - 1 of every workgroup are
                   neither updated nor summed
  drop_last_row    every workgroup skips the last row it holds
  T_not_transposed the trailing update of the factorization applies T where T' belongs
  nlive_short      nlive is one short in the last panel: its last column is never updated or reduced
  stale_tau        the sigma == 0 branch leaves tau as the previous column found it (the first column of a call finds what
                   the previous call left in the workspace: modelled as 1)
  no_prescale      the range guard is missing
"""
import numpy as np

QR_NB = 16
WG = 256
DEFECTS = ("no_second_trip", "one_sweep", "drop_last_row", "T_not_transposed", "nlive_short", "stale_tau", "no_prescale")


def rows_per_thread(m):
    return max(1, (m + WG * 1024 - 1) // (WG * 1024))


def max_blocks(m):
    """qr_max_blocks: what the backend sizes `part` by; every launch must stay at or below it."""
    rpt = rows_per_thread(m)
    return (m + WG * rpt - 1) // (WG * rpt) + 1


def prescale_exponent(amax):
    """qr_prescale_exponent."""
    if not (amax > 0.0) or np.isinf(amax):
        return 0
    if 2.0 ** -400 <= amax <= 2.0 ** 400:
        return 0
    e = int(np.frexp(amax)[1])                      # ilogb + 1
    return max(-1000, min(1000, e))


def _step(A, m, jb, b, j, last_panel, do_update, do_reduce, scale, tw, rpt, defect):
    """qr_step_kernel over all its workgroups; returns the partials (nblocks x nlive) when do_reduce."""
    nlive = jb + b - j
    if defect == "nlive_short" and last_panel:
        nlive -= 1
    rows = m - j
    rpb = WG * rpt
    nblocks = (rows + rpb - 1) // rpb
    assert nblocks <= max_blocks(m)
    r = np.arange(rows)
    live = np.ones(rows, dtype=bool)
    if defect == "one_sweep":
        live &= (r % rpb) < WG
    if defect == "drop_last_row":
        live[np.minimum((np.arange(nblocks) + 1) * rpb, rows) - 1] = False
    idx = j + r[live]
    if do_update:
        v = A[idx, j - 1] * scale
        A[idx, j - 1] = v
        if nlive > 0:
            A[idx, j:j + nlive] = A[idx, j:j + nlive] - v[:, None] * tw[None, j - jb:j - jb + nlive]
    if not do_reduce:
        return None
    nl = max(nlive, 0)
    P = np.zeros((nblocks * rpb, nl))
    sel = live & (r > 0)
    X = A[j + r[sel], j:j + nl]
    P[r[sel]] = X[:, :1] * X
    return P.reshape(nblocks, rpb, nl).sum(axis=1)


def _house(A, jb, b, j, last_panel, part, tw, state, tau, defect):
    """qr_house_kernel: returns the scale the next sweep applies."""
    nlive = jb + b - j
    if defect == "nlive_short" and last_panel:
        nlive -= 1
    if defect == "no_second_trip":
        part = part[:16]
    s_sum = np.zeros(QR_NB)
    if nlive > 0:
        s_part = np.zeros((16, nlive))
        for g in range(min(16, part.shape[0])):
            s_part[g] = part[g::16].sum(axis=0)
        s_sum[:nlive] = s_part.sum(axis=0)
    alpha = A[j, j]
    sigma = s_sum[0]
    with np.errstate(all="ignore"):
        if sigma == 0.0:
            beta, scale = alpha, 0.0
            t = state["tau"] if defect == "stale_tau" else 0.0
        else:
            beta = -np.copysign(np.sqrt(alpha * alpha + sigma), alpha)
            t = (beta - alpha) / beta
            scale = 1.0 / (alpha - beta)
        A[j, j] = beta
        tau[j] = state["tau"] = t
        for k in range(1, nlive):
            c = j + k
            wk = A[j, c] + s_sum[k] * scale
            A[j, c] = A[j, c] - t * wk
            tw[c - jb] = t * wk
    return scale


def _copyV(A, jb, b):
    V = np.tril(A[jb:, jb:jb + b], -1)
    V[np.arange(b), np.arange(b)] = 1.0
    return V


def _buildT(G, tau):
    b = len(tau)
    T = np.zeros((b, b))
    for i in range(b):
        T[:i, i] = -tau[i] * (T[:i, :i] @ G[:i, i])
        T[i, i] = tau[i]
    return T


def _apply_block_reflector(V, T, transT, C):
    """C <- (I - V op(T) V') C, as apply_block_reflector forms it: Wt = C'V, W2 = op(T) Wt', C -= V W2."""
    Wt = C.T @ V
    W2 = (T.T if transT else T) @ Wt.T
    return C - V @ W2


def qr(Y, defect=None):
    """(Q, R, tau) of the m x l panel Y (m >= l) as the device computes them."""
    assert defect is None or defect in DEFECTS, defect
    A = np.array(Y, dtype=np.float64, order="F")
    m, l = A.shape
    assert 1 <= l <= m
    e = 0
    if defect != "no_prescale":
        e = prescale_exponent(float(np.abs(A).max()))   # fmax drops NaN on the device; the cases hold none
        if e:
            A *= np.ldexp(1.0, -e)
    rpt = rows_per_thread(m)
    npanels = (l + QR_NB - 1) // QR_NB
    tau = np.zeros(l)
    Ts = []
    state = {"tau": 1.0}
    with np.errstate(all="ignore"):
        for pk in range(npanels):
            jb = pk * QR_NB
            b = min(QR_NB, l - jb)
            last = pk == npanels - 1
            tw = np.zeros(QR_NB)
            scale = 0.0
            for j in range(jb, jb + b + 1):
                do_update, do_reduce = j > jb, j < jb + b
                if m - j <= 0:
                    break
                part = _step(A, m, jb, b, j, last, do_update, do_reduce, scale, tw, rpt, defect)
                if do_reduce:
                    scale = _house(A, jb, b, j, last, part, tw, state, tau, defect)
            V = _copyV(A, jb, b)
            T = _buildT(V.T @ V, tau[jb:jb + b])
            Ts.append(T)
            if l - jb - b > 0:
                A[jb:, jb + b:] = _apply_block_reflector(V, T, defect != "T_not_transposed", A[jb:, jb + b:])
        R = np.triu(A[:l, :l])
        Q = np.zeros((m, l), order="F")
        Q[np.arange(l), np.arange(l)] = 1.0
        for pk in range(npanels - 1, -1, -1):
            jb = pk * QR_NB
            b = min(QR_NB, l - jb)
            Q[jb:, jb:] = _apply_block_reflector(_copyV(A, jb, b), Ts[pk], False, Q[jb:, jb:])
        if e:
            R = R * np.ldexp(1.0, e)
    return Q, R, tau
