"""Cases, references and checks for the Householder tier of qr_thinQ (csrc/panel_qr.hip), shared by
tests/test_householder_qr_model.py (the numpy restatement and its planted defects), tests/test_householder_qr_cpu.py (LAPACK
and the CPU reference library: they show that the bars are fair) and tests/test_householder_qr_gpu.py (the HIP kernels).
Nothing here touches a GPU or a device library: every check takes `qr`, a callable Y -> (Q, R).

Reference: an unblocked Householder QR in np.longdouble with dlarfg's convention, beta = -copysign(norm, alpha), and
tau = 0 (H = I) where the column is zero below the diagonal.  Both backends use that convention, so Q and R are unique and
equal to LAPACK's to rounding: the reference pins their signs, which Q'Q = I and Q R = Y alone do not.

Bars (eps = 2^-52; cn_j = the 2-norm of column j of Y, 1 where that is zero; kappa = kappa_2 of Y with unit columns):
  finite, R exactly zero below the diagonal
  orth    |Q'Q - I|max <= 1e-13                                    the bar of test_gpu_parity.test_qr_thinQ
  resid   ||Y_j - (Q R)_j||_2 <= (l + 4) eps cn_j, column by column, the product in long double: Householder QR is
          column-wise backward stable; a max-norm over a graded panel does not look at its small columns
  R       max_ij |R_ij - Rref_ij| / cn_j <= (l + 4) eps kappa       only where kappa < 1e3
  Q       max_ij |Q_ij - Qref_ij| <= (l + 4) eps kappa              likewise; Q is determined once R's signs are
  range   rank-deficient cases instead of R and Q: ||Y - Q Q'Y||_F <= 1e-11 ||Y||_F, the bar of test_qr_rank_deficient
The constants rest on the formats and on the form test_jacobi_svd_gpu.py and test_cholqr_kernels_gpu.py use (column-scaled
condition number, constant 1, l + 4 for the l reflectors and the few operations of each); what LAPACK and the CPU library
measure against them is printed by tests/test_householder_qr_cpu.py and quoted in tests/test_householder_qr_gpu.py.  One
yardstick misses one bar -- the CPU library's R at 262145 x 17, 2.58 of it, because it sums 262145 terms one after the
other -- and test_householder_qr_cpu.py widens that bar for that library and that case alone; nothing is widened for the
HIP kernels, LAPACK or the restatement.

Out of scope: leading dimensions other than m (the public entry point always passes ld == m); per-column extremes of
range, i.e. one column at 2^-530 beside columns at 1 (the range cases scale the whole panel).
"""
import collections

import numpy as np

import jacobi_svd_model as jm

EPS = 2.0 ** -52
LD = np.longdouble

Case = collections.namedtuple("Case", "name m l kind edge")

# ---- the table: full-rank cases that need GSI_NO_CHOLQR to reach the tier -------------------------------------------
FORCED = [
    Case("1x1", 1, 1, "normal", "smallest: the only reflector has no rows below it (sigma == 0)"),
    Case("2x1", 2, 1, "normal", "one row below the diagonal; a single partial panel of one column"),
    Case("5x5", 5, 5, "normal", "m == l inside one partial panel: the last reflector takes sigma == 0"),
    Case("16x16", 16, 16, "normal", "m == l at a panel edge: the sweep after the last column has no rows (rows <= 0: break)"),
    Case("17x17", 17, 17, "normal", "m == l past a panel edge: second panel one column wide with no rows below it"),
    Case("33x32", 33, 32, "normal", "m = l + 1: one row below the last diagonal entry; two full panels"),
    Case("300x15", 300, 15, "normal", "panel width 15"),
    Case("300x16", 300, 16, "normal", "panel width 16, no trailing update"),
    Case("300x17", 300, 17, "normal", "second panel one column wide (b = 1)"),
    Case("257x31", 257, 31, "normal", "one row in the last workgroup at j = 0; second panel 15 wide"),
    Case("513x33", 513, 33, "normal", "one row in the third workgroup; third panel one column wide"),
    Case("4400x20", 4400, 20, "normal", "18 workgroups: second trip of the partial sum in qr_house_kernel; second panel 4 wide"),
    Case("262145x17", 262145, 17, "normal", "rows_per_thread == 2, one row into the second sweep of every thread; part sized by qr_max_blocks"),
    Case("300x41graded", 300, 41, "graded", "column norms over 40 binades: the column-wise bars see the small columns"),
    Case("4400x20graded", 4400, 20, "graded", "the same beyond 16 workgroups"),
]
# ---- full-rank cases that the gate sends to the tier, no switch set ---------------------------------------------------
GATE = [
    Case("100x60", 100, 60, "normal", "m < 2 l: Householder by the gate"),
    Case("1100x1025", 1100, 1025, "normal", "l > 1024 by the gate; 65 panels, the last one column wide"),
]
# ---- rank-deficient cases: they pass the gate, both CholeskyQR tiers decline ------------------------------------------
RANKDEF = [
    Case("2000x40rank7", 2000, 40, "rank7", "exact rank 7 from integer factors"),
    Case("2000x40rank7zerocol", 2000, 40, "rank7zero", "the same with column 5 exactly zero: sigma == 0 and alpha == 0 in mid-panel"),
    Case("300x12rank5", 300, 12, "rank5", "rank 5 of 12 in one partial panel"),
]
NO_REFERENCE = {"1100x1025"}          # the long-double reference would take minutes: residual, orthogonality, triangularity only
SCALE_BASE = Case("300x33", 300, 33, "normal", "the panel of the scaling and range cases")
SCALINGS = [300, -300, 400, -400]     # qr(2^s Y) must return the bits of Q and 2^s R
RANGES = [520, -520, 600, -600]       # beyond plain sums of squares: raise, or meet every bar


def panel(case):
    m, l = case.m, case.l
    rng = np.random.default_rng(1000003 * m + l)
    if case.kind == "normal":
        Y = rng.standard_normal((m, l))
    elif case.kind == "graded":
        Y = jm.graded(m, l, seed=0, span_bits=40)
    else:
        r = 5 if case.kind == "rank5" else 7
        Y = rng.integers(-4, 5, size=(m, r)).astype(np.float64) @ rng.integers(-4, 5, size=(r, l)).astype(np.float64)
        if case.kind == "rank7zero":
            Y[:, 5] = 0.0
    return np.asfortranarray(Y)


# ---- reference -----------------------------------------------------------------------------------------------------------
def reference_qr(Y):
    """(Q, R, tau) in np.longdouble: unblocked Householder QR, dlarfg's signs, thin Q formed from the last reflector first."""
    A = np.array(Y, dtype=LD, order="F")
    m, l = A.shape
    tau = np.zeros(l, dtype=LD)
    for j in range(l):
        alpha = A[j, j]
        x = A[j + 1:, j]
        sigma = np.dot(x, x)
        if sigma == 0:
            continue
        beta = -np.copysign(np.sqrt(alpha * alpha + sigma), alpha)
        tau[j] = (beta - alpha) / beta
        x /= (alpha - beta)
        A[j, j] = beta
        if j + 1 < l:
            w = tau[j] * (A[j, j + 1:] + x @ A[j + 1:, j + 1:])
            A[j, j + 1:] -= w
            A[j + 1:, j + 1:] -= np.outer(x, w)
    R = np.triu(A[:l, :l])
    Q = np.zeros((m, l), dtype=LD, order="F")
    Q[np.arange(l), np.arange(l)] = 1
    for j in range(l - 1, -1, -1):
        if tau[j] == 0:
            continue
        x = A[j + 1:, j]
        w = tau[j] * (Q[j, j:] + x @ Q[j + 1:, j:])
        Q[j, j:] -= w
        Q[j + 1:, j:] -= np.outer(x, w)
    return Q, R, tau


def column_norms(Y):
    """cn_j in long double (no overflow for a panel scaled by 2^600); 1 for a zero column."""
    Yl = np.asarray(Y, dtype=LD)
    cn = np.sqrt((Yl * Yl).sum(axis=0))
    return np.where(cn == 0, LD(1), cn)


def kappa_normalised(Y):
    Yn = (np.asarray(Y, dtype=LD) / column_norms(Y)).astype(np.float64)
    s = np.linalg.svd(Yn, compute_uv=False)
    return float(s[0] / s[-1]) if s[-1] > 0 else np.inf


_REF = {}


def reference(case):
    """{Y, cn, kappa, Q, R} of a table case, computed once per process and left unchanged."""
    if case.name not in _REF:
        Y = panel(case)
        ref = {"Y": Y, "cn": column_norms(Y), "kappa": None, "Q": None, "R": None}
        if case.kind in ("normal", "graded") and case.name not in NO_REFERENCE:
            ref["kappa"] = kappa_normalised(Y)
            ref["Q"], ref["R"], _ = reference_qr(Y)
        _REF[case.name] = ref
    return _REF[case.name]


# ---- checks -------------------------------------------------------------------------------------------------------------
def product_longdouble(Q, R):
    """Q R in long double, R upper triangular: column block by column block, only the rows of R that are not zero."""
    Ql, Rl = np.asarray(Q, dtype=LD), np.asarray(R, dtype=LD)
    m, l = Ql.shape
    P = np.empty((m, l), dtype=LD)
    for j0 in range(0, l, 128):
        j1 = min(l, j0 + 128)
        P[:, j0:j1] = Ql[:, :j1] @ Rl[:j1, j0:j1]
    return P


def measure(Y, Q, R, ref=None, rank_deficient=False):
    """{bar: measured / bar} for the factors (Q, R) of Y; `finite` and `triangular` are 0 or inf.  ref: {cn, kappa, Q, R}
    (R, Q compared where kappa < 1e3)."""
    m, l = Y.shape
    out = {}
    Q, R = np.asarray(Q), np.asarray(R)
    out["finite"] = 0.0 if (np.isfinite(Q).all() and np.isfinite(R).all()) else np.inf
    out["triangular"] = 0.0 if not np.tril(R, -1).any() else np.inf
    if out["finite"]:
        return out
    cn = ref["cn"] if ref is not None else column_norms(Y)
    out["orth"] = float(np.abs(Q.T @ Q - np.eye(l)).max() / 1e-13)
    D = np.asarray(Y, dtype=LD) - product_longdouble(Q, R)
    out["resid"] = float((np.sqrt((D * D).sum(axis=0)) / cn).max() / ((l + 4) * EPS))
    if rank_deficient:
        Yl = np.asarray(Y, dtype=LD)
        Ql = Q.astype(LD)
        E = Yl - Ql @ (Ql.T @ Yl)
        out["range"] = float(np.sqrt((E * E).sum()) / np.sqrt((Yl * Yl).sum()) / 1e-11)
    elif ref is not None and ref["R"] is not None and ref["kappa"] < 1e3:
        bar = (l + 4) * EPS * ref["kappa"]
        out["R"] = float((np.abs(R.astype(LD) - ref["R"]) / cn[None, :]).max() / bar)
        out["Q"] = float(np.abs(Q.astype(LD) - ref["Q"]).max() / bar)
    return out


def failed(ratios, widen=None):
    """widen: {bar: factor} for a yardstick that is known to miss a bar on one case (the callers say why); never for HIP."""
    return any(not (v <= (widen or {}).get(k, 1.0)) for k, v in ratios.items())


MEASURED = {}     # who -> case name -> ratios: the record behind the figures quoted in the docstrings


def _note(who, name, ratios):
    MEASURED.setdefault(who, {})[name] = ratios
    print(who, name, {k: float("%.3g" % v) for k, v in ratios.items()})


def check_case(qr, case, who="?", widen=None):
    """One table case through `qr`, every bar asserted; returns the ratios (always against the bars as stated above)."""
    ref = reference(case)
    Q, R = qr(ref["Y"].copy(order="F"))
    ratios = measure(ref["Y"], Q, R, ref, rank_deficient=case in RANKDEF)
    _note(who, case.name, ratios)
    assert not failed(ratios, widen), (case.name, ratios)
    if case in RANKDEF:
        assert set(ratios) == {"finite", "triangular", "orth", "resid", "range"}, ratios
    elif case.name not in NO_REFERENCE:
        assert set(ratios) == {"finite", "triangular", "orth", "resid", "R", "Q"}, (ratios, ref["kappa"])
    return ratios


# ---- exact cases ----------------------------------------------------------------------------------------------------------
def upper_triangular_panel(n=20, m=40):
    """[U; 0] with U upper triangular, integer entries in [-4, 4]: every step takes the sigma == 0 branch (H = I)."""
    U = np.triu(np.random.default_rng(2020).integers(-4, 5, size=(n, n)).astype(np.float64))
    return np.asfortranarray(np.vstack([U, np.zeros((m - n, n))])), U


def signed_selection_panel(m, l, first_row=0):
    """One entry of +-1 per column, in distinct rows >= first_row: all arithmetic of the factorization stays in {0, +-1}."""
    rng = np.random.default_rng(7 * m + l)
    rows = first_row + rng.permutation(m - first_row)[:l]
    Y = np.zeros((m, l), order="F")
    Y[rows, np.arange(l)] = rng.choice([-1.0, 1.0], size=l)
    return Y


EXACT = ["upper40x20", "signed40x20", "signed600x33"]


def check_exact(qr, name):
    if name == "upper40x20":
        Y, U = upper_triangular_panel()
        Q, R = qr(Y.copy(order="F"))
        assert np.array_equal(R, U), np.abs(R - U).max()
        assert np.array_equal(Q, np.eye(40, 20))
        return
    Y = signed_selection_panel(40, 20) if name == "signed40x20" else signed_selection_panel(600, 33, first_row=256)
    l = Y.shape[1]
    Q, R = qr(Y.copy(order="F"))
    assert np.isin(Q, (-1.0, 0.0, 1.0)).all() and np.isin(R, (-1.0, 0.0, 1.0)).all()
    assert not np.tril(R, -1).any()
    assert np.array_equal(Q @ R, Y)
    assert np.array_equal(Q.T @ Q, np.eye(l))


def exact_failed(qr, name):
    try:
        check_exact(qr, name)
    except AssertionError:
        return True
    return False


# ---- scaling and range ------------------------------------------------------------------------------------------------------
def check_scaling(qr, s, base=None):
    """qr(2^s Y) returns the bits of Q and 2^s R.  base: (Q, R) of the unscaled panel, if the caller has it already."""
    Y = reference(SCALE_BASE)["Y"]
    Q0, R0 = base if base is not None else qr(Y.copy(order="F"))
    Q, R = qr(np.asfortranarray(np.ldexp(Y, s)))
    assert np.array_equal(Q, Q0), (s, np.abs(Q - Q0).max())
    assert np.array_equal(R, np.ldexp(R0, s)), s


def scaled_reference(s):
    """The reference of 2^s Y for the base panel: the same Q, 2^s R and 2^s cn, exactly (long double keeps the range)."""
    ref = reference(SCALE_BASE)
    f = np.ldexp(LD(1), s)
    return {"Y": np.asfortranarray(np.ldexp(ref["Y"], s)), "cn": ref["cn"] * f, "kappa": ref["kappa"], "Q": ref["Q"],
            "R": ref["R"] * f}


def range_ratios(qr, s, errors):
    """None when `qr` raised one of `errors` for 2^s Y (a refusal is a legal answer), else the ratios of every full-rank bar."""
    ref = scaled_reference(s)
    try:
        Q, R = qr(ref["Y"].copy(order="F"))
    except errors:
        return None
    return measure(ref["Y"], Q, R, ref)


def check_range(qr, s, errors, who="?"):
    ratios = range_ratios(qr, s, errors)
    if ratios is None:
        _note(who, "300x33*2^%d" % s, {"raised": 0.0})
        return None
    _note(who, "300x33*2^%d" % s, ratios)
    assert not failed(ratios), (s, ratios)
    assert set(ratios) == {"finite", "triangular", "orth", "resid", "R", "Q"}, ratios
    return ratios
