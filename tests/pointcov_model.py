"""A host model of how the scattered-point covariance product picks and tiles its kernel, the case table of
test_pointcov_kernels_gpu.py, the long-double reference of the entries and the per-entry bar.  No GPU, no library.

model(M, L, K, roff, koff, rows, forced, ncus, wide_on) mirrors

  csrc/pointcov_gemm.hip  wide_applies          :410-414  96 < L (GSI_POINTCOV_WIDE=0: never) -- otherwise gemm_f64.hip's GEN 2
                          wide_tiling           :370-409  NTQ / MT / RGN, column chunks, workgroups, the K split and kchunk
                          pointcov_wide_kernel  :57-58    NT = (8 / RGN) NTQ 16-column tiles, BM = 16 MT RGN rows
                                                :78-82    r0, kbeg, kend, ntiles = ceil((kend - kbeg) / 16)
                                                :96       NS: X prefetch sets, 2 at MT = 2, 1 at MT = 3
                                                :165,203  the uniform "does the diagonal cross this slot" test
  csrc/pipeline.cpp       op_mul / op_mul_t     :134,313  A X: (mloc, l, n, roff = row0, koff = 0); A' X: (n, l, mloc, 0, row0)
  context.py              Context.shard                   pad = ceil(n / ranks), row0 = rank pad

The reference (reference()) is numpy.longdouble (64-bit mantissa, asserted) from the unscaled, untranslated points:
sigma2 poly(a) exp(-arg), nugget where row index == column index and nowhere else.

Bar per entry, relative to the reference entry:  bar = 16 (1 + arg + delta) 2^-53,  E = the largest coordinate extent of the
point set in the kernel's scaled units (scale c1 / ell, 1 / (ell sqrt 2) for the Gaussian), delta = E (exponential, Matern),
E sqrt(2 arg) (Gaussian).  Where the 16 comes from: translate-then-scale of a coordinate and the subtraction put at most
~4 E 2^-53 absolute into the argument; square root and argument reduction ~2 arg 2^-53 into the exponent; polynomial, table,
sigma2 and the Matern factor a few ulp: <= 8 units, and the bar is twice that.  Entries whose reference is below
2^-1000 sigma2 (subnormal results of ldexp) leave the relative check: finite, >= 0, <= 2^-999 sigma2, exactly 0 where
arg > 760."""
import collections
import functools

import numpy as np

NCUS = 256                       # MI355X
WBK = 16
KINDS = ("gaussian", "exponential", "matern32", "matern52")
C1 = {"gaussian": None, "exponential": 1.0, "matern32": 1.7320508075688772, "matern52": 2.23606797749979}
ELL, SIGMA2 = 3.7, 2.5
NUGGET = 0.75 * SIGMA2
OFFSET = (5.0e5, 4.6e6, 120.0)
LD = np.longdouble
U = LD(2.0) ** -53
TAIL = LD(2.0) ** -1000
MAX_TAIL_FRACTION = 0.10


# ---- the launcher ------------------------------------------------------------------------------------------------------------
def wide_applies(L, wide_on=True, tall_on=True):
    return wide_on and (L > 160 or (tall_on and L > 96))


def wide_tiling(M, L, K, rows=96, forced=0, ncus=NCUS):
    w = {}
    tiles = (L + 15) // 16
    if L <= 160:
        w["rgn"], w["mt"] = 4, 3
        w["ntq"] = 4 if tiles <= 8 else 5
        w["nchunks"] = 1
        w["pack_groups"] = (2 * w["ntq"] * 16 + 63) // 64
        w["active"] = (M + 191) // 192
    else:
        w["rgn"] = 2
        w["mt"] = 2 if rows == 64 else 3
        nch = (tiles + 19) // 20
        nt = (tiles + nch - 1) // nch
        w["ntq"] = max((nt + 3) // 4, 3)
        w["nchunks"] = (L + 64 * w["ntq"] - 1) // (64 * w["ntq"])
        w["pack_groups"] = w["ntq"]
        w["active"] = ((M + 32 * w["mt"] - 1) // (32 * w["mt"])) * w["nchunks"]
    nsplit = 1
    if K > 0 and forced > 0:
        nsplit = forced
    elif K > 0:
        best, sp = 0.0, 1
        while sp <= 16 and (sp == 1 or K // sp >= 4096):
            cost = float((w["active"] * sp + ncus - 1) // ncus) / float(sp) * (1.0 + 0.002 * float(sp))
            if sp == 1 or cost < best:
                best, nsplit = cost, sp
            sp += 1
    w["nsplit"] = nsplit
    kchunk = (K + nsplit - 1) // nsplit
    kchunk = ((kchunk + 31) // 32) * 32
    if kchunk == 0:
        kchunk = 32
    w["kchunk"] = kchunk
    w["ns_eff"] = (K + kchunk - 1) // kchunk if K > 0 else 1
    return w


GEN2 = "GEN2"


def model(M, L, K, roff=0, koff=0, rows=96, forced=0, ncus=NCUS, wide_on=True):
    """What one product launches.  kernel: GEN2 or (NTQ, MT, RGN)."""
    if M <= 0 or L <= 0 or K <= 0:
        return None
    if not wide_applies(L, wide_on):
        return {"kernel": GEN2, "M": M, "L": L, "K": K, "roff": roff, "koff": koff}
    w = wide_tiling(M, L, K, rows, forced, ncus)
    BM = 16 * w["mt"] * w["rgn"]
    chunk_cols = (8 // w["rgn"]) * w["ntq"] * 16
    ntiles, diag = [], False
    for split in range(w["ns_eff"]):
        kbeg = split * w["kchunk"]
        kend = min(kbeg + w["kchunk"], K)
        ntiles.append((kend - kbeg + WBK - 1) // WBK if kend > kbeg else 0)
        for r0 in range(0, M, BM):
            # some k in [kbeg, kend) with 0 <= koff + k - roff - r0 < BM
            lo, hi = max(kbeg, roff + r0 - koff), min(kend, roff + r0 - koff + BM)
            diag = diag or lo < hi
    return {"kernel": (w["ntq"], w["mt"], w["rgn"]), "M": M, "L": L, "K": K, "roff": roff, "koff": koff, "BM": BM,
            "nchunks": w["nchunks"], "ns_eff": w["ns_eff"], "kchunk": w["kchunk"], "ntiles": tuple(sorted(ntiles)),
            "last_split": (ntiles[-1], (K - (w["ns_eff"] - 1) * w["kchunk"]) % WBK != 0),     # (tiles, ragged last tile)
            "NS": 2 if w["mt"] == 2 else 1, "ragged_rows": M % BM != 0, "ragged_cols": L % 16 != 0,
            "unused_cols": chunk_cols * w["nchunks"] - L, "diag": diag}


def shard(n, ranks, rank):
    pad = -(-n // ranks)
    row0 = min(rank * pad, n)
    return row0, min(pad, n - row0)


# ---- environments and cases --------------------------------------------------------------------------------------------------
# name -> (environment of the child process, rows knob, forced split, wide kernel on, rank threads)
Env = collections.namedtuple("Env", "vars rows forced wide_on ranks")
ENVS = collections.OrderedDict([
    ("default", Env({}, 96, 0, True, 1)),
    ("rows64", Env({"GSI_POINTCOV_ROWS": "64"}, 64, 0, True, 1)),
    ("split2", Env({"GSI_GEMM_FORCE_SPLIT": "2"}, 96, 2, True, 1)),
    ("split3", Env({"GSI_GEMM_FORCE_SPLIT": "3"}, 96, 3, True, 1)),
    ("rows64-split2", Env({"GSI_POINTCOV_ROWS": "64", "GSI_GEMM_FORCE_SPLIT": "2"}, 64, 2, True, 1)),
    ("rows64-split3", Env({"GSI_POINTCOV_ROWS": "64", "GSI_GEMM_FORCE_SPLIT": "3"}, 64, 3, True, 1)),
    ("wide0", Env({"GSI_POINTCOV_WIDE": "0"}, 96, 0, False, 1)),
    ("ranks3", Env({"GSI_LOCAL_COMM": "1"}, 96, 0, True, 3)),
    ("ranks3-rows64", Env({"GSI_LOCAL_COMM": "1", "GSI_POINTCOV_ROWS": "64"}, 64, 0, True, 3)),
    ("ranks3-split2", Env({"GSI_LOCAL_COMM": "1", "GSI_GEMM_FORCE_SPLIT": "2"}, 96, 2, True, 3)),
    ("ranks3-rows64-split3", Env({"GSI_LOCAL_COMM": "1", "GSI_POINTCOV_ROWS": "64", "GSI_GEMM_FORCE_SPLIT": "3"}, 64, 3, True, 3)),
])

Case = collections.namedtuple("Case", "group env kind d n l offset")

# group -> (environment, [(l, [n, ...]), ...]); a group is what one child process (one GPU test) runs
_TABLE = collections.OrderedDict([
    # GEN 2 (l <= 96) and the 192-row arrangement <4,3,4> (l <= 128), <5,3,4> (l <= 160): BM = 192
    ("narrow", ("default", [(16, [1, 17, 130]), (96, [1, 17, 130]),
                            (97, [1, 33, 192, 400]), (128, [16, 191, 193]), (129, [1, 192, 193]), (160, [16, 33, 191, 400])])),
    # 96 rows: NTQ = 3, 3, 4, 4, 5, 5, then 3 in two chunks, 4 in two chunks, 4 in three chunks
    ("rows96", ("default", [(161, [1, 17, 96, 200]), (192, [16, 33, 97]), (200, [1, 95, 224]), (256, [17, 96, 200]),
                            (257, [16, 33, 97]), (320, [1, 17, 95, 96, 97, 224]), (321, [16, 33, 200]), (400, [17, 96, 224]),
                            (641, [1, 33, 97, 200])])),
    # 64 rows (NS == 2): tile counts 1, 1, 2, 2, 3, 3, 4, 4, 4, 5, 13 at n = 1, 16, 17, 32, 33, 48, 49, 63, 64, 65, 208
    ("rows64", ("rows64", [(161, [1, 17, 33, 49, 65, 208]), (200, [16, 32, 48, 64, 65]), (320, [1, 17, 33, 63, 64, 65, 208]),
                           (321, [16, 49, 208]), (400, [17, 33, 64, 65])])),
    ("split2", ("split2", [(128, [40]), (160, [100]), (161, [200]), (200, [40]), (320, [100]), (400, [200])])),
    ("split3", ("split3", [(128, [200]), (160, [40]), (161, [100]), (200, [200]), (320, [40]), (641, [100])])),
    ("rows64-split2", ("rows64-split2", [(161, [40]), (200, [100]), (320, [200]), (321, [100])])),
    ("rows64-split3", ("rows64-split3", [(161, [200]), (200, [40]), (320, [100]), (400, [200])])),
    # l = 200 and 320 through GEN 2: the other generator call site on the same entries
    ("wide0", ("wide0", [(200, [17, 130]), (320, [33, 200])])),
    # three rank threads: n = 2 leaves a rank without rows, n = 100 gives 34 / 34 / 32 rows
    ("ranks3", ("ranks3", [(128, [100, 333]), (200, [2, 200]), (320, [100, 333])])),
    ("ranks3-rows64", ("ranks3-rows64", [(200, [100, 333]), (320, [2, 200])])),
    ("ranks3-split2", ("ranks3-split2", [(128, [200]), (200, [100]), (320, [333])])),
    ("ranks3-rows64-split3", ("ranks3-rows64-split3", [(200, [200, 333]), (320, [100])])),
])
# the chooser itself splits this one (K / 2 >= 4096); entries of 320 selected columns only
NATURAL = Case("natural", "default", "exponential", 2, 8192, 320, True)


def _cases():
    out = []
    for group, (env, rows) in _TABLE.items():
        i = 0                                         # (kind, d) cycle through all twelve pairs within a group
        for l, ns in rows:
            for n in ns:
                out.append(Case(group, env, KINDS[i % 4], 1 + i % 3, n, l, i % 2 == 1))
                i += 1
    return out + [NATURAL]


CASES = _cases()
GROUPS = list(_TABLE) + ["natural"]


def case_id(c):
    return "%s-%s%dd-n%d-l%d%s" % (c.group, c.kind, c.d, c.n, c.l, "-utm" if c.offset else "")


def group_cases(group):
    return [c for c in CASES if c.group == group]


def launches(case, ncus=NCUS):
    """[(which product, rank, model)] of the case's A X and A' X on every rank that has rows."""
    e = ENVS[case.env]
    out = []
    for rank in range(e.ranks):
        row0, mloc = shard(case.n, e.ranks, rank)
        if mloc == 0:
            out.append(("none", rank, None))
            continue
        out.append(("mul", rank, model(mloc, case.l, case.n, row0, 0, e.rows, e.forced, ncus, e.wide_on)))
        out.append(("mul_t", rank, model(case.n, case.l, mloc, 0, row0, e.rows, e.forced, ncus, e.wide_on)))
    return out


# ---- point sets, inputs ------------------------------------------------------------------------------------------------------
def _seed(case):
    return 100003 * case.n + 1009 * case.d + 17 * int(case.offset) + 1


def n_far(n):
    """Points moved out to 300 .. 800 ell: eight, fewer where their rows and columns would be more than 8 % of the matrix."""
    k = 8
    while k > 0 and (2 * k > n or 1.0 - ((n - k) / n) ** 2 > 0.08):
        k -= 1
    return k


@functools.lru_cache(maxsize=None)
def _points(d, n, offset, seed):
    rng = np.random.default_rng(seed)
    P = rng.uniform(0.0, 25.0 * ELL, size=(d, n))
    order = rng.permutation(n)
    npairs = min(8, n // 4)
    for p in range(npairs):                           # coincident pairs off the diagonal
        P[:, order[2 * p + 1]] = P[:, order[2 * p]]
    far = order[2 * npairs:2 * npairs + n_far(n)]
    # 800 ell first (beyond the underflow for every kind), then down to 300 ell (the far tail of the relative check)
    P[rng.integers(0, d, size=far.size), far] += np.linspace(800.0, 300.0, max(far.size, 2))[:far.size] * ELL
    if offset:
        P = P + np.array(OFFSET[:d])[:, None]
    P = np.asfortranarray(P)
    P.setflags(write=False)
    return P


def points(case):
    return _points(case.d, case.n, case.offset, _seed(case))


def onehot_bases(case):
    """Bases of the one-hot products: column c of product p selects reduction index (base_p + c) mod n; together the
    products select every index (n = 8192: one product across the boundary of the two splits)."""
    if case.n > 2048:
        return [case.n // 2 - case.l // 2]
    base0 = (3 * case.l + 5) % case.n
    return [base0 + p * case.l for p in range(-(-case.n // case.l))]


def onehot_columns(case, base):
    return (base + np.arange(case.l)) % case.n


def onehot(case, base):
    X = np.zeros((case.n, case.l), order="F")
    X[onehot_columns(case, base), np.arange(case.l)] = 1.0
    return X


def normal_panel(case):
    return np.asfortranarray(np.random.default_rng(_seed(case) + 7).standard_normal((case.n, case.l)))


def has_product_check(case):
    return case.n <= 2048


# ---- reference and bar -------------------------------------------------------------------------------------------------------
def check_longdouble():
    assert np.finfo(LD).eps < 2e-19, "numpy.longdouble has no 64-bit mantissa here"


def reference(P, kind, cols=None, ell=ELL, sigma2=SIGMA2, nugget=NUGGET):
    """(A[:, cols], arg[:, cols]) in long double."""
    check_longdouble()
    n = P.shape[1]
    cols = np.arange(n) if cols is None else np.asarray(cols)
    Pl = P.astype(LD)
    d2 = np.zeros((n, cols.size), dtype=LD)
    for a in range(P.shape[0]):
        t = Pl[a][:, None] - Pl[a][cols][None, :]
        d2 += t * t
    r = np.sqrt(d2) / LD(ell)
    if kind == "gaussian":
        arg, poly = r * r / LD(2), LD(1)
    elif kind == "exponential":
        arg, poly = r, LD(1)
    elif kind == "matern32":
        arg = np.sqrt(LD(3)) * r
        poly = 1 + arg
    else:
        arg = np.sqrt(LD(5)) * r
        poly = 1 + arg + arg * arg / LD(3)
    A = LD(sigma2) * poly * np.exp(-arg)
    A = A + LD(nugget) * (np.arange(n)[:, None] == cols[None, :])
    return A, arg


@functools.lru_cache(maxsize=8)
def _case_reference(kind, d, n, offset, seed):
    P = _points(d, n, offset, seed)
    A, arg = reference(P, kind)
    bar = entry_bar(P, kind, arg)
    for a in (A, arg, bar):
        a.setflags(write=False)
    return A, arg, bar


def case_reference(case, cols=None):
    """(A, arg, bar), the full matrix (n <= 2048) or the selected columns."""
    if cols is None or case.n <= 2048:
        A, arg, bar = _case_reference(case.kind, case.d, case.n, case.offset, _seed(case))
        return (A, arg, bar) if cols is None else (A[:, cols], arg[:, cols], bar[:, cols])
    P = points(case)
    A, arg = reference(P, case.kind, cols)
    return A, arg, entry_bar(P, case.kind, arg)


def point_scale(kind, ell=ELL):
    return 1.0 / (ell * np.sqrt(2.0)) if kind == "gaussian" else C1[kind] / ell


def extent(P, kind, ell=ELL):
    return float((P.max(axis=1) - P.min(axis=1)).max() * point_scale(kind, ell))


def entry_bar(P, kind, arg, ell=ELL):
    E = LD(extent(P, kind, ell))
    delta = E * np.sqrt(2 * arg) if kind == "gaussian" else E
    return 16 * (1 + arg + delta) * U


def fp64_formula(P, kind, cols=None, ell=ELL, sigma2=SIGMA2, nugget=NUGGET):
    """pointcov::kernel's association (csrc/pointcov.hpp) in float64 numpy."""
    n = P.shape[1]
    cols = np.arange(n) if cols is None else np.asarray(cols)
    d2 = np.zeros((n, cols.size))
    for a in range(P.shape[0]):
        t = P[a][:, None] - P[a][cols][None, :]
        d2 += t * t
    inv_ell = 1.0 / ell
    r2 = d2 * inv_ell * inv_ell
    if kind == "gaussian":
        v = np.exp(-0.5 * r2)
    else:
        r = np.sqrt(r2)
        if kind == "exponential":
            v = np.exp(-r)
        elif kind == "matern32":
            a = 1.7320508075688772 * r
            v = (1.0 + a) * np.exp(-a)
        else:
            a = 2.23606797749979 * r
            v = (1.0 + a + a * a * (1.0 / 3.0)) * np.exp(-a)
    v = v * sigma2
    return v + nugget * (np.arange(n)[:, None] == cols[None, :])


def relative_mask(A, sigma2=SIGMA2):
    """Entries that take the relative check (the others: the tail rule)."""
    return A >= TAIL * LD(sigma2)


def check_entries(G, A, arg, bar, sigma2=SIGMA2):
    """The per-entry bar and the tail rule on generated entries G (float64) against (A, arg, bar).  Returns the largest
    |G - A| / (bar A) over the relative entries; raises AssertionError with the worst entry otherwise."""
    rel = relative_mask(A, sigma2)
    Gl = G.astype(LD)
    assert np.isfinite(G).all(), "non-finite entries"
    ratio = np.zeros(A.shape, dtype=LD)
    ratio[rel] = np.abs(Gl[rel] - A[rel]) / (bar[rel] * A[rel])
    worst = float(ratio.max()) if ratio.size else 0.0
    if worst > 1.0:
        i, j = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
        raise AssertionError("entry (%d, column %d): got %r, reference %r, arg %.6g, %.3g x the bar; %d entries over the bar"
                             % (i, j, float(G[i, j]), float(A[i, j]), float(arg[i, j]), worst, int((ratio > 1.0).sum())))
    tail = ~rel
    if tail.any():
        Gt = G[tail]
        assert (Gt >= 0.0).all(), "negative entry in the far tail"
        assert (Gt.astype(LD) <= 2 * TAIL * LD(sigma2)).all(), "far-tail entry above 2^-999 sigma2: %r" % float(Gt.max())
        zero = tail & (arg > 760)
        assert (G[zero] == 0.0).all(), "entry with arg > 760 is not exactly 0: %r" % float(G[zero].max())
    return worst


def agree_entries(G1, G2, A, bar, sigma2=SIGMA2):
    """A X and A' X generate the same entries: they agree within the bar (relative entries) / the tail allowance."""
    rel = relative_mask(A, sigma2)
    diff = np.abs(G1.astype(LD) - G2.astype(LD))
    ratio = np.zeros(A.shape, dtype=LD)
    ratio[rel] = diff[rel] / (bar[rel] * A[rel])
    worst = float(ratio.max()) if ratio.size else 0.0
    assert worst <= 1.0, "A X and A' X differ by %.3g x the bar" % worst
    assert (diff[~rel] <= 2 * TAIL * LD(sigma2)).all()
    return worst


def check_product(Y, X, A, bar, sigma2=SIGMA2):
    """|Y - A X|_ij <= sum_k (K 2^-53 + bar_ik) |A_ik| |X_kj| componentwise, in long double; K = the full reduction length.
    (Far-tail entries enter with their absolute allowance 2^-999 sigma2 in place of bar_ik |A_ik|.)  Returns the largest
    ratio of the left side to the right."""
    K = A.shape[1]
    Xl = X.astype(LD)
    rel = relative_mask(A, sigma2)
    Eb = np.where(rel, bar * np.abs(A), 2 * TAIL * LD(sigma2))
    rhs = (K * U * np.abs(A) + Eb) @ np.abs(Xl)
    lhs = np.abs(Y.astype(LD) - A @ Xl)
    assert np.isfinite(Y).all()
    worst = float((lhs / rhs).max())
    if worst > 1.0:
        i, j = np.unravel_index(int(np.argmax(lhs / rhs)), lhs.shape)
        raise AssertionError("product entry (%d, %d): |Y - A X| = %.3g, %.3g x the bound" % (i, j, float(lhs[i, j]), worst))
    return worst


def check_case(case, run):
    """Both checks of a case.  run: dict with "e<p>" / "et<p>" (A X / A' X of one-hot product p) and "y" / "yt" (of the normal
    panel).  Returns the record of the largest ratios."""
    rec = {"case": case_id(case), "entries": 0.0, "entries_t": 0.0, "mul_vs_mul_t": 0.0, "bit_identical": True}
    for p, base in enumerate(onehot_bases(case)):
        cols = onehot_columns(case, base)
        A, arg, bar = case_reference(case, cols)
        G, Gt = run["e%d" % p], run["et%d" % p]
        assert G.shape == A.shape and Gt.shape == A.shape
        rec["entries"] = max(rec["entries"], check_entries(G, A, arg, bar))
        rec["entries_t"] = max(rec["entries_t"], check_entries(Gt, A, arg, bar))
        rec["mul_vs_mul_t"] = max(rec["mul_vs_mul_t"], agree_entries(G, Gt, A, bar))
        rec["bit_identical"] = rec["bit_identical"] and bool(np.array_equal(G, Gt))
    if has_product_check(case):
        A, arg, bar = case_reference(case)
        X = normal_panel(case)
        rec["product"] = check_product(run["y"], X, A, bar)
        rec["product_t"] = check_product(run["yt"], X, A, bar)
    return rec


def run_case(gsi, ctx, case, rank0=True):
    """The case's products through the library (any backend): the dict check_case takes."""
    out = {}
    op = gsi.pointcov_implicit_operator(ctx, points(case), case.kind, ell=ELL, sigma2=SIGMA2, nugget=NUGGET)
    try:
        for p, base in enumerate(onehot_bases(case)):
            X = onehot(case, base)
            out["e%d" % p], out["et%d" % p] = op.matmul(X), op.rmatmul_t(X)
        if has_product_check(case):
            X = normal_panel(case)
            out["y"], out["yt"] = op.matmul(X), op.rmatmul_t(X)
    finally:
        op.close()
    return out
