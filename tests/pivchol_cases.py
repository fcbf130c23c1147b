"""Shared cases and checks of the diagonal-pivoted Cholesky factorization (`gsi_op_pivoted_cholesky`,
`RandMatFact.pivoted_cholesky`, `principal_factor`, `lowrank_preconditioner(method="pivoted_cholesky")`, `getxis_pivchol`)
for tests/test_pivchol_cpu.py (the CPU reference library: the host path of csrc/pivoted_chol_host.hpp, "composed") and
tests/test_pivchol_gpu.py (csrc/pivoted_chol.hip, "fused").  Not a test module.  The reference is tests/pivchol_model.py.

The loop edges of the kernels (csrc/pivoted_chol.hip) that the shapes sit at:
  rows       256 rows per workgroup of the step kernel: n = 255, 256, 257 (and 1, 2, 63, 64, 65: one wave more or less; 1000:
             four workgroups, the last one partly filled);
  columns    the row loop takes 8 earlier columns per trip: K = 33 passes every j from 0 to 32, i.e. no full trip, exactly one
             .. four full trips, and every remainder 0 .. 7; K = 1 never enters it; K = n = 257 ends with d exhausted to rounding;
  partials   the deciding workgroup takes 256 partials per sweep: the 257 x 256 grid has 257 of them;
  ties       a table or point operator has a constant diagonal: the lowest index must win step 0 in every workgroup tree.
"""
import ctypes as C
import os

import numpy as np

import pcg_cases as pg
import pivchol_model as pm
import solve_cases as sc

EPS = np.finfo(np.float64).eps
ERRORS = {}       # case name -> the attained figures, for profiles/pivchol_errors.json

# (n, K) for dense operators; (nx, ny, K) for caller-table operators
DENSE = [(1, 1), (2, 1), (2, 2), (63, 33), (64, 33), (65, 33), (255, 33), (256, 33), (257, 33), (257, 257), (1000, 1), (1000, 33)]
TABLE = [(1, 1, 1), (3, 21, 33), (8, 8, 33), (5, 13, 33), (16, 16, 33), (257, 1, 33), (40, 25, 33)]
TABLE_MANY_PARTIALS = (257, 256, 8)


class composed_path:
    """GSI_PCHOL_COMPOSED=1 for the calls inside (the library reads it at every call)."""

    def __enter__(self):
        self.old = os.environ.get("GSI_PCHOL_COMPOSED")
        os.environ["GSI_PCHOL_COMPOSED"] = "1"

    def __exit__(self, *exc):
        if self.old is None:
            del os.environ["GSI_PCHOL_COMPOSED"]
        else:
            os.environ["GSI_PCHOL_COMPOSED"] = self.old


def dense_matrix(n):
    """An exponential covariance (ell = 0.3) of n random points in the unit square: positive definite, distinct entries."""
    return np.asfortranarray(sc.expcov(sc.points(n, 2, seed=n)))


def table_of(nx, ny, ell=3.0):
    dx, dy = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
    return np.exp(-np.sqrt(dx * dx + dy * dy) / ell)


def factor(gsi, op, K, tol=0.0):
    """(L on the host, piv, info)."""
    Ld, piv, rep = gsi.pivoted_cholesky(op, K, tol, return_info=True)
    try:
        return Ld.to_host(), piv, rep
    finally:
        Ld.close()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def check_against_model(name, got, ref, path):
    L, piv, rep = got
    assert rep["path"] == path, rep
    assert rep["rank"] == ref["rank"] and rep["reason"] == ref["reason"], (name, rep, ref["rank"], ref["reason"])
    assert np.array_equal(piv, ref["piv"]), (name, piv, ref["piv"])
    assert same_bits(L, ref["L"]), (name, np.abs(L - ref["L"]).max())
    assert rep["trace0"] == ref["trace0"] or abs(rep["trace0"] - ref["trace0"]) <= 4 * L.shape[0] * EPS * ref["trace0"]
    assert abs(rep["trace"] - ref["trace"]) <= 4 * L.shape[0] * EPS * ref["trace0"], (name, rep["trace"], ref["trace"])
    assert rep["dmax"] == ref["dmax"], (name, rep["dmax"], ref["dmax"])


# ---------------------------------------------------------------- bit parity
def parity_dense(gsi, ctx, n, K, path, also_composed=False):
    """Pivots and L equal to the model's bit for bit; two calls equal; on the device the composed leg equals the fused one."""
    A = dense_matrix(n)
    ref = pm.pivchol(*pm.matrix_source(A), K)
    op = gsi.dense_operator(ctx, A)
    try:
        got = factor(gsi, op, K)
        check_against_model(f"dense n={n} K={K}", got, ref, path)
        assert got[2]["form"] == "stored" and got[2]["polls"] >= (1 if path == "fused" else 0)
        again = factor(gsi, op, K)
        assert same_bits(got[0], again[0]) and np.array_equal(got[1], again[1]) and got[2] == again[2]
        if also_composed:
            with composed_path():
                leg = factor(gsi, op, K)
            assert leg[2]["path"] == "composed"
            assert same_bits(got[0], leg[0]) and np.array_equal(got[1], leg[1])
            assert (leg[2]["rank"], leg[2]["reason"], leg[2]["dmax"]) == (got[2]["rank"], got[2]["reason"], got[2]["dmax"])
    finally:
        op.close()


def parity_table(gsi, ctx, nx, ny, K, path, also_composed=False):
    T = table_of(nx, ny)
    ref = pm.pivchol(*pm.table_source(T), K)
    assert ref["piv"][0] == 0                                   # the constant diagonal: the lowest index wins
    op = gsi.gridcov_implicit_operator(ctx, nx, ny, 1.0, table=T)
    try:
        got = factor(gsi, op, K)
        check_against_model(f"table {nx}x{ny} K={K}", got, ref, path)
        assert got[2]["form"] == "table"
        again = factor(gsi, op, K)
        assert same_bits(got[0], again[0]) and np.array_equal(got[1], again[1])
        if also_composed:
            with composed_path():
                leg = factor(gsi, op, K)
            assert leg[2]["path"] == "composed"
            assert same_bits(got[0], leg[0]) and np.array_equal(got[1], leg[1])
    finally:
        op.close()


def host_matrix_in_host_factor_out(gsi, ctx, path):
    """randsvd's convention: a host matrix in, a host L out; and the keyword defaults."""
    A = dense_matrix(65)
    L, piv = gsi.pivoted_cholesky(A, 9, ctx=ctx)
    assert isinstance(L, np.ndarray) and L.shape == (65, 9) and piv.shape == (9,) and piv.dtype == np.int64
    ref = pm.pivchol(*pm.matrix_source(A), 9)
    assert same_bits(L, ref["L"]) and np.array_equal(piv, ref["piv"])
    L2, piv2, rep = gsi.RandMatFact.pivoted_cholesky(A, 9, 0.0, return_info=True, ctx=ctx)
    assert same_bits(L, L2) and rep["path"] == path and rep["stopped_by"] == "rank"


# ---------------------------------------------------------------- stopping
def stopping(gsi, ctx, path):
    rng = np.random.default_rng(41)
    B = rng.standard_normal((300, 5))
    A = np.asfortranarray(B @ B.T)
    ref = pm.pivchol(*pm.matrix_source(A), 20, 1e-10)
    print(f"B B' 300 x 5, K = 20, tol = 1e-10: model rank {ref['rank']}, reason {ref['reason']}, "
          f"final trace {ref['trace'] / ref['trace0']:.2e} of trace_0")
    assert (ref["rank"], ref["reason"]) == (5, 2)
    L, piv, rep = gsi.pivoted_cholesky(A, 20, 1e-10, return_info=True, ctx=ctx)
    assert (rep["rank"], rep["reason"], rep["path"]) == (5, 2, path), rep
    assert len(piv) == 5 and np.array_equal(piv, ref["piv"]) and same_bits(L, ref["L"])
    assert not L[:, 5:].any()                                   # columns rank .. K - 1 are zeros
    assert rep["trace"] <= 1e-10 * rep["trace0"]
    # tol = 0 with K reached
    L, piv, rep = gsi.pivoted_cholesky(dense_matrix(64), 7, 0.0, return_info=True, ctx=ctx)
    assert (rep["rank"], rep["reason"]) == (7, 1), rep
    # rank 3, 40 x 40
    B3 = rng.standard_normal((40, 3))
    A3 = np.asfortranarray(B3 @ B3.T)
    L, piv, rep = gsi.pivoted_cholesky(A3, 3, 0.0, return_info=True, ctx=ctx)
    assert (rep["rank"], rep["reason"]) == (3, 1), rep
    assert np.abs(A3 - L @ L.T).max() <= 64 * EPS * np.abs(A3).max()
    L, piv, rep = gsi.pivoted_cholesky(A3, 10, 1e-12, return_info=True, ctx=ctx)
    assert (rep["rank"], rep["reason"]) == (3, 2), rep
    # a zero matrix
    L, piv, rep = gsi.pivoted_cholesky(np.zeros((17, 17)), 4, 0.0, return_info=True, ctx=ctx)
    assert (rep["rank"], rep["reason"], rep["stopped_by"]) == (0, 3, "exhausted") and len(piv) == 0 and not L.any()
    assert rep["trace0"] == 0.0 and rep["dmax"] == 0.0
    # one NaN on the diagonal
    An = dense_matrix(40)
    An[7, 7] = float("nan")
    try:
        gsi.pivoted_cholesky(An, 4, ctx=ctx)
    except gsi.GsiError as e:
        assert e.code == 7 and "step 0" in str(e), e
    else:
        raise AssertionError("a NaN on the diagonal must return GSI_ERR_NOT_POSDEF")
    # an infinity off the diagonal is met in the column of its step (the composed path meets it one step earlier: its
    # columns are products with a unit vector, and 0 x inf is a NaN in the rows that hold it)
    Ai = dense_matrix(40)
    ref = pm.pivchol(*pm.matrix_source(Ai), 4)
    p1 = int(ref["piv"][1])
    q = (p1 + 1) % 40 if (p1 + 1) % 40 != int(ref["piv"][0]) else (p1 + 2) % 40
    Ai[q, p1] = Ai[p1, q] = float("inf")
    try:
        gsi.pivoted_cholesky(Ai, 4, ctx=ctx)
    except gsi.GsiError as e:
        assert e.code == 7 and ("step 1" if path == "fused" else "step 0") in str(e), e
    else:
        raise AssertionError("an infinity in a pivot column must return GSI_ERR_NOT_POSDEF")
    parity_dense(gsi, ctx, 63, 33, path)                        # the context is as good as before


# ---------------------------------------------------------------- refusals
def refusals(gsi, ctx, other_ctx):
    """Every refusal by message fragment, with nothing allocated on the way."""
    n = 12
    A = dense_matrix(n)
    op = gsi.dense_operator(ctx, A)
    rect = gsi.dense_operator(ctx, np.ones((n, n + 1)))
    big = gsi.gridcov_implicit_operator(ctx, 50, 41, 3.0, kind=1)       # n = 2050
    fft = gsi.fft_powerlaw_operator(ctx, [12, 9], -3.5)
    lowrank, _ = sc.lowrank_case(gsi, ctx)
    opo = gsi.dense_operator(other_ctx, A)
    Lok = gsi.DeviceMatrix(ctx, n, 6)
    Lrows = gsi.DeviceMatrix(ctx, n + 1, 6)
    Lbig = gsi.DeviceMatrix(ctx, 2050, 2049)
    Lfft = gsi.DeviceMatrix(ctx, 108, 4)
    Llow = gsi.DeviceMatrix(ctx, 200, 4)
    Lother = gsi.DeviceMatrix(other_ctx, n, 6)
    lib = ctx.lib

    def call(o, K, tol, L, cx=ctx):
        piv = np.zeros(max(int(K), 1), dtype=np.int64)
        info = (C.c_int64 * 6)()
        st = lib.gsi_op_pivoted_cholesky(cx.h, o.h, int(K), float(tol), L.h, piv.ctypes.data_as(C.POINTER(C.c_int64)), info, None)
        if st != 0:
            raise gsi.GsiError(st, lib.gsi_last_error().decode())
    try:
        before = ctx.device_bytes()
        for K in (0, -1):
            sc.refused(gsi, lambda: call(op, K, 0.0, Lok), "K must be at least 1")
        sc.refused(gsi, lambda: call(op, n + 1, 0.0, Lok), "K exceeds the size of op")
        sc.refused(gsi, lambda: call(big, 2049, 0.0, Lbig), "K exceeds 2048")
        sc.refused(gsi, lambda: call(op, 7, 0.0, Lok), "K exceeds the columns of L")
        sc.refused(gsi, lambda: call(op, 3, 0.0, Lrows), "L must have size(op, 1)")
        for t in (-1e-300, 1.0, 2.0, float("nan"), float("inf")):
            sc.refused(gsi, lambda: call(op, 3, t, Lok), "tol must lie in [0, 1)")
        sc.refused(gsi, lambda: call(op, 3, 0.0, Lother), "L belongs to another context")
        sc.refused(gsi, lambda: call(opo, 3, 0.0, Lok), "op belongs to another context")
        sc.refused(gsi, lambda: call(rect, 3, 0.0, Lok), "not square")
        for o, Lo in ((fft, Lfft), (lowrank, Llow)):
            sc.refused(gsi, lambda: call(o, 3, 0.0, Lo), "use randsvd")
            sc.refused(gsi, lambda: call(o, 3, 0.0, Lo), "dense, an implicit grid-covariance or an implicit point-covariance")
        assert ctx.device_bytes() == before                      # nothing was allocated on the way to a refusal
        call(op, 6, 0.0, Lok)                                    # a following valid call succeeds
        assert same_bits(Lok.to_host(), pm.pivchol(*pm.matrix_source(A), 6)["L"])
        # the Python faces
        for bad in (0, n + 1):
            try:
                gsi.pivoted_cholesky(op, bad)
            except ValueError:
                pass
            else:
                raise AssertionError("K out of range must raise")
        sc.refused(gsi, lambda: gsi.pivoted_cholesky(fft, 3), "use randsvd")
        try:
            gsi.lowrank_preconditioner(op, rank=3, shift=0.1, method="cholesky")
        except ValueError:
            pass
        else:
            raise AssertionError("an unknown method must raise")
    finally:
        for h in (op, rect, big, fft, lowrank, opo, Lok, Lrows, Lbig, Lfft, Llow, Lother):
            h.close()


# ---------------------------------------------------------------- scattered points
# kind, d, nugget, the seed of the points (a seed is replaced when the fixture conditions below do not hold)
SCATTERED = [("exponential", 2, 0.0, 1), ("exponential", 3, 0.01, 2), ("matern52", 2, 0.01, 3), ("matern52", 3, 0.0, 7)]      # (seed 4: gap 1.9e-7)


def ulp_moves(n, p, seed):
    """The move of the entries of column p in ulp: an integer in [-2, 2] for every row, a function of the unordered pair
    {i, p} alone (so the perturbed matrix is symmetric), 0 on the diagonal."""
    i = np.arange(n, dtype=np.uint64)
    lo, hi = np.minimum(i, np.uint64(p)), np.maximum(i, np.uint64(p))
    h = (lo * np.uint64(n) + hi + np.uint64(seed)) * np.uint64(0x9E3779B97F4A7C15)          # (wraps modulo 2^64)
    h ^= h >> np.uint64(29)
    h *= np.uint64(0xBF58476D1CE4E5B9)
    h ^= h >> np.uint64(32)
    k = (h % np.uint64(5)).astype(np.int64) - 2
    k[p] = 0
    return k


def identities(Acols, diagA, L, piv, d):
    """max |A[:, piv] - L L[piv, :]'| and max |diag(A - L L') - d|; Acols = A[:, piv]."""
    r = len(piv)
    Lr = L[:, :r]
    e1 = float(np.abs(Acols - Lr @ Lr[piv, :].T).max()) if r else 0.0
    e2 = float(np.abs((diagA - (Lr * Lr).sum(axis=1)) - d).max())
    return e1, e2


def scattered(gsi, ctx, kind, d, nugget, seed, path, n=1000, K=64):
    """Against the model run on the operator's own matrix (op_mul on the identity, which is exact; taken column by column
    as the model asks for them, the diagonal being the one value k(0) + nugget): equal pivots; L within 4 x (the change
    of the model's L under a +-2 ulp perturbation of the off-diagonal entries) relative to max |L| -- the column kernel and
    the tile loader of the product may round an entry differently by a couple of ulp; the two identities within 8 x what
    the model attains on the same matrix (floor 16 eps max A)."""
    P = sc.points(n, d, seed=seed)
    op = gsi.pointcov_implicit_operator(ctx, P, kind=kind, ell=0.3, nugget=nugget)
    try:
        cols = {}

        def column(p):
            if p not in cols:
                e = np.zeros(n)
                e[p] = 1.0
                cols[p] = op.matmul(e)
            return cols[p]

        def moved(p):
            c = column(p)
            return c + ulp_moves(n, p, seed) * np.spacing(c)
        diagA = np.full(n, column(0)[0])
        ref = pm.pivchol(column, diagA, K)
        alt = pm.pivchol(moved, diagA, K)
        # the conditions on the fixture
        gap = float(ref["gaps"][1:].min())
        assert gap >= 1e-7, f"fixture: smallest gap between the two largest d {gap:.2e}; take another seed"
        assert np.array_equal(alt["piv"], ref["piv"]), "fixture: the perturbed model run moved a pivot; take another seed"
        assert ref["piv"][0] == 0 and ref["rank"] == K
        Acols = np.column_stack([cols[p] for p in ref["piv"]])
        assert np.array_equal(Acols[ref["piv"], :], Acols[ref["piv"], :].T)           # symmetric where it was read
        assert (Acols[ref["piv"], np.arange(K)] == diagA[0]).all()                     # the diagonal is one value
        scale = np.abs(ref["L"]).max()
        bar = 4.0 * float(np.abs(alt["L"] - ref["L"]).max()) / scale
        assert bar > 0.0
        L, piv, rep = factor(gsi, op, K)
        assert (rep["path"], rep["form"], rep["rank"], rep["reason"]) == (path, "points", K, 1), rep
        assert np.array_equal(piv, ref["piv"]), (piv, ref["piv"])
        err = float(np.abs(L - ref["L"]).max()) / scale
        dl = pm.diag_from_factor(diagA, L, piv)
        m1, m2 = identities(Acols, diagA, ref["L"], ref["piv"], ref["d"])
        e1, e2 = identities(Acols, diagA, L, piv, dl)
        amax = max(np.abs(Acols).max(), diagA[0])
        floor = 16 * EPS * amax
        name = f"pointcov {kind} d={d} nugget={nugget}"
        print(f"{name}: smallest gap {gap:.2e}; max|dL|/max|L| {err:.3e}, bar {bar:.3e}; pivot columns {e1:.3e} "
              f"(model {m1:.3e}), diagonal {e2:.3e} (model {m2:.3e}), floor {floor:.3e}")
        ERRORS[name] = {"L_error": err, "L_bar": bar, "pivot_columns": e1, "pivot_columns_model": m1, "diagonal": e2,
                        "diagonal_model": m2, "floor": floor, "smallest_gap": gap}
        assert err <= bar, (err, bar)
        assert e1 <= max(8 * m1, floor), (e1, m1)
        assert e2 <= max(8 * m2, floor), (e2, m2)
        # err_out is the trace and the maximum of that d
        assert abs(rep["trace"] - np.maximum(dl, 0).sum()) <= 4 * n * EPS * rep["trace0"]
        assert abs(rep["dmax"] - dl.max()) <= 64 * EPS * amax
    finally:
        op.close()


def identities_dense_table(gsi, ctx, path):
    """The two identities where L is the model's bit for bit: against the model's own value on the same matrix."""
    for name, A, make in (("dense n=257", dense_matrix(257), lambda: gsi.dense_operator(ctx, dense_matrix(257))),
                          ("table 8x8", None, lambda: gsi.gridcov_implicit_operator(ctx, 8, 8, 1.0, table=table_of(8, 8)))):
        op = make()
        try:
            if A is None:
                A = np.asfortranarray(op.matmul(np.eye(64)))
            K = 33
            ref = pm.pivchol(*pm.matrix_source(A), K)
            L, piv, rep = factor(gsi, op, K)
            assert rep["path"] == path and np.array_equal(piv, ref["piv"])
            dl = pm.diag_from_factor(np.diag(A), L, piv)
            m1, m2 = identities(A[:, ref["piv"]], np.diag(A), ref["L"], ref["piv"], ref["d"])
            e1, e2 = identities(A[:, piv], np.diag(A), L, piv, dl)
            floor = 16 * EPS * np.abs(A).max()
            print(f"{name}: pivot columns {e1:.3e} (model {m1:.3e}), diagonal {e2:.3e} (model {m2:.3e})")
            ERRORS[name] = {"pivot_columns": e1, "pivot_columns_model": m1, "diagonal": e2, "diagonal_model": m2, "floor": floor}
            assert e1 <= max(8 * m1, floor) and e2 <= max(8 * m2, floor)
            assert same_bits(dl, ref["d"])
        finally:
            op.close()


def large_rank(gsi, ctx, path, n=2304, K=2048):
    """The two identities at K = 2048 against numpy's A - L L', not the model.  The bar: an entry of L L[piv, :]' is a sum of at
    most K products, sum_c |L_ic L_pc| <= sqrt(A_ii A_pp) <= max A because sum_c L_ic^2 <= A_ii; the factorization rounds each
    of them and each partial sum once, and numpy's product of the same numbers does so again: 2 (K + 2) eps max A."""
    A = np.asfortranarray(sc.expcov(sc.points(n, 2, seed=n)) + 0.1 * np.eye(n))
    op = gsi.dense_operator(ctx, A)
    try:
        L, piv, rep = factor(gsi, op, K)
        assert (rep["path"], rep["rank"], rep["reason"]) == (path, K, 1), rep
        assert len(set(piv.tolist())) == K and piv.min() >= 0 and piv.max() < n
        dl = pm.diag_from_factor(np.diag(A), L, piv)
        e1, e2 = identities(A[:, piv], np.diag(A), L, piv, dl)
        bar = 2 * (K + 2) * EPS * np.abs(A).max()
        print(f"dense n={n} K={K}: pivot columns {e1:.3e}, diagonal {e2:.3e}, bar {bar:.3e}; final trace "
              f"{rep['trace'] / rep['trace0']:.3e} of trace_0")
        ERRORS[f"dense n={n} K={K}"] = {"pivot_columns": e1, "diagonal": e2, "bar": bar}
        assert e1 <= bar and e2 <= bar
        assert (dl >= -bar).all() and np.abs(dl[piv]).max() <= bar       # (a pivot's d is zeroed at its step; later steps round around it)
        assert abs(rep["dmax"] - dl.max()) == 0.0
    finally:
        op.close()


# ---------------------------------------------------------------- on top
def preconditioner(gsi, ctx, path, n=2000):
    """`lowrank_preconditioner(op, rank=64, method="pivoted_cholesky", diag=d)` on a point covariance: the solvers' bars
    (true residual <= 2 tol at tol = 1e-10) and strictly fewer iterations than plain CG in every column."""
    P = sc.points(n, 2, seed=17)
    op = gsi.pointcov_implicit_operator(ctx, P, kind="exponential", ell=0.3)
    d = 0.01 * (1.0 + np.random.default_rng(11).random(n))
    # the factor is dropped: a second create / close cycle leaves the device memory account where the first left it (the
    # device backend keeps released blocks for reuse and counts them, so the first cycle fills that cache)
    gsi.lowrank_preconditioner(op, rank=64, method="pivoted_cholesky", diag=d).close()
    before = ctx.device_bytes()
    gsi.lowrank_preconditioner(op, rank=64, method="pivoted_cholesky", diag=d).close()
    assert ctx.device_bytes() == before
    pc = gsi.lowrank_preconditioner(op, rank=64, method="pivoted_cholesky", diag=d)
    try:
        assert pc.rank == 64 and pc.n == n
        X, rep, B = pg.run_case(gsi, op, d, 3, pc, f"pcg pointcov n={n}, pivoted Cholesky rank 64", path)
        _, plain = op.solve(B, diag=d, tol=sc.TOL, return_info=True)
        print(f"pivoted Cholesky rank 64, n={n}: iterations {rep['iters']}, plain CG {plain['iters']}")
        assert (rep["iters"] < plain["iters"]).all(), (rep["iters"], plain["iters"])
    finally:
        pc.close()
    # fewer columns by tol: the rank that was reached is reported
    pc = gsi.lowrank_preconditioner(op, rank=64, method="pivoted_cholesky", diag=d, tol=0.5)
    try:
        assert 1 <= pc.rank < 64, pc.rank
    finally:
        pc.close()
        op.close()


def principal(gsi, ctx):
    """Z Z' = L L' and Z'Z diagonal, to the bars tests/test_jacobi_svd_gpu.py:check_bars holds the tall SVD to (1e-11)."""
    A = dense_matrix(257)
    op = gsi.dense_operator(ctx, A)
    Ld, piv, rep = gsi.pivoted_cholesky(op, 33, return_info=True)
    try:
        Zd, s = gsi.principal_factor(Ld)
        assert isinstance(Zd, gsi.DeviceMatrix) and Zd.shape == (257, 33) and s.shape == (33,)
        Z, L = Zd.to_host(), Ld.to_host()
        Zd.close()
        G = L @ L.T
        assert np.linalg.norm(Z @ Z.T - G) <= 1e-11 * np.linalg.norm(G)
        assert (np.diff(s) <= 0).all() and (s > 0).all()
        V = Z / s
        assert np.abs(V.T @ V - np.eye(33)).max() < 1e-11
        assert np.abs(s - np.linalg.svd(L, compute_uv=False)).max() <= 1e-12 * s[0]
        # a host matrix in, a host matrix out; fewer columns
        Zh, sh = gsi.principal_factor(L, 5, ctx=ctx)
        G5 = L[:, :5] @ L[:, :5].T
        assert isinstance(Zh, np.ndarray) and Zh.shape == (257, 5)
        assert np.linalg.norm(Zh @ Zh.T - G5) <= 1e-11 * np.linalg.norm(G5)
    finally:
        Ld.close()
        op.close()


def pcga_end_to_end(gsi, ctx, M, N, mu, principal_form):
    """tests/test_gpu_parity.py:test_pcga_end_to_end with the basis from `getxis_pivchol`, within that test's own 2e-2."""
    import scipy.sparse as sp
    rng = np.random.default_rng(2017 + M + N)
    x = rng.standard_normal(N)
    Q0 = rng.standard_normal((M, N))
    Q = Q0.T @ Q0
    w, V = np.linalg.eigh(Q)
    truep = (V * np.sqrt(np.clip(w, 0, None))) @ V.T @ rng.standard_normal(N) + mu
    forward = lambda pv: pv * x
    basis = gsi.getxis_pivchol(Q, M, principal=principal_form, ctx=ctx)
    try:
        assert isinstance(basis, gsi.DeviceBasis) and basis.K == M and basis.n == N
        X = np.full(N, float(mu))
        noise = 1e-4
        R = noise ** 2 * sp.identity(N, format="csc")
        yobs = forward(truep) + noise * rng.standard_normal(N)
        popt = gsi.pcgadirect(forward, X.copy(), X, basis, R, yobs)
        err = np.linalg.norm(popt - truep) / np.linalg.norm(truep)
        print(f"pcgadirect on getxis_pivchol (M={M}, N={N}, principal={principal_form}): error {err:.3e}")
        assert err < 2e-2
    finally:
        basis.close()
