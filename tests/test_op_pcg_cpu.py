"""`gsi_precond_lowrank_create` / `gsi_op_solve_pcg` / `lowrank_preconditioner` / `solve(..., precond=)` on the CPU
reference library: the host driver of solvers.cpp with cg_state.hpp's preconditioned recurrences composed from the
backend's primitives (csrc/block_cg_host.hpp; path 3, "composed"), against numpy.  Cases and checks: tests/pcg_cases.py on
top of tests/solve_cases.py.  tests/test_op_pcg_gpu.py runs the same checks on csrc/block_pcg.hip.
OP_PRECOND_ERRORS=<path>: the largest ratios seen, as profiles/op_precond_errors.json."""
import json
import os

import numpy as np
import pytest

import cpuref
import pcg_cases as pg
import solve_cases as sc

PATH = "composed"
_KEEP = []


@pytest.fixture(scope="module")
def cx(gsi):
    lib = cpuref.load_cpuref()
    c = gsi.Context(0, lib=lib)
    yield c
    c.close()
    path = os.environ.get("OP_PRECOND_ERRORS")
    if path:
        with open(path, "w") as f:
            json.dump({"tol": sc.TOL, "library": "cpu reference, composed path",
                       "bars": {"true_relres_over_tol": 2.0, "solution_error_over_bound": 1.0, "apply_error_over_bar": 1.0},
                       "apply_bar": "4 x the float64 Woodbury restatement's error against the longdouble P^-1 R, floor 1e-13",
                       "largest_apply_error_over_bar": max(pg.APPLY_RATIOS.values(), default=0.0),
                       "apply": pg.APPLY_RATIOS,
                       "solves": {k: v for k, v in sc.RATIOS.items() if k.startswith("pcg")}}, f, indent=1, sort_keys=True)
            f.write("\n")


def test_exported(gsi):
    for name in ("lowrank_preconditioner", "Preconditioner"):
        assert name in gsi.__all__ and callable(getattr(gsi, name)), name
    assert callable(gsi.Preconditioner.apply) and callable(gsi.Preconditioner.close)
    import inspect
    assert "precond" in inspect.signature(gsi.solve).parameters
    assert "precond" in inspect.signature(gsi.Operator.solve).parameters


def test_inputs_are_fair(gsi, cx):
    """On every case used below the numpy restatement at tol 1e-10 ends with a true relative residual <= 1 tol: what
    justifies the 2 tol bar of sc.check_solve."""
    for n, b, diag, K in pg.DENSE + [(1000, 3, "u", 16), (1000, 3, "u", 17)]:
        op, d, A = pg.dense_inputs(gsi, cx, n, diag)
        op.close()
        M = A + (np.diag(d) if d is not None else 0.0)
        Z = pg.eig_basis(A, K)
        pg.fair(f"dense n={n} diag={diag} K={K}", M, sc.rhs(n, min(b, 3), seed=n + b), pg.numpy_pinv(Z, K, d, pg.shift_for(d)),
                10 * n)
    for which in ("pointcov2", "pointcov3", "powerlaw"):
        op, d, A, b = pg.operator_inputs(gsi, cx, which)
        op.close()
        n = A.shape[0]
        pg.fair(which, A + np.diag(d), sc.rhs(n, min(b, 3), seed=n + b), pg.numpy_pinv(pg.eig_basis(A, 8), 8, d, 0.0), 10 * n)
    # another diag; a zero basis; the exact factor of the lowrank case; the large diagonal case of the device file
    op, d, A = pg.dense_inputs(gsi, cx, 257, "vec")
    op.close()
    B = sc.rhs(257, 3, seed=257 + 5)
    pg.fair("another diag", A + np.diag(d), B, pg.numpy_pinv(pg.eig_basis(A, 16), 16, np.full(257, 0.05), 0.01), 2570)
    pg.fair("zero basis", A + np.diag(d), B, lambda r: r / d, 2570)
    op, d = sc.lowrank_case(gsi, cx)
    A = sc.dense_of(op, None)
    op.close()
    Z = pg.eig_basis(A, None, keep=1e-12)
    its = pg.fair("lowrank exact factor", A + np.diag(d), sc.rhs(200, 3, seed=200 + 16), pg.numpy_pinv(Z, Z.shape[1], d, 0.0), 2000)
    assert its.max() <= 2
    n = 128 * 256 + 1
    lam, dd = 1.0 + (np.arange(n) % 5), 0.25 * (1.0 + (np.arange(n) % 2))
    Zr, Zv = np.array([0, n - 1, n // 2]), np.array([1.0, 2.0, 0.5])
    e = 1.0 / dd
    w = e[Zr] * Zv / np.sqrt(1.0 + Zv * Zv * e[Zr])              # Z'EZ is diagonal: one nonzero row per column

    def pinv(r):
        z = e * r
        z[Zr] -= w * (w * r[Zr])
        return z

    class Diag:                                                 # M @ p for the diagonal matrix, without n^2 numbers
        def __matmul__(self, p):
            return (lam + dd) * p
    Bl = sc.rhs(n, 2, seed=1)
    X, its = pg.numpy_pcg(Diag(), Bl, pinv, sc.TOL, 100)
    rho = np.sqrt((((Bl.astype(sc.LD) - (lam + dd)[:, None].astype(sc.LD) * X.astype(sc.LD)) ** 2).sum(axis=0))
                  / (Bl.astype(sc.LD) ** 2).sum(axis=0)).astype(float)
    print(f"large diagonal n={n}: numpy PCG {its} iterations, true relres {rho.max():.3e}")
    assert (rho <= sc.TOL).all() and its.max() <= 13


@pytest.mark.parametrize("n,b,diag,K", pg.DENSE)
def test_dense(gsi, cx, n, b, diag, K):
    pg.dense_solve(gsi, cx, n, b, diag, K, PATH)


@pytest.mark.parametrize("which", ["pointcov2", "pointcov3", "powerlaw"])
def test_operators(gsi, cx, which):
    pg.operator_solve(gsi, cx, which, PATH)


def test_another_diag(gsi, cx):
    pg.other_diag(gsi, cx, PATH)


def test_zero_basis_is_jacobi(gsi, cx):
    pg.zero_basis(gsi, cx, PATH)


def test_exact_factor_converges_at_once(gsi, cx):
    pg.does_its_work_lowrank(gsi, cx, PATH)


def test_rank_64_halves_the_iterations(gsi, cx):
    op, d, A = pg.dense_inputs(gsi, cx, 1000, "u")
    pc = gsi.lowrank_preconditioner(op, basis=pg.eig_basis(A, 64), diag=d)
    try:
        pg.halves_the_iterations(gsi, op, d, pc, PATH, "pcg dense n=1000 K=64 against plain CG")
    finally:
        pc.close()
        op.close()


@pytest.mark.parametrize("n,K,b", pg.APPLY)
def test_apply(gsi, cx, n, K, b):
    pg.apply_case(gsi, cx, n, K, b)


def test_preconditioner_handle(gsi, cx):
    op, d, A = pg.dense_inputs(gsi, cx, 63, 0.1)
    try:
        before = cx.device_bytes()
        with gsi.lowrank_preconditioner(op, basis=pg.eig_basis(A, 5), rank=3, diag=d, shift=0.05) as pc:
            assert pc.rank == 3 and pc.info == {"rank": 3, "n": 63, "diag_min": pc.info["diag_min"], "diag_max": pc.info["diag_max"]}
            assert abs(pc.info["diag_min"] - 0.15) < 1e-15 and abs(pc.info["diag_max"] - 0.15) < 1e-15
            assert cx.device_bytes() == before + 8 * 63 * (3 + 1)       # e and W, nothing else
        assert pc.h is None and cx.device_bytes() == before
        pc.close()                                                       # closing twice is harmless
    finally:
        op.close()


def test_special_columns(gsi, cx):
    pg.special_columns(gsi, cx, PATH)


def test_determinism(gsi, cx):
    pg.determinism(gsi, cx, PATH)


def test_budget(gsi, cx):
    pg.budget(gsi, cx, PATH)


def test_breakdown(gsi, cx):
    pg.breakdown(gsi, cx, PATH)


def test_refusals(gsi, cx):
    other = gsi.Context(0, lib=cx.lib)
    try:
        pg.refusals(gsi, cx, other, PATH)
    finally:
        other.close()


def test_refuses_a_communicator(gsi, monkeypatch):
    lib = cpuref.load_cpuref()
    cbs = (cpuref.ALLREDUCE_FN(lambda buf, count: None),
           cpuref.ALLGATHER_FN(lambda send, recv, count: [recv.__setitem__(i, send[i]) for i in range(count)] and None))
    _KEEP.extend(cbs)                      # the library keeps the pointers
    lib.gsi_cpuref_set_collectives(*cbs)
    monkeypatch.setenv("GSI_FORCE_COMM", "1")
    cc = gsi.Context(0, lib=lib)
    try:
        cc.comm_init(1, 0, b"\0" * 128)
        op = gsi.dense_operator(cc, np.eye(4))
        sc.refused(gsi, lambda: gsi.lowrank_preconditioner(op, basis=np.ones((4, 1)), shift=1.0), "communicator")
        op.close()
    finally:
        cc.close()


def test_kriging_weights_with_drift(gsi, cx):
    P = sc.points(150, 2, seed=21)
    op = gsi.pointcov_implicit_operator(cx, P, kind="exponential", ell=0.3)
    A = sc.dense_of(op, None)
    pc = gsi.lowrank_preconditioner(op, basis=pg.eig_basis(A, 16), diag=0.1)
    try:
        pg.kriging_drift(gsi, cx, op, P, 0.1, pc, "pcg kriging drift, pointcov m=150")
    finally:
        pc.close()
        op.close()
