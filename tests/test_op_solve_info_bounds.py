"""The `info` arrays of the five conjugate-gradient entry points have different lengths -- `gsi_op_solve_cg` and
`gsi_op_solve` 4, `gsi_op_solve_pcg` and `gsi_op_solve_pcg_host` 6, `gsi_op_solve_trace` 7 -- and all five report through
one helper of csrc/api.cpp.  Callers (kriging.py, the tests) allocate exactly the documented length, so nothing may be
written from that length onward: after a converged solve, after a call refused with GSI_ERR_ARG, after a breakdown.
Once on the CPU reference library (csrc/solvers.cpp's composed path) and once on the device (the fused path)."""
import ctypes as C

import numpy as np
import pytest

import cpuref

SENTINEL = -0x5EED
LENGTH = {"cg": 4, "solve": 4, "pcg": 6, "pcg_host": 6, "trace": 7}
B_COLS = 3
GSI_ERR_ARG, GSI_ERR_NOT_POSDEF = 1, 7
dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int64)


def _call(gsi, ctx, entry, op, pc, B, tol, maxiter=400):
    """One entry point on B with a 12-entry info full of sentinels: (status, info)."""
    lib, n, b = ctx.lib, B.shape[0], B.shape[1]
    info = np.full(12, SENTINEL, dtype=np.int64)
    relres, iters, quad = np.zeros(b), np.zeros(b, dtype=np.int64), np.zeros(2 * b)
    X = np.zeros((n, b), order="F")
    a = lambda v, t=dp: v.ctypes.data_as(t)
    if entry == "solve":
        st = lib.gsi_op_solve(ctx.h, op.h, None, a(B), n, b, a(X), n, tol, maxiter, a(info, ip), a(relres), a(iters, ip))
    elif entry == "pcg_host":
        st = lib.gsi_op_solve_pcg_host(ctx.h, op.h, None, pc.h, a(B), n, b, a(X), n, tol, maxiter, a(info, ip), a(relres),
                                       a(iters, ip))
    else:
        Bd, Xd = gsi.DeviceMatrix.from_host(ctx, B), gsi.DeviceMatrix(ctx, n, b)
        try:
            if entry == "cg":
                st = lib.gsi_op_solve_cg(ctx.h, op.h, None, Bd.h, Xd.h, tol, maxiter, a(info, ip), a(relres), a(iters, ip))
            elif entry == "pcg":
                st = lib.gsi_op_solve_pcg(ctx.h, op.h, None, pc.h, Bd.h, Xd.h, tol, maxiter, a(info, ip), a(relres), a(iters, ip))
            else:
                st = lib.gsi_op_solve_trace(ctx.h, op.h, None, pc.h if pc is not None else None, Bd.h, Xd.h, 1, 64, tol, maxiter,
                                            a(info, ip), a(relres), a(iters, ip), a(quad))
        finally:
            Bd.close()
            Xd.close()
    return st, info


def _check(gsi, ctx, n, path):
    rng = np.random.default_rng(n)
    M = rng.standard_normal((n, n))
    A = np.asfortranarray(M @ M.T / n + np.eye(n))
    lam, V = np.linalg.eigh(A)
    B = np.asfortranarray(rng.standard_normal((n, B_COLS)))
    spd, neg = gsi.dense_operator(ctx, A), gsi.dense_operator(ctx, np.asfortranarray(-np.eye(n)))
    pc = gsi.lowrank_preconditioner(spd, basis=np.asfortranarray(V[:, -4:] * np.sqrt(lam[-4:])), shift=0.5)
    try:
        for entry, length in LENGTH.items():
            p = pc if entry in ("pcg", "pcg_host") else None
            for what, op, tol, status in (("converged", spd, 1e-10, 0), ("refused", spd, 2.0, GSI_ERR_ARG),
                                          ("breakdown", neg, 1e-10, GSI_ERR_NOT_POSDEF)):
                st, info = _call(gsi, ctx, entry, op, p, B, tol)
                print(f"n={n} {entry} {what}: status {st}, info {info.tolist()}")
                assert st == status, (entry, what, st, ctx.lib.gsi_last_error())
                assert (info[length:] == SENTINEL).all(), (entry, what, info.tolist())
                assert (info[:length] != SENTINEL).all(), (entry, what, info.tolist())
                if what == "converged":
                    assert info[1] == B_COLS and info[2] == path and info[3] == 0, (entry, info.tolist())
                if what == "breakdown":
                    assert info[2] == path and 1 <= info[3] <= B_COLS, (entry, info.tolist())
        # the traced solve reports the preconditioned pair's fields also without a preconditioner: kind 0 / 1, rank 0
        for op, status, kind in ((spd, 0, 0), (neg, GSI_ERR_NOT_POSDEF, 1)):
            st, info = _call(gsi, ctx, "trace", op, None, B, 1e-10)
            assert st == status and info[4] == kind and info[5] == 0, (st, info.tolist())
        st, info = _call(gsi, ctx, "trace", spd, pc, B, 1e-10)
        assert st == 0 and info[4] == 0 and info[5] == 4 and (info[7:] == SENTINEL).all(), (st, info.tolist())
    finally:
        pc.close()
        neg.close()
        spd.close()


@pytest.fixture(scope="module")
def cx(gsi):
    c = gsi.Context(0, lib=cpuref.load_cpuref())
    yield c
    c.close()


@pytest.mark.parametrize("n", [33, 34])
def test_info_bounds_cpu(gsi, cx, n):
    _check(gsi, cx, n, 3)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [33, 34])
def test_info_bounds_gpu(gsi, n):
    _check(gsi, gsi.default_context(), n, 1)
