"""FFTRF fields at scattered points on the GPU (csrc/fftrf_points.hpp, csrc/fftrf_interp.hip; `gsi_fftrf_interpolate`,
`gsi_fftrf_fields_at`, `gsi_op_lowrank_fftrf_at`).

1. `gsi_fftrf_interpolate` against the numpy restatement (tests/fftrf_interp_model.py), BIT FOR BIT: the planner and the
   kernel perform the model's IEEE operations one by one (no fused multiply-add), so no tolerance is needed.
2. `gsi_fftrf_fields_at` = `gsi_fftrf_fields` followed by `gsi_fftrf_interpolate`, bit for bit (phi and seed mode).
3. Against the oracle: fm.oracle_field interpolated by the model.  Bar
       max |F - F_ref| <= fm.BAR max |F_ref - k0| + 8 d eps max |F_ref|:
   the sampler's own bar carried through a convex combination, plus the combination's own rounding.
4. A field's bits do not depend on the batch it rides in.
5. The operator over such fields: samples, products, getxis.
6. Two ranks: each holds exactly its rows, with the extrema taken over ALL points.
7. Refusals through the C ABI: GSI_ERR_ARG naming the limit, nothing allocated."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import fftrf_interp_model as im
import fftrf_model as fm
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EPS = np.finfo(np.float64).eps


@pytest.fixture(scope="module")
def ctx(gsi):
    return gsi.default_context()


def _host(M):
    try:
        return M.to_host()
    finally:
        M.close()


def _interp(gsi, ctx, P, G, Ns, **kw):
    return _host(gsi.FFTRF.interpolate(ctx, P, G, Ns, **kw))


# ---- 1. the interpolation kernel against the model, bit for bit --------------------------------------------------------
@pytest.mark.parametrize("Ns", im.GRIDS, ids=im.gid)
def test_interpolate_equals_the_model_bit_for_bit(gsi, ctx, Ns):
    """Every point count x field count; duplicated points and points at both extrema of every axis are in the set
    (im.scattered_points); with the points' own extrema (m >= 2: one point has no extent) and with a box inside them."""
    grids = {nf: im.random_fields(Ns, nf, seed=2) for nf in im.FIELD_COUNTS}
    dev = {nf: gsi.DeviceMatrix.from_host(ctx, V) for nf, V in grids.items()}
    try:
        for m in im.POINT_COUNTS:
            P = im.scattered_points(Ns, m, seed=9)
            boxes = [im.inner_box(P)] + ([None] if m >= 2 else [])
            for box in boxes:
                base, frac = im.plan(P, Ns, box)
                if m >= 4:
                    assert (frac == 0.0).any() and (frac == 1.0).any()        # the extrema / the clamp are exercised
                for nf in im.FIELD_COUNTS:
                    got = _interp(gsi, ctx, P, dev[nf], Ns, box=box)
                    assert got.shape == (m, nf)
                    assert np.array_equal(got, im.interp(grids[nf], Ns, base, frac)), (m, nf, box is not None)
    finally:
        for M in dev.values():
            M.close()


@pytest.mark.parametrize("Ns", im.GRIDS, ids=im.gid)
def test_interpolate_at_the_nodes_returns_the_field(gsi, ctx, Ns):
    V = im.random_fields(Ns, 3, seed=4)
    for scale, shift in ((1.0, 0.0), (0.25, 1024.0)):
        assert np.array_equal(_interp(gsi, ctx, im.node_points(Ns, scale, shift), V, Ns), V), (scale, shift)


def test_interpolate_with_several_field_groups_per_workgroup(gsi, ctx):
    """20001 points, 131 fields: 79 workgroups of points leave 26 slices of the fields, so a workgroup walks two groups of
    four fields (the smaller cases above give every workgroup one group) and the last slice only the three left over."""
    Ns, m, nf = (25, 37), 20001, 131
    V = im.random_fields(Ns, nf, seed=7)
    P = im.scattered_points(Ns, m, seed=3)
    assert np.array_equal(_interp(gsi, ctx, P, V, Ns), im.interpolate(P, V, Ns))


def test_interpolate_row_shards_use_the_extrema_of_all_points(gsi, ctx):
    Ns = (6, 4, 5)
    V = im.random_fields(Ns, 3, seed=4)
    P = im.scattered_points(Ns, 257, seed=1)
    whole = im.interpolate(P, V, Ns)
    for row0, rows in ((0, 100), (101, 156), (256, 1)):
        got = _interp(gsi, ctx, P, V, Ns, row0=row0, rows=rows)
        assert np.array_equal(got, whole[row0:row0 + rows]), (row0, rows)


# ---- 2. the sampler path equals the two-step path ----------------------------------------------------------------------
@pytest.mark.parametrize("Ns", [(25, 25), (6, 4, 5)], ids=im.gid)
def test_fields_at_equals_fields_then_interpolate(gsi, ctx, Ns):
    F = gsi.FFTRF
    nf, args, seed = 5, (2.0, 3.14, -3.5), 20170301
    rng = np.random.default_rng(8)
    phi = [rng.standard_normal(F.phi_shape(Ns)) for _ in range(nf)]
    P = im.scattered_points(Ns, 300, seed=6)
    nodes = im.node_points(Ns, 0.25, 1024.0)
    for kw in ({"phi": phi}, {"seed": seed}):
        S = F.powerlaw_fields(ctx, Ns, *args, nf, **kw)
        try:
            H = S.to_host()
            for pts, box in ((P, None), (P, im.inner_box(P)), (nodes, None)):
                two_step = _interp(gsi, ctx, pts, S, Ns, box=box)
                one_step = _host(F.powerlaw_fields_at(ctx, pts, Ns, *args, nf, box=box, **kw))
                assert np.array_equal(one_step, two_step), (list(kw), box is not None)
                assert np.array_equal(one_step, im.interpolate(pts, H, Ns, box))
            assert np.array_equal(one_step, H)                           # node points: the structured fields themselves
        finally:
            S.close()


# ---- 3. against the oracle ---------------------------------------------------------------------------------------------
ORACLE_CASES = [fm.Case((25, 25), k0=2.0, dk=3.14), fm.Case((3, 9)), fm.Case((7, 11)), fm.Case((6, 4, 5)), fm.Case((2, 300, 2))]


@pytest.mark.parametrize("case", ORACLE_CASES, ids=[c.id for c in ORACLE_CASES])
def test_fields_at_match_the_interpolated_oracle(gsi, ctx, case):
    phi = case.phi()
    P = im.scattered_points(case.Ns, 300, seed=12)
    got = _host(gsi.FFTRF.powerlaw_fields_at(ctx, P, case.Ns, case.k0, case.dk, case.beta, case.nfields, phi=phi))
    assert got.shape == (300, case.nfields)
    d = len(case.Ns)
    for c, ph in enumerate(phi):
        ref = im.interpolate(P, fm.oracle_field(case.Ns, case.k0, case.dk, case.beta, ph), case.Ns)[:, 0]
        err = np.abs(got[:, c] - ref).max()
        bar = fm.BAR * np.abs(ref - case.k0).max() + 8 * d * EPS * np.abs(ref).max()
        print(case.id, c, "error", err, "bar", bar)
        assert np.isfinite(got[:, c]).all() and err <= bar


@pytest.mark.parametrize("N", [2, 3])
def test_powerlaw_unstructuredgrid_returns_one_value_per_point(gsi, ctx, N):
    """The reference's own test (testfftrf.jl:17-25): length(k) == size(points, 2)."""
    rng = np.random.default_rng(2017 + N)
    points = rng.standard_normal((N, 100))
    Ns = [int(round(25 * (1 + x))) for x in rng.random(N)]
    k0, dk, beta = rng.standard_normal(), rng.random(), -2 - rng.random()
    gsi.RandMatFact.seed(3)
    k = gsi.FFTRF.powerlaw_unstructuredgrid(points, Ns, k0, dk, beta, ctx=ctx)
    assert k.shape == (100,) and np.isfinite(k).all()
    gsi.RandMatFact.seed(3)
    grid = gsi.FFTRF.powerlaw_structuredgrid(Ns, k0, dk, beta, ctx=ctx)
    assert np.array_equal(k, im.interpolate(points, grid, Ns)[:, 0])
    ks = gsi.FFTRF.powerlaw_unstructuredgrid(points, Ns, k0, dk, beta, seed=5, ctx=ctx)
    assert np.array_equal(ks, im.interpolate(points, gsi.FFTRF.powerlaw_structuredgrid(Ns, k0, dk, beta, seed=5, ctx=ctx), Ns)[:, 0])


# ---- 4. independence of batching ---------------------------------------------------------------------------------------
def test_a_field_at_points_does_not_depend_on_its_batch(gsi, ctx, monkeypatch):
    Ns, nf, args, seed = fm.BATCH_CASE.Ns, fm.BATCH_CASE.nfields, (0.0, 1.0, -3.5), 77
    P = im.scattered_points(Ns, 40, seed=2)

    def fields(n, field0=0):
        return _host(gsi.FFTRF.powerlaw_fields_at(ctx, P, Ns, *args, n, seed=seed, field0=field0))

    monkeypatch.delenv("GSI_FFTRF_BATCH", raising=False)
    whole = fields(nf)
    assert whole.shape == (40, nf)
    monkeypatch.setenv("GSI_FFTRF_BATCH", "7")
    assert np.array_equal(fields(nf), whole)
    monkeypatch.delenv("GSI_FFTRF_BATCH")
    for f in (0, 6, 7, 130):
        assert np.array_equal(fields(1, field0=f)[:, 0], whole[:, f]), f
    assert not np.array_equal(whole[:, 0], whole[:, 1])


# ---- 5. the operator ---------------------------------------------------------------------------------------------------
OP_ARGS = ((25, 25), 2.0, 3.14, -3.5, 24)
OP_SEED = 4242


def _op_points():
    return im.scattered_points(OP_ARGS[0], 400, seed=21)


@pytest.fixture(scope="module")
def op_fields(gsi, ctx):
    Ns, k0, dk, beta, nf = OP_ARGS
    return _host(gsi.FFTRF.powerlaw_fields_at(ctx, _op_points(), Ns, k0, dk, beta, nf, seed=OP_SEED))      # 400 x 24


def test_operator_samples_are_the_centred_fields_at_the_points(gsi, ctx, op_fields):
    op = gsi.lowrank_fftrf_operator(ctx, *OP_ARGS, seed=OP_SEED, points=_op_points())
    lr = gsi.LowRankCovMatrix(op_fields.T, ctx=ctx)
    try:
        assert op.shape == (400, 400)
        assert np.array_equal(gsi.device_samples(op, 24), lr.samples)
    finally:
        op.close(); lr.close()


def test_operator_product_matches_the_oracle(gsi, ctx, op_fields):
    op = gsi.lowrank_fftrf_operator(ctx, *OP_ARGS, seed=OP_SEED, points=_op_points())
    try:
        X = np.random.default_rng(3).standard_normal((400, 7))
        ref = orc.LowRankCovMatrix(op_fields.T)
        full = ref.samples.T @ ref.samples / (24 - 1)
        Y = op.matmul(X)
        err = np.abs(Y - full @ X).max() / np.abs(full @ X).max()
        print("product", err)
        assert err < 1e-10
    finally:
        op.close()


def test_getxis_fftrf_at_points_matches_getxis_on_the_same_fields(gsi, ctx):
    Ns, k0, dk, beta, nf = OP_ARGS
    P = _op_points()
    H = _host(gsi.FFTRF.powerlaw_fields_at(ctx, P, Ns, k0, dk, beta, nf, seed=0))
    Om = np.random.default_rng(0).standard_normal((400, 15))
    xis = gsi.getxis_fftrf(Ns, k0, dk, beta, nf, 10, 5, 3, seed=0, Omega=Om, ctx=ctx, points=P)
    assert len(xis) == 10 and xis[0].shape == (400,)
    it = iter(range(nf))
    xis_host, _ = gsi.getxis_iwantfields(lambda: H[:, next(it)], nf, 10, 5, 3, 0, Omega=Om, ctx=ctx)
    err = orc.xis_error_up_to_sign(np.stack(xis, axis=1), np.stack(xis_host, axis=1), 10)
    print("xis", err)
    assert err < 1e-6
    basis = gsi.getxis_fftrf(Ns, k0, dk, beta, nf, 10, 5, 3, seed=0, Omega=Om, ctx=ctx, device=True, points=P)
    assert orc.xis_error_up_to_sign(np.stack([basis[i] for i in range(10)], axis=1), np.stack(xis, axis=1), 10) < 1e-6


# ---- 6. two ranks ------------------------------------------------------------------------------------------------------
_RANKS_CHILD = r'''
import sys, threading, traceback
sys.path[:0] = [sys.argv[1], sys.argv[2]]
import numpy as np
import gsi_amd as gsi
args, seed, world, path = ((25, 25), 2.0, 3.14, -3.5, 24), int(sys.argv[3]), 2, sys.argv[4]
P = np.load(sys.argv[5])
m = P.shape[1]
ctx0 = gsi.Context(0)
uid = ctx0.unique_id()
rows, errs = [None] * world, []
def run(rank):
    try:
        ctx = ctx0 if rank == 0 else gsi.Context(0)
        ctx.comm_init(world, rank, uid)
        op = gsi.lowrank_fftrf_operator(ctx, *args, seed=seed, points=P)
        rows[rank] = (ctx.shard(m), gsi.device_samples(op, 24).copy())
        op.close()
        if rank != 0:
            ctx.close()
    except Exception:
        errs.append(traceback.format_exc())
ts = [threading.Thread(target=run, args=(r,)) for r in range(world)]
[t.start() for t in ts]
[t.join() for t in ts]
if errs:
    print(errs[0]); raise SystemExit(1)
np.savez(path, **{"r%d" % r: rows[r][1] for r in range(world)}, shards=np.array([rows[r][0] for r in range(world)]))
print("fftrf-at-ranks-ok", flush=True)
'''


def test_row_sharded_operator_at_points_holds_exactly_its_rows(gsi, ctx, tmp_path):
    """Two ranks (threads of one child process, GSI_LOCAL_COMM=1).  Both extrema of axis 0 lie in rank 1's shard and both
    extrema of axis 1 in rank 0's: a rank that took the extrema of its own rows would place every point elsewhere."""
    P = np.random.default_rng(31).random((2, 400))
    P[0, 300], P[0, 301] = -0.5, 1.5
    P[1, 10], P[1, 11] = -0.5, 1.5
    path, ppath = str(tmp_path / "rows.npz"), str(tmp_path / "points.npy")
    np.save(ppath, P)
    env = dict(os.environ, GSI_LOCAL_COMM="1")
    r = subprocess.run([sys.executable, "-c", _RANKS_CHILD, ROOT, HERE, str(OP_SEED), path, ppath], capture_output=True,
                       text=True, env=env, timeout=300)
    assert r.returncode == 0 and "fftrf-at-ranks-ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
    got = np.load(path)
    op = gsi.lowrank_fftrf_operator(ctx, *OP_ARGS, seed=OP_SEED, points=P)
    try:
        whole = gsi.device_samples(op, 24)                              # 24 x 400
    finally:
        op.close()
    assert [tuple(s) for s in got["shards"]] == [(0, 200), (200, 200)]
    for rk, (r0, nl) in enumerate(got["shards"]):
        assert got["r%d" % rk].shape == (24, nl)
        assert np.array_equal(got["r%d" % rk], whole[:, r0:r0 + nl]), rk


# ---- 7. refusals -------------------------------------------------------------------------------------------------------
def _call(gsi, ctx, which, Ns, P, box=None, rows=None, row0=0, m=None, grid_rows=None):
    """Status and message of one of the three entry points called through ctypes; a refusal must leave device_bytes() and
    *op as they were."""
    lib = ctx.lib
    P = np.asfortranarray(P, dtype=np.float64)
    m = P.shape[1] if m is None else m
    rows = max(m - row0, 1) if rows is None else rows
    arr = (C.c_int64 * len(Ns))(*Ns)
    pp = P.ctypes.data_as(gsi._lib.c_dp)
    bx = np.ascontiguousarray(box, dtype=np.float64) if box is not None else None
    bp = bx.ctypes.data_as(gsi._lib.c_dp) if bx is not None else None
    out = gsi.DeviceMatrix(ctx, rows, 2)
    grid = gsi.DeviceMatrix(ctx, grid_rows or max(int(np.prod(Ns)), 1), 2)
    h = C.c_void_p()
    try:
        before = ctx.device_bytes()
        if which == "interpolate":
            st = lib.gsi_fftrf_interpolate(ctx.h, out.h, grid.h, len(Ns), arr, pp, m, bp, row0)
        elif which == "fields_at":
            st = lib.gsi_fftrf_fields_at(ctx.h, out.h, len(Ns), arr, 0.0, 1.0, -3.5, None, 0, 0, 0, pp, m, bp, row0)
        else:
            st = lib.gsi_op_lowrank_fftrf_at(ctx.h, C.byref(h), len(Ns), arr, 0.0, 1.0, -3.5, 8, 0, pp, m, bp, 0, m)
        msg = (lib.gsi_last_error() or b"").decode()
        if st != 0:
            assert ctx.device_bytes() == before, "a refused call allocated device memory"
            assert not h.value, "a refused call left an operator"
        return st, msg
    finally:
        out.close(); grid.close()


def _refusal_cases():
    Ns = (5, 4)
    P = im.scattered_points(Ns, 50, seed=1)
    box = im.inner_box(P)

    def changed(A, at, v):
        Q = np.array(A, dtype=np.float64)
        Q[at] = v
        return Q

    same = P.copy()
    same[0, :] = 2.5
    far = P.copy()
    far[0, 0], far[0, 1] = 1.5e308, -1.5e308
    return [
        ("N<2", dict(Ns=(1, 7), P=P), "N[a] >= 2"),
        ("N<2-3d", dict(Ns=(5, 3, 1), P=im.scattered_points((5, 3, 2), 50)), "N[a] >= 2"),
        ("m<1", dict(Ns=Ns, P=P, m=0), "m >= 1"),
        ("nan-coordinate", dict(Ns=Ns, P=changed(P, (1, 17), np.nan)), "finite"),
        ("inf-coordinate", dict(Ns=Ns, P=changed(P, (0, 3), np.inf)), "finite"),
        ("nan-box", dict(Ns=Ns, P=P, box=changed(box, 3, np.nan)), "finite"),
        ("inf-box", dict(Ns=Ns, P=P, box=changed(box, 0, -np.inf)), "finite"),
        ("zero-extent", dict(Ns=Ns, P=same), "extent"),
        ("infinite-extent", dict(Ns=Ns, P=far), "extent"),
        ("zero-extent-box", dict(Ns=Ns, P=P, box=[0.0, 1.0, 0.0, 2.0]), "extent"),
        ("box-hi<lo", dict(Ns=Ns, P=P, box=[0.0, 1.0, 1.0, 0.5]), "hi >= lo"),
        ("1-D", dict(Ns=(50,), P=P[:1]), "dimension"),
        ("2731x2", dict(Ns=(2731, 2), P=P), "2730"),
    ]


@pytest.mark.parametrize("which", ["interpolate", "fields_at", "operator"])
@pytest.mark.parametrize("name,kw,word", _refusal_cases(), ids=[c[0] for c in _refusal_cases()])
def test_refusals_name_the_limit(gsi, ctx, which, name, kw, word):
    st, msg = _call(gsi, ctx, which, **kw)
    assert st == 1 and word in msg, (st, msg)


def test_refuses_an_out_with_the_wrong_row_count(gsi, ctx):
    Ns = (5, 4)
    P = im.scattered_points(Ns, 50, seed=1)
    for which in ("interpolate", "fields_at"):
        st, msg = _call(gsi, ctx, which, Ns, P, rows=51)
        assert st == 1 and "rows" in msg, (which, st, msg)
        st, msg = _call(gsi, ctx, which, Ns, P, rows=11, row0=40)
        assert st == 1 and "rows" in msg, (which, st, msg)
        st, msg = _call(gsi, ctx, which, Ns, P, rows=10, row0=40)
        assert st == 0, (which, st, msg)
    st, msg = _call(gsi, ctx, "interpolate", Ns, P, grid_rows=19)
    assert st == 1 and "prod(N)" in msg, (st, msg)
