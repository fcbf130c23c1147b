"""The device FFTRF sampler (csrc/fftrf_sample.hip, `gsi_fftrf_fields`, `gsi_op_lowrank_fftrf`) on the GPU.

1. Entry by entry against the oracle's restatement of FFTRF.jl:83-100, explicit phi, over the table of tests/fftrf_model.py
   (every kernel instantiation the launcher can produce: tests/test_fftrf_model.py asserts that on the CPU).
   Bar: max |F - F_ref| <= 1e-12 max |F_ref - k0| per field -- the bar of the line transform's own tests
   (test_fft_gridcov_gpu.py, test_fft_pass_kernels_gpu.py): Higham's log2(M) eta per transform, eta ~ 36 eps, is 2e-13 for
   two transforms of 8192 points; Bluestein runs 2 d transforms instead of 2 plus chirp products of ~eps each, 6e-13 in the
   3-D worst case; the normalisation divides signal and error by the same std.
2. Seed mode is what the header says: field f = the stream `gsi_mat_randn` writes with seed s + f, bit for bit.
3. A field's bits do not depend on the batch it rides in.
4. The LowRankCovMatrix built from such fields: samples, products, getxis, row shards.
5. Refusals: GSI_ERR_ARG naming the limit, nothing allocated.

GSI_FFTRF_RECORD=<path> writes the largest error ratio per case (device and the numpy model) and the launches per case."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import fftrf_model as fm
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
RECORD_ENV = "GSI_FFTRF_RECORD"
_record = {}


@pytest.fixture(scope="module")
def ctx(gsi):
    return gsi.default_context()


@pytest.fixture(scope="module")
def record():
    yield _record
    path = os.environ.get(RECORD_ENV)
    if path and _record:
        with open(path, "w") as f:
            json.dump({"bar": fm.BAR, "ratio": "max |F - F_oracle| / max |F_oracle - k0|, largest over the case's fields",
                       "cases": _record}, f, indent=1, sort_keys=True)
            f.write("\n")


def _device_fields(gsi, ctx, case, phi):
    F = gsi.FFTRF.powerlaw_fields(ctx, case.Ns, case.k0, case.dk, case.beta, len(phi), phi=phi)
    try:
        return F.to_host()
    finally:
        F.close()


def _worst_ratio(case, Fdev, phi):
    worst = 0.0
    for c, ph in enumerate(phi):
        ref = fm.oracle_field(case.Ns, case.k0, case.dk, case.beta, ph)
        got = Fdev[:, c].reshape(case.Ns, order="F")
        assert np.isfinite(got).all(), (case.id, c)
        worst = max(worst, fm.error_ratio(got, ref, case.k0))
    return worst


# ---- 1. entry by entry against the oracle ------------------------------------------------------------------------------
@pytest.mark.parametrize("case", fm.CASES, ids=[c.id for c in fm.CASES])
def test_fields_match_the_oracle_entry_by_entry(gsi, ctx, record, case):
    phi = case.phi()
    F = _device_fields(gsi, ctx, case, phi)
    assert F.shape == (int(np.prod(case.Ns)), case.nfields)
    worst = _worst_ratio(case, F, phi)
    print(case.id, "device", worst)
    entry = {"device": worst, "launches": fm.launches(case.Ns), "fields": case.nfields, "beta": case.beta}
    if os.environ.get(RECORD_ENV):
        entry["numpy_model"] = fm.error_ratio(fm.field(case.Ns, case.k0, case.dk, case.beta, phi[0]),
                                              fm.oracle_field(case.Ns, case.k0, case.dk, case.beta, phi[0]), case.k0)
    record[case.id] = entry
    assert worst <= fm.BAR


def test_ragged_batches_match_the_oracle(gsi, ctx, record, monkeypatch):
    """131 fields of a 5 x 3 grid at the default batch and in batches of 7 (ragged last batch)."""
    case = fm.BATCH_CASE
    phi = case.phi()
    monkeypatch.delenv("GSI_FFTRF_BATCH", raising=False)
    F0 = _device_fields(gsi, ctx, case, phi)
    monkeypatch.setenv("GSI_FFTRF_BATCH", "7")
    F7 = _device_fields(gsi, ctx, case, phi)
    monkeypatch.delenv("GSI_FFTRF_BATCH")
    w0, w7 = _worst_ratio(case, F0, phi), _worst_ratio(case, F7, phi)
    print(case.id, "default batch", w0, "batches of 7", w7)
    record[case.id + " x131"] = {"device": max(w0, w7), "launches": fm.launches(case.Ns), "fields": case.nfields,
                                 "beta": case.beta}
    assert w0 <= fm.BAR and w7 <= fm.BAR
    assert np.array_equal(F0, F7)


# ---- 2. seed mode ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Ns", [(25, 25), (6, 4, 5)], ids=["25x25", "6x4x5"])
def test_seed_mode_is_the_randn_stream_of_the_header(gsi, ctx, Ns):
    s, nf, k0, dk, beta = 20170301, 5, 2.0, 3.14, -3.5
    shp = gsi.FFTRF.phi_shape(Ns)
    mtot = int(np.prod(shp))
    phi = []
    for f in range(nf):
        M = gsi.DeviceMatrix(ctx, mtot, 1).randn(s + f)
        phi.append(M.to_host()[:, 0].reshape(shp, order="F"))
        M.close()
    Fs = gsi.FFTRF.powerlaw_fields(ctx, Ns, k0, dk, beta, nf, seed=s)
    Fp = gsi.FFTRF.powerlaw_fields(ctx, Ns, k0, dk, beta, nf, phi=phi)
    Hs, Hp = Fs.to_host(), Fp.to_host()
    Fs.close(); Fp.close()
    for f in range(nf):
        ref = fm.oracle_field(Ns, k0, dk, beta, phi[f])
        r = fm.error_ratio(Hs[:, f].reshape(Ns, order="F"), ref, k0)
        print(Ns, f, r)
        assert r <= fm.BAR
    assert np.array_equal(Hs, Hp)


# ---- 3. independence of batching ---------------------------------------------------------------------------------------
def test_a_field_does_not_depend_on_its_batch(gsi, ctx, monkeypatch):
    Ns, s, args = (25, 25), 77, (2.0, 3.14, -3.5)

    def fields(nf, field0=0):
        F = gsi.FFTRF.powerlaw_fields(ctx, Ns, *args, nf, seed=s, field0=field0)
        try:
            return F.to_host()
        finally:
            F.close()

    monkeypatch.delenv("GSI_FFTRF_BATCH", raising=False)
    whole = fields(5)
    assert np.array_equal(fields(5), whole)                 # a second identical call
    singles = np.concatenate([fields(1, field0=f) for f in range(5)], axis=1)
    assert np.array_equal(singles, whole)
    for b in ("1", "2"):
        monkeypatch.setenv("GSI_FFTRF_BATCH", b)
        assert np.array_equal(fields(5), whole), b
    monkeypatch.delenv("GSI_FFTRF_BATCH")
    assert not np.array_equal(whole[:, 0], whole[:, 1])


def test_powerlaw_structuredgrid_mirrors_the_reference(gsi, ctx):
    Ns = (7, 11)
    phi = np.random.default_rng(5).standard_normal(gsi.FFTRF.phi_shape(Ns))
    f = gsi.FFTRF.powerlaw_structuredgrid(Ns, 1.5, 0.5, -3.0, phi=phi, ctx=ctx)
    assert f.shape == Ns
    assert fm.error_ratio(f, fm.oracle_field(Ns, 1.5, 0.5, -3.0, phi), 1.5) <= fm.BAR
    gsi.RandMatFact.seed(9)
    a = gsi.FFTRF.powerlaw_structuredgrid(Ns, 1.5, 0.5, -3.0, ctx=ctx)
    gsi.RandMatFact.seed(9)
    b = gsi.FFTRF.powerlaw_structuredgrid(Ns, 1.5, 0.5, -3.0, ctx=ctx)
    assert np.array_equal(a, b) and abs(a.mean() - 1.5) < 1e-12 and abs(a.std(ddof=1) - 0.5) < 1e-12


# ---- 4. the operator ---------------------------------------------------------------------------------------------------
OP_ARGS = ((25, 25), 2.0, 3.14, -3.5, 24)
OP_SEED = 4242


@pytest.fixture(scope="module")
def op_fields(gsi, ctx):
    F = gsi.FFTRF.powerlaw_fields(ctx, *OP_ARGS, seed=OP_SEED)
    H = F.to_host()
    F.close()
    return H                                                    # 625 x 24


def test_operator_samples_are_the_centred_fields(gsi, ctx, op_fields):
    op = gsi.lowrank_fftrf_operator(ctx, *OP_ARGS, seed=OP_SEED)
    lr = gsi.LowRankCovMatrix(op_fields.T, ctx=ctx)
    try:
        assert op.shape == (625, 625)
        assert np.array_equal(gsi.device_samples(op, 24), lr.samples)
    finally:
        op.close(); lr.close()


def test_operator_product_matches_the_oracle(gsi, ctx, op_fields):
    op = gsi.lowrank_fftrf_operator(ctx, *OP_ARGS, seed=OP_SEED)
    try:
        X = np.random.default_rng(3).standard_normal((625, 7))
        ref = orc.LowRankCovMatrix(op_fields.T)
        full = ref.samples.T @ ref.samples / (24 - 1)
        Y = op.matmul(X)
        err = np.abs(Y - full @ X).max() / np.abs(full @ X).max()
        print("product", err)
        assert err < 1e-10
    finally:
        op.close()


def test_getxis_fftrf_matches_getxis_on_the_same_fields(gsi, ctx):
    Ns, k0, dk, beta, nf = OP_ARGS
    F = gsi.FFTRF.powerlaw_fields(ctx, Ns, k0, dk, beta, nf, seed=0)
    H = F.to_host()
    F.close()
    Om = np.random.default_rng(0).standard_normal((625, 15))
    xis = gsi.getxis_fftrf(Ns, k0, dk, beta, nf, 10, 5, 3, seed=0, Omega=Om, ctx=ctx)
    it = iter(range(nf))
    xis_host, _ = gsi.getxis_iwantfields(lambda: H[:, next(it)], nf, 10, 5, 3, 0, Omega=Om, ctx=ctx)
    err = orc.xis_error_up_to_sign(np.stack(xis, axis=1), np.stack(xis_host, axis=1), 10)
    print("xis", err)
    assert err < 1e-6
    basis = gsi.getxis_fftrf(Ns, k0, dk, beta, nf, 10, 5, 3, seed=0, Omega=Om, ctx=ctx, device=True)
    assert orc.xis_error_up_to_sign(np.stack([basis[i] for i in range(10)], axis=1), np.stack(xis, axis=1), 10) < 1e-6


_RANKS_CHILD = r'''
import sys, threading, traceback
sys.path[:0] = [sys.argv[1], sys.argv[2]]
import numpy as np
import gsi_amd as gsi
args, seed, world, path = ((25, 25), 2.0, 3.14, -3.5, 24), int(sys.argv[3]), 2, sys.argv[4]
ctx0 = gsi.Context(0)
uid = ctx0.unique_id()
rows, errs = [None] * world, []
def run(rank):
    try:
        ctx = ctx0 if rank == 0 else gsi.Context(0)
        ctx.comm_init(world, rank, uid)
        op = gsi.lowrank_fftrf_operator(ctx, *args, seed=seed)
        rows[rank] = (ctx.shard(625), gsi.device_samples(op, 24).copy())
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
print("fftrf-ranks-ok", flush=True)
'''


def test_row_sharded_operator_holds_exactly_its_rows(gsi, ctx, op_fields, tmp_path):
    """Two ranks (threads of one child process, GSI_LOCAL_COMM=1): each generates every field and keeps its own rows."""
    path = str(tmp_path / "rows.npz")
    env = dict(os.environ, GSI_LOCAL_COMM="1")
    r = subprocess.run([sys.executable, "-c", _RANKS_CHILD, ROOT, HERE, str(OP_SEED), path], capture_output=True, text=True,
                       env=env, timeout=300)
    assert r.returncode == 0 and "fftrf-ranks-ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
    got = np.load(path)
    op = gsi.lowrank_fftrf_operator(ctx, *OP_ARGS, seed=OP_SEED)
    try:
        whole = gsi.device_samples(op, 24)                              # 24 x 625
    finally:
        op.close()
    assert [tuple(s) for s in got["shards"]] == [(0, 313), (313, 312)]
    for rk, (r0, nl) in enumerate(got["shards"]):
        assert got["r%d" % rk].shape == (24, nl)
        assert np.array_equal(got["r%d" % rk], whole[:, r0:r0 + nl]), rk


# ---- 5. refusals -------------------------------------------------------------------------------------------------------
def _refused(gsi, ctx, rows, Ns, k0=0.0, dk=1.0, beta=-3.5, phi=None, ldphi=0):
    lib = ctx.lib
    F = gsi.DeviceMatrix(ctx, rows, 1)
    try:
        before = ctx.device_bytes()
        arr = (C.c_int64 * len(Ns))(*Ns)
        st = lib.gsi_fftrf_fields(ctx.h, F.h, len(Ns), arr, k0, dk, beta,
                                  phi.ctypes.data_as(gsi._lib.c_dp) if phi is not None else None, ldphi, 0, 0)
        msg = (lib.gsi_last_error() or b"").decode()
        assert ctx.device_bytes() == before, "a refused call allocated device memory"
        return st, msg
    finally:
        F.close()


@pytest.mark.parametrize("Ns,rows,word", [
    ((50,), 50, "dimension"), ((3, 3, 3, 3), 81, "dimension"), ((2731, 2), 5462, "2730"), ((4097, 1), 4097, "2730"),
    ((1, 1), 1, "n >= 2"), ((25, 25), 624, "rows")], ids=["1-D", "4-D", "2731x2", "4097x1", "1x1", "wrong-rows"])
def test_refusals_name_the_limit(gsi, ctx, Ns, rows, word):
    st, msg = _refused(gsi, ctx, rows, Ns)
    assert st == 1 and word in msg, (st, msg)


def test_refuses_non_finite_dk_and_short_ldphi(gsi, ctx):
    st, msg = _refused(gsi, ctx, 625, (25, 25), dk=float("inf"))
    assert st == 1 and "finite" in msg, (st, msg)
    st, msg = _refused(gsi, ctx, 625, (25, 25), dk=float("nan"))
    assert st == 1 and "finite" in msg, (st, msg)
    phi = np.zeros(2500)
    st, msg = _refused(gsi, ctx, 625, (25, 25), phi=phi, ldphi=2499)
    assert st == 1 and "ldphi" in msg, (st, msg)
    h = C.c_void_p()
    before = ctx.device_bytes()
    arr = (C.c_int64 * 2)(2731, 2)
    st = ctx.lib.gsi_op_lowrank_fftrf(ctx.h, C.byref(h), 2, arr, 0.0, 1.0, -3.5, 8, 0, 0, 5462)
    assert st == 1 and not h.value and ctx.device_bytes() == before
