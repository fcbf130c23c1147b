"""The circulant-embedding sampler for grid covariance functions (csrc/gridcov_sample.hip, `gsi_gridcov_sampler_*`,
`gsi_gridcov_fields`, `gsi_op_lowrank_gridcov`) on the GPU, against the numpy model of tests/gridcov_sample_model.py.

1. The plan's spectrum, neg_mass, lambda_min and lambda_max against the model: max |dlambda| <= 1e-12 lambda_0, with
   lambda_0 = sum of the torus table (+ nugget) = lambda_max, since the four kernels are non-negative.  The statistics follow
   from that bound: |d lambda_min|, |d lambda_max| <= 1e-12 lambda_0, and |d neg_mass| <= 1e-12 lambda_0 / (sigma2 + nugget)
   (every |lambda_k| that enters or leaves the sum, or changes within it, moves by at most the bound; the sum is divided by
   Mtot (sigma2 + nugget)).
2. The passes, every instantiation of the line kernel (tests/test_gridcov_sample_model.py asserts that on the CPU): explicit
   noise, odd and even field counts, expected fields = the model's from the DEVICE's own spectrum (the square root of a
   lambda near zero is ill-conditioned and not what this checks).  Bar 1e-12 max |F|, the FFTRF sampler's.
3. The covariance of the device's fields by impulses: F F' against the dense matrix at 1e-12 (sigma2 + nugget) (the error is
   linear in dlambda, Mtot <= 1024), and the clamp's bound attained on the diagonal.
4. Refusal (GSI_ERR_NOT_POSDEF, nothing left allocated) and embed="auto".
5. Determinism: seed mode = the randn streams of the header; batches, field counts, field0 and row ranges change no bit.
6. The LowRankCovMatrix over such fields.  7. Composition with FFTRF.interpolate.

GSI_GRIDCOV_RECORD=<path> writes the largest ratio to its bar per case (profiles/gridcov_sample_errors.json)."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import gridcov_sample_model as gm

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
RECORD_ENV = "GSI_GRIDCOV_RECORD"
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
            json.dump({"bars": {"spectrum": "max |lambda - lambda_model| / lambda_0 <= 1e-12",
                                "fields": "max |F - F_model(device spectrum)| / max |F_model| <= 1e-12",
                                "covariance": "max |F F' - C| / (sigma2 + nugget) <= 1e-12"},
                       "ratio": "measured / bar, largest over the case", "cases": _record}, f, indent=1, sort_keys=True)
            f.write("\n")


def _sampler(gsi, ctx, c, **kw):
    return gsi.gridcov_sampler(ctx, c.N, c.kind, c.ell, c.theta, c.sigma2, c.nugget, embed=c.M, **kw)


def _host(F):
    try:
        return F.to_host()
    finally:
        F.close()


def _note(record, c, key, ratio):
    record.setdefault(gm.case_id(c), {})[key] = ratio


# ---- 1. the spectrum -----------------------------------------------------------------------------------------------------
_STRICT = set(gm.EXACT_CASES + gm.DEFAULT_CASES)


@pytest.mark.parametrize("c", gm.GPU_CASES, ids=[gm.case_id(c) for c in gm.GPU_CASES])
def test_spectrum_matches_the_model(gsi, ctx, record, c):
    lam = gm.spectrum(c)
    lam0 = gm.torus_table(c).sum() + c.nugget
    assert abs(lam.max() - lam0) <= 1e-12 * lam0
    s = _sampler(gsi, ctx, c, neg_tol=1e-12 if c in _STRICT else 1.0)     # the default bar carries what numpy says it carries
    try:
        assert s.M == c.M
        dev = s.spectrum()
        assert dev.shape == c.M
        err = np.abs(dev - lam).max() / lam0
        stats = max(abs(s.lam_min - lam.min()) / lam0, abs(s.lam_max - lam.max()) / lam0,
                    abs(s.neg_mass - gm.neg_mass(c, lam)) * (c.sigma2 + c.nugget) / lam0)
        print(gm.case_id(c), "spectrum", err, "statistics", stats, "neg_mass", s.neg_mass, "clamped", s.clamped)
        _note(record, c, "spectrum", max(err, stats) / gm.COV_BAR)
        assert err <= gm.COV_BAR and stats <= gm.COV_BAR
        assert s.lam_min == dev.min() and s.lam_max == dev.max() and s.clamped == int((dev < 0).sum())
    finally:
        s.close()


# ---- 2. the passes -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", gm.TRANSFORM_CASES, ids=[gm.case_id(c) for c in gm.TRANSFORM_CASES])
def test_fields_match_the_model_in_every_instantiation(gsi, ctx, record, c):
    mtot = int(np.prod(c.M))
    eps = np.asfortranarray(np.random.default_rng(mtot).standard_normal((mtot, 4)))
    s = _sampler(gsi, ctx, c, neg_tol=1.0)
    try:
        ref = gm.fields_from_eps(s.spectrum(), c.N, eps)
        F4 = _host(s.fields(4, eps=eps))
        F3 = _host(s.fields(3, eps=eps))
    finally:
        s.close()
    assert F4.shape == (int(np.prod(c.N)), 4) and np.isfinite(F4).all()
    err = np.abs(F4 - ref).max() / np.abs(ref).max()
    print(gm.case_id(c), gm.pass_instantiations(c), "fields", err)
    _note(record, c, "fields", err / gm.FIELD_BAR)
    assert err <= gm.FIELD_BAR
    assert np.array_equal(F3, F4[:, :3])


# ---- 3. the covariance ---------------------------------------------------------------------------------------------------
def _impulse_cov(gsi, ctx, c, neg_tol):
    mtot = int(np.prod(c.M))
    s = _sampler(gsi, ctx, c, neg_tol=neg_tol)
    try:
        F = _host(s.fields(2 * mtot, eps=gm.impulse_eps(mtot)))
    finally:
        s.close()
    return F @ F.T


@pytest.mark.parametrize("c", gm.EXACT_CASES, ids=[gm.case_id(c) for c in gm.EXACT_CASES])
def test_device_fields_have_the_dense_covariance(gsi, ctx, record, c):
    err = np.abs(_impulse_cov(gsi, ctx, c, 1e-12) - gm.dense_cov(c)).max() / (c.sigma2 + c.nugget)
    print(gm.case_id(c), "covariance", err)
    _note(record, c, "covariance", err / gm.COV_BAR)
    assert err <= gm.COV_BAR


def test_the_clamp_bound_is_attained_on_the_device(gsi, ctx, record):
    c = gm.BOUND_CASE
    nm = gm.neg_mass(c, gm.spectrum(c))
    E = _impulse_cov(gsi, ctx, c, 0.05) - gm.dense_cov(c)
    gap = abs(np.abs(np.diag(E)).max() - nm * c.sigma2)
    print(gm.case_id(c), "diag error", np.abs(np.diag(E)).max(), "neg_mass sigma2", nm * c.sigma2, "gap", gap)
    _note(record, c, "covariance", gap / gm.COV_BAR)
    assert gap <= 1e-12
    assert np.abs(E).max() <= nm * c.sigma2 + 1e-12


# ---- 4. refusal and auto -------------------------------------------------------------------------------------------------
def test_refusal_names_neg_mass_and_auto_finds_the_torus(gsi, ctx):
    c = gm.NOT_CARRIED
    args = (c.N, c.kind, c.ell)
    before = ctx.device_bytes()
    with pytest.raises(gsi.GsiError) as ei:
        gsi.gridcov_sampler(ctx, *args)
    assert ei.value.code == 7 and "neg_mass" in str(ei.value) and "larger embedding" in str(ei.value), ei.value
    assert ctx.device_bytes() == before
    # info is filled in both outcomes
    h, info = C.c_void_p(), (C.c_double * 4)()
    N, ell = (C.c_int64 * 2)(*c.N), (C.c_double * 2)(*c.ell)
    assert ctx.lib.gsi_gridcov_sampler_create(ctx.h, C.byref(h), 2, N, None, 1, ell, 0.0, 1.0, 0.0, 1e-12, info) == 7
    assert not h.value and abs(info[0] - gm.NOT_CARRIED_NEG_MASS[64]) <= 0.005 * info[0] and info[1] < 0 < info[2] and info[3] > 0
    assert ctx.device_bytes() == before
    s = gsi.gridcov_sampler(ctx, *args, embed="auto")
    try:
        assert s.M == (512, 512) and s.neg_mass <= 1e-12
    finally:
        s.close()
    s = gsi.gridcov_sampler(ctx, *args, embed=(512, 512))
    s.close()
    s = gsi.gridcov_sampler(ctx, *args, neg_tol=0.05)               # accepted as an approximation, and says by how much
    try:
        assert s.M == (64, 64) and abs(s.neg_mass - info[0]) == 0.0 and s.clamped == int(info[3])
    finally:
        s.close()


def test_fields_refuse_bad_arguments_by_name(gsi, ctx):
    c = gm.EXACT_CASES[0]
    s = _sampler(gsi, ctx, c)
    F = gsi.DeviceMatrix(ctx, 32, 2)
    G = gsi.DeviceMatrix(ctx, 31, 2)
    eps = np.zeros((128, 2), order="F")
    try:
        before = ctx.device_bytes()
        for args, word in (((s.h, G.h, None, 0, 0, 0), "rows"), ((s.h, F.h, None, 0, 0, 1), "field0"),
                           ((s.h, F.h, None, 0, 0, -2), "field0"), ((s.h, F.h, gsi._lib.dptr(eps), 127, 0, 0), "ldeps")):
            assert ctx.lib.gsi_gridcov_fields(ctx.h, *args) == 1
            assert word in ctx.lib.gsi_last_error().decode(), (word, ctx.lib.gsi_last_error())
        h = C.c_void_p()
        assert ctx.lib.gsi_op_lowrank_gridcov(ctx.h, C.byref(h), s.h, 1, 0, 0, 32) == 1 and not h.value
        assert ctx.lib.gsi_op_lowrank_gridcov(ctx.h, C.byref(h), s.h, 8, 0, 0, 31) == 1 and not h.value
        assert ctx.device_bytes() == before
        with pytest.raises(ValueError):
            s.fields(3, eps=eps)
    finally:
        F.close(); G.close(); s.close()


# ---- 5. determinism ------------------------------------------------------------------------------------------------------
DET_CASES = [gm.DEFAULT_CASES[1], gm.DEFAULT_CASES[4]]                  # 37 x 29 rotated on 128 x 64; 8 x 6 x 5 on 16 x 16 x 16


@pytest.mark.parametrize("c", DET_CASES, ids=[gm.case_id(c) for c in DET_CASES])
def test_seed_mode_is_the_randn_stream_of_the_header(gsi, ctx, c):
    seed, nf = 20170301, 5
    mtot = int(np.prod(c.M))
    eps = np.empty((mtot, 6), order="F")
    for f in range(6):
        R = gsi.DeviceMatrix(ctx, mtot, 1).randn(seed + f)
        eps[:, f] = R.to_host()[:, 0]
        R.close()
    s = _sampler(gsi, ctx, c)
    try:
        Fs, Fe = _host(s.fields(nf, seed=seed)), _host(s.fields(nf, eps=eps))
        ref = gm.fields_from_eps(s.spectrum(), c.N, eps)[:, :nf]
    finally:
        s.close()
    assert np.array_equal(Fs, Fe)
    assert np.abs(Fs - ref).max() <= gm.FIELD_BAR * np.abs(ref).max()
    assert 0.2 < Fs.std() / np.sqrt(c.sigma2 + c.nugget) < 2.0           # fields of that variance, not noise or zeros


def test_a_field_does_not_depend_on_batch_count_or_field0(gsi, ctx, monkeypatch):
    c, seed = DET_CASES[0], 77
    s = _sampler(gsi, ctx, c)
    try:
        monkeypatch.delenv("GSI_GRIDCOV_BATCH", raising=False)
        whole = _host(s.fields(8, seed=seed))
        assert np.array_equal(_host(s.fields(8, seed=seed)), whole)           # a second identical call
        assert np.array_equal(_host(s.fields(5, seed=seed)), whole[:, :5])
        assert np.array_equal(_host(s.fields(6, seed=seed, field0=2)), whole[:, 2:])
        assert np.array_equal(_host(s.fields(1, seed=seed, field0=6)), whole[:, 6:7])
        for b in ("1", "3"):
            monkeypatch.setenv("GSI_GRIDCOV_BATCH", b)
            assert np.array_equal(_host(s.fields(8, seed=seed)), whole), b
            assert np.array_equal(_host(s.fields(5, seed=seed)), whole[:, :5]), b
        monkeypatch.delenv("GSI_GRIDCOV_BATCH")
        assert not np.array_equal(whole[:, 0], whole[:, 1]) and not np.array_equal(whole[:, 0], whole[:, 2])
    finally:
        s.close()


# ---- 6. the operator -----------------------------------------------------------------------------------------------------
OP_CASE, OP_NF, OP_SEED = gm.DEFAULT_CASES[0], 24, 4242               # 24 x 20: n = 480


@pytest.fixture(scope="module")
def op_fields(gsi, ctx):
    s = _sampler(gsi, ctx, OP_CASE)
    try:
        return _host(s.fields(OP_NF, seed=OP_SEED))                     # 480 x 24
    finally:
        s.close()


def test_operator_samples_and_products(gsi, ctx, op_fields):
    s = _sampler(gsi, ctx, OP_CASE)
    op = gsi.lowrank_gridcov_operator(ctx, s, OP_NF, seed=OP_SEED)
    lr = gsi.LowRankCovMatrix(op_fields.T, ctx=ctx)
    try:
        n = int(np.prod(OP_CASE.N))
        assert op.shape == (n, n)
        assert np.array_equal(gsi.device_samples(op, OP_NF), lr.samples)
        X = np.random.default_rng(3).standard_normal((n, 16))
        S = op_fields - op_fields.mean(axis=1, keepdims=True)
        full = S @ S.T / (OP_NF - 1)
        err = np.abs(op.matmul(X) - full @ X).max() / np.abs(full @ X).max()
        print("product", err)
        assert err < 1e-10
    finally:
        op.close(); lr.close(); s.close()


_RANKS_CHILD = r'''
import sys, threading, traceback
sys.path[:0] = [sys.argv[1], sys.argv[2]]
import numpy as np
import gsi_amd as gsi
import gridcov_sample_model as gm
c, nf, seed, world, path = gm.DEFAULT_CASES[0], 24, int(sys.argv[3]), 2, sys.argv[4]
n = int(np.prod(c.N))
ctx0 = gsi.Context(0)
uid = ctx0.unique_id()
rows, errs = [None] * world, []
def run(rank):
    try:
        ctx = ctx0 if rank == 0 else gsi.Context(0)
        ctx.comm_init(world, rank, uid)
        s = gsi.gridcov_sampler(ctx, c.N, c.kind, c.ell, c.theta, c.sigma2, c.nugget)
        op = gsi.lowrank_gridcov_operator(ctx, s, nf, seed=seed)
        rows[rank] = (ctx.shard(n), gsi.device_samples(op, nf).copy())
        op.close(); s.close()
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
print("gridcov-ranks-ok", flush=True)
'''


def test_a_row_range_holds_exactly_its_rows(gsi, ctx, op_fields, tmp_path):
    """Two ranks (threads of one child process, GSI_LOCAL_COMM=1): each generates every field and keeps rows
    [row0, row0 + n_local) of it, the same bits as those rows of the full call."""
    path = str(tmp_path / "rows.npz")
    env = dict(os.environ, GSI_LOCAL_COMM="1")
    r = subprocess.run([sys.executable, "-c", _RANKS_CHILD, ROOT, HERE, str(OP_SEED), path], capture_output=True, text=True,
                       env=env, timeout=300)
    assert r.returncode == 0 and "gridcov-ranks-ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
    got = np.load(path)
    lr = gsi.LowRankCovMatrix(op_fields.T, ctx=ctx)                      # the full call's fields, centred as the operator's
    try:
        centred = lr.samples                                             # 24 x 480
    finally:
        lr.close()
    assert [tuple(s) for s in got["shards"]] == [(0, 240), (240, 240)]
    for rk, (r0, nl) in enumerate(got["shards"]):
        assert got["r%d" % rk].shape == (OP_NF, nl)
        assert np.array_equal(got["r%d" % rk], centred[:, r0:r0 + nl]), rk


# ---- 7. composition ------------------------------------------------------------------------------------------------------
def test_fields_at_mesh_points_through_fftrf_interpolate(gsi, ctx):
    c = gm.DEFAULT_CASES[3]                                              # 16 x 12
    pts = np.asfortranarray(np.random.default_rng(11).uniform(0.0, 1.0, (2, 200)))
    s = _sampler(gsi, ctx, c)
    F = s.fields(3, seed=5)
    try:
        H = F.to_host()
        dev = _host(gsi.FFTRF.interpolate(ctx, pts, F, c.N))
        host = _host(gsi.FFTRF.interpolate(ctx, pts, H.reshape(c.N + (3,), order="F"), c.N))
        assert dev.shape == (200, 3) and np.array_equal(dev, host)
        assert H.min() - 1e-12 <= dev.min() and dev.max() <= H.max() + 1e-12
    finally:
        F.close(); s.close()


def test_gridcov_structuredgrid_returns_one_field(gsi, ctx):
    c = gm.DEFAULT_CASES[3]
    a = gsi.gridcov_structuredgrid(c.N, c.kind, c.ell, seed=9, ctx=ctx)
    s = _sampler(gsi, ctx, c)
    try:
        assert a.shape == c.N and np.array_equal(a.reshape(-1, order="F"), _host(s.fields(1, seed=9))[:, 0])
    finally:
        s.close()
    gsi.RandMatFact.seed(9)
    b1 = gsi.gridcov_structuredgrid(c.N, c.kind, c.ell, ctx=ctx)
    gsi.RandMatFact.seed(9)
    b2 = gsi.gridcov_structuredgrid(c.N, c.kind, c.ell, ctx=ctx)
    assert np.array_equal(b1, b2) and not np.array_equal(a, b1)
