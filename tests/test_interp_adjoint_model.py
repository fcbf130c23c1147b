"""The adjoint of FFTRF.interpolate without a GPU:

1. The numpy restatement (tests/interp_adjoint_model.py): its dense W against `fftrf_interp_model.interp`, its rows summing to
   one, and its spread against W' X.
2. The host planner of the inverted index (csrc/interp_adjoint_plan.hpp) built stand-alone under the address and
   undefined-behaviour sanitizers (tests/interp_adjoint_check.cpp) and compared with the model entry for entry.
3. The new names are exported, and `diagonal()`'s lag bookkeeping on a host stand-in for the grid operator.
4. The seed of the GPU test that compares the operator with the sampler's empirical covariance: the model's fields for
   that seed stay inside the Monte-Carlo bound."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import fftrf_interp_model as im
import gridcov_sample_model as gm
import interp_adjoint_model as am

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -53


# ---- 1. the model ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 63, 1000])
@pytest.mark.parametrize("Ns", im.GRIDS, ids=im.gid)
def test_dense_W_equals_the_interpolation_model(Ns, m):
    P = im.scattered_points(Ns, m, seed=2)
    V = im.random_fields(Ns, 3, seed=4)
    for box in (None, im.inner_box(P))[m == 1:]:          # (a single point has no extent of its own)
        base, frac = im.plan(P, Ns, box)
        W = am.weights_matrix(Ns, base, frac)
        # 1 - f, a corner weight of up to three rounded factors, one product with V, a 2^d-term sum -- against nested two-term sums
        assert np.abs(W @ V - im.interp(V, Ns, base, frac)).max() <= 4 * EPS * np.abs(V).max()
        assert np.abs(W.sum(axis=1) - 1.0).max() <= (1 << len(Ns)) * EPS
        assert (W >= 0.0).all() and ((W != 0).sum(axis=1) <= (1 << len(Ns))).all()


@pytest.mark.parametrize("Ns", [(3, 5), (6, 4, 5), (33, 2, 17)], ids=im.gid)
def test_model_spread_is_the_transpose(Ns):
    P = im.scattered_points(Ns, 257, seed=6)
    base, frac = im.plan(P, Ns, im.inner_box(P))
    X = np.random.default_rng(1).standard_normal((257, 3))
    G = am.spread(X, Ns, base, frac)
    ref = am.weights_matrix(Ns, base, frac).T.astype(np.longdouble) @ X.astype(np.longdouble)
    scale = am.spread(X, Ns, base, frac, absolute=True)
    assert (np.abs(G - ref) <= 8 * EPS * scale + 1e-300).all()
    k = am.node_counts(base, Ns)
    assert k.sum() == 257 * (1 << len(Ns)) and (G[k == 0] == 0.0).all()


# ---- 2. the planner under sanitizers -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build the planner check"
    exe = str(tmp_path_factory.mktemp("interp_adjoint") / "interp_adjoint_check")
    src = os.path.join(ROOT, "tests", "interp_adjoint_check.cpp")
    inc = os.path.join(ROOT, "geostatinversion.jl_amd", "csrc")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", inc, src, "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def chunk_limit(planner):
    r = subprocess.run([planner, "--chunk"], capture_output=True, text=True, check=True)
    return int(r.stdout)


def _run(exe, tmp_path, Ns, P, box=None, chunk=None):
    d, m = P.shape
    N3 = list(Ns) + [1] * (3 - len(Ns))
    case, out = str(tmp_path / "case.bin"), str(tmp_path / "index.bin")
    with open(case, "wb") as f:
        np.array([d] + N3[:3] + [m, int(box is not None), 0, m], dtype=np.int64).tofile(f)
        np.asfortranarray(P, dtype=np.float64).reshape(-1, order="F").tofile(f)
        if box is not None:
            np.asarray(box, dtype=np.float64).tofile(f)
    r = subprocess.run([exe, case, out] + ([str(chunk)] if chunk else []), capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("indexed"), r.stdout + r.stderr     # its own checks: once each, in order
    raw = open(out, "rb").read()
    head = np.frombuffer(raw[:56], dtype=np.int64)
    n, m_, total, nlong, nchunk, maxlen, ch = (int(v) for v in head)
    got, o = {"n": n, "m": m_, "chunk": ch, "maxlen": maxlen}, 56
    for name, dt, cnt in (("nodeptr", np.int64, n + 1), ("point", np.int32, total), ("corner", np.uint8, total),
                          ("long_node", np.int32, nlong), ("long_chunk0", np.int64, nlong + 1), ("chunk_off", np.int64, nchunk),
                          ("chunk_len", np.int32, nchunk)):
        nb = cnt * np.dtype(dt).itemsize
        got[name] = np.frombuffer(raw[o:o + nb], dtype=dt)
        o += nb
    assert o == len(raw)
    return got


def _same(got, ref):
    assert set(got) == set(ref)
    for k in ref:
        assert np.array_equal(got[k], ref[k]), k


def _compare(exe, tmp_path, Ns, P, box, chunk):
    got = _run(exe, tmp_path, Ns, P, box, chunk)
    base, _ = im.plan(P, Ns, box)
    _same(got, am.index(base, Ns, got["chunk"]))
    # every (point, corner) pair exactly once, every list in ascending point order
    pairs = got["point"].astype(np.int64) * (1 << len(Ns)) + got["corner"]
    assert np.array_equal(np.sort(pairs), np.arange(P.shape[1] << len(Ns)))
    node_of = np.repeat(np.arange(got["n"]), np.diff(got["nodeptr"]))
    inside = node_of[1:] == node_of[:-1]
    assert (np.diff(got["point"].astype(np.int64))[inside] > 0).all()
    return got


@pytest.mark.parametrize("m", [1, 63, 1000])
@pytest.mark.parametrize("Ns", im.MODEL_GRIDS, ids=im.gid)
def test_planner_equals_the_model_index(planner, chunk_limit, tmp_path, Ns, m):
    P = im.scattered_points(Ns, m, seed=5)
    for box, chunk in ((None, None), (im.inner_box(P), None), (im.inner_box(P), 3))[m == 1:]:   # (one point: no extent of its own)
        got = _compare(planner, tmp_path, Ns, P, box, chunk)
        assert got["chunk"] == (chunk or chunk_limit)


def test_all_points_identical_and_all_outside(planner, chunk_limit, tmp_path):
    Ns = (6, 4, 5)
    m = 3 * chunk_limit + 5                    # at least 3 chunks and a remainder at every node of the cell
    P = np.tile(np.array([[0.3], [0.4], [0.6]]), (1, m))
    got = _compare(planner, tmp_path, Ns, P, np.array([0.0, 0.0, 0.0, 1.0, 1.0, 1.0]), None)
    assert len(got["long_node"]) == 8 and got["maxlen"] == m
    assert np.array_equal(np.diff(got["long_chunk0"]), np.full(8, 4))
    assert np.array_equal(got["chunk_len"].reshape(8, 4), np.tile([chunk_limit] * 3 + [5], (8, 1)))
    # every point outside an inner box: all of them clamped onto the boundary nodes
    Ns = (25, 37)
    Q = im.scattered_points(Ns, 1000, seed=9) * 100.0
    box = np.array([-0.5, -0.5, 0.5, 0.5])
    keep = ((np.abs(Q) > 0.5).any(axis=0))
    got = _compare(planner, tmp_path, Ns, Q[:, keep], box, None)
    idx = np.stack(np.unravel_index(np.nonzero(np.diff(got["nodeptr"]))[0], Ns, order="F"))
    top = np.array(Ns)[:, None] - 1
    assert ((idx <= 1) | (idx >= top - 1)).any(axis=0).all()      # only nodes of the boundary cells are reached


def test_a_long_list_is_cut_into_chunks_and_a_remainder(planner, chunk_limit, tmp_path):
    Ns = (3, 5)
    m = 3 * chunk_limit + 7
    rng = np.random.default_rng(3)
    P = np.vstack([0.5 + 0.4 * rng.random(m), 1.5 + 0.4 * rng.random(m)])      # one cell
    got = _compare(planner, tmp_path, Ns, P, np.array([0.0, 0.0, 2.0, 4.0]), None)
    assert len(got["long_node"]) == 4 and (np.diff(got["long_chunk0"]) == 4).all()
    assert (got["chunk_len"].reshape(4, 4) == np.array([chunk_limit] * 3 + [7])).all()
    assert np.array_equal(got["chunk_off"].reshape(4, 4)[:, 0], got["nodeptr"][got["long_node"]])
    # exactly at the limit: one list, no chunk
    got = _compare(planner, tmp_path, Ns, P[:, :chunk_limit], np.array([0.0, 0.0, 2.0, 4.0]), None)
    assert len(got["long_node"]) == 0 and got["maxlen"] == chunk_limit


# ---- 3. exports, and diagonal() on the host ----------------------------------------------------------------------------
def test_new_names_are_exported(gsi):
    for name in ("fft_operator_at", "FFTOperatorAt"):
        assert name in gsi.__all__ and callable(getattr(gsi, name)), name
    assert callable(gsi.FFTRF.spread)
    for sym in ("gsi_fftrf_spread", "gsi_op_fft_at"):
        assert sym in gsi._lib.SIGNATURES
    hdr = open(os.path.join(ROOT, "include", "gsi_hip.h")).read()
    assert "int gsi_fftrf_spread(" in hdr and "int gsi_op_fft_at(" in hdr


class _HostGridOp:
    """A dense stand-in for the grid operator: `diagonal()` only calls matmul."""

    def __init__(self, Cm):
        self.C = Cm

    def matmul(self, X):
        return self.C @ X


@pytest.mark.parametrize("Ns,theta", [((7, 5), 0.6), ((2, 2), 0.3), ((2, 6), -0.4), ((4, 3, 2), 0.0)], ids=str)
def test_diagonal_needs_only_the_unit_lags(gsi, Ns, theta):
    import test_fft_gridcov_cpu as gc
    d = len(Ns)
    ell = (3.0, 1.5, 2.0)[:d]
    Cm = gc.dense_matrix(Ns, 1, ell, theta, 1.7, 0.01)
    P = im.scattered_points(Ns, 63, seed=8)
    box = im.inner_box(P)
    from gsi_amd import fftrf as F
    op = F.FFTOperatorAt.__new__(F.FFTOperatorAt)
    op.grid_op, op.Ns, op._P, op._B = _HostGridOp(Cm), tuple(Ns), np.asfortranarray(P), box
    base, frac = im.plan(P, Ns, box)
    W = am.weights_matrix(Ns, base, frac)
    ref = np.einsum("ij,jk,ik->i", W, Cm, W)
    assert np.abs(op.diagonal() - ref).max() <= 1e-13 * np.abs(ref).max()


# ---- 4. the sampler comparison's seed ----------------------------------------------------------------------------------
def test_sampler_seed_stays_inside_the_monte_carlo_bound():
    Ns, P, box = am.sampler_case()
    c = gm.case(Ns, None, "exponential", 6.0)
    lam = gm.spectrum(c)
    while gm.neg_mass(c, lam) > 1e-12:             # embed="auto": double every axis until the torus carries the covariance
        c = gm.case(Ns, tuple(2 * v for v in c.M), "exponential", 6.0)
        lam = gm.spectrum(c)
    F = gm.fields_from_eps(lam, Ns, am.sampler_noise(lam.size))
    base, frac = im.plan(P, Ns, box)
    W = am.weights_matrix(Ns, base, frac)
    V = W @ F
    emp = V @ V.T / am.SAMPLER_N
    A = W @ gm.dense_cov(c) @ W.T
    ratio = np.abs(emp - A).max() / am.sampler_bound()
    print(f"torus {c.M}: max |cov_model - A| / bound = {ratio:.3f}")
    assert ratio <= 1.0
