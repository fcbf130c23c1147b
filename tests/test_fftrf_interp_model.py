"""FFTRF.interpolate as the device computes it, on the CPU.

1. The numpy restatement (tests/fftrf_interp_model.py) against scipy's RegularGridInterpolator on linspace(lo, hi, N) axes.
   scipy finds t by searching the axis and dividing by the local spacing, the contract by one division by a global step: t
   differs by a few N eps, and each axis contributes at most |dt| 2 max|V| to the value, so the bar is
   6 d max(N) eps max|V|.
2. Exactness at the nodes: points equal to the grid nodes return vec(V) bit for bit, f = 1 in the last cell included.
3. The host planner (csrc/fftrf_points.hpp) built stand-alone under the address and undefined-behaviour sanitizers: its
   plan equals the numpy plan bit for bit -- index and every f --, and it refuses what the header says it refuses.
4. The Python entry points raise ValueError on a wrong shape before any library call (no context is created here)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import fftrf_interp_model as im

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(np.float64).eps


# ---- 1. the model against scipy ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("Ns", im.MODEL_GRIDS, ids=im.gid)
def test_model_matches_scipy(Ns):
    from scipy.interpolate import RegularGridInterpolator
    rng = np.random.default_rng([11] + list(Ns))
    P = rng.standard_normal((len(Ns), 1000))
    V = rng.standard_normal(Ns)
    lo, hi = im.extent(P)
    rgi = RegularGridInterpolator([np.linspace(lo[a], hi[a], Ns[a]) for a in range(len(Ns))], V, method="linear",
                                  bounds_error=False, fill_value=None)
    ref = rgi(P.T)
    got = im.interpolate(P, V, Ns)[:, 0]
    bar = 6 * len(Ns) * max(Ns) * EPS * np.abs(V).max()
    err = np.abs(got - ref).max()
    print(im.gid(Ns), "max error", err, "bar", bar, "in max(N) eps max|V|:", err / (max(Ns) * EPS * np.abs(V).max()))
    assert err <= bar


# ---- 2. exactness at the nodes -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale,shift", [(1.0, 0.0), (0.25, 1024.0)], ids=["integer", "quarter+1024"])
@pytest.mark.parametrize("Ns", im.MODEL_GRIDS, ids=im.gid)
def test_nodes_return_the_field_bit_for_bit(Ns, scale, shift):
    V = im.random_fields(Ns, 2, seed=3)
    P = im.node_points(Ns, scale, shift)
    base, frac = im.plan(P, Ns)
    assert np.array_equal(base + (frac[0] == 1.0) + sum((frac[a] == 1.0) * int(np.prod(Ns[:a])) for a in range(1, len(Ns))),
                          np.arange(int(np.prod(Ns))))
    assert np.isin(frac, (0.0, 1.0)).all()
    assert np.array_equal(im.interp(V, Ns, base, frac), V)


# ---- 3. the planner under sanitizers -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build the planner check"
    exe = str(tmp_path_factory.mktemp("fftrf_points") / "fftrf_points_check")
    src = os.path.join(ROOT, "tests", "fftrf_points_check.cpp")
    inc = os.path.join(ROOT, "geostatinversion.jl_amd", "csrc")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", inc, src, "-o", exe], check=True)
    return exe


def _run_planner(exe, tmp_path, Ns, P, box=None, row0=0, rows=None, m=None, ndims=None):
    d = len(Ns) if ndims is None else ndims
    m = P.shape[1] if m is None else m
    rows = m - row0 if rows is None else rows
    N3 = list(Ns) + [1] * (3 - len(Ns))
    case, out = str(tmp_path / "case.bin"), str(tmp_path / "plan.bin")
    if os.path.exists(out):
        os.remove(out)
    with open(case, "wb") as f:
        np.array([d] + N3[:3] + [m, int(box is not None), row0, rows], dtype=np.int64).tofile(f)
        np.asfortranarray(P, dtype=np.float64).reshape(-1, order="F").tofile(f)
        if box is not None:
            np.asarray(box, dtype=np.float64).tofile(f)
    r = subprocess.run([exe, case, out], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    if r.stdout.startswith("refused:"):
        assert not os.path.exists(out)
        return r.stdout.strip(), None, None
    raw = open(out, "rb").read()
    base = np.frombuffer(raw[:4 * rows], dtype=np.int32)
    frac = np.frombuffer(raw[4 * rows:], dtype=np.float64).reshape(d, rows)
    return r.stdout.strip(), base, frac


@pytest.mark.parametrize("Ns", im.MODEL_GRIDS, ids=im.gid)
def test_planner_equals_the_numpy_plan_bit_for_bit(planner, tmp_path, Ns):
    P = im.scattered_points(Ns, 1000, seed=5)
    box = im.inner_box(P)
    nodes = im.node_points(Ns, 0.25, 1024.0)
    for pts, kw in ((P, {}), (P, {"row0": 7, "rows": 333}), (P, {"box": box}), (P, {"box": box, "row0": 501, "rows": 499}),
                    (nodes, {})):
        msg, base, frac = _run_planner(planner, tmp_path, Ns, pts, **kw)
        assert base is not None, msg
        ref_base, ref_frac = im.plan(pts, Ns, kw.get("box"), kw.get("row0", 0), kw.get("rows"))
        assert np.array_equal(base, ref_base), kw
        assert np.array_equal(frac, ref_frac), kw
        assert frac.min() >= 0.0 and frac.max() <= 1.0
        top = np.array(Ns) - 2
        idx = np.stack(np.unravel_index(base, Ns, order="F"))
        assert (idx <= top[:, None]).all() and base.min() >= 0
    # the box is smaller than the points' extent: the clamp acted at both ends
    _, base, frac = _run_planner(planner, tmp_path, Ns, P, box=box)
    assert (frac == 0.0).any() and (frac == 1.0).any()


def test_planner_refusals(planner, tmp_path):
    Ns = (5, 4)
    P = im.scattered_points(Ns, 50, seed=1)

    def refused(word, Ns=Ns, P=P, **kw):
        msg, base, _ = _run_planner(planner, tmp_path, Ns, P, **kw)
        assert base is None and msg.startswith("refused:") and word in msg, (word, msg)

    refused("N[a] >= 2", Ns=(1, 7))
    refused("N[a] >= 2", Ns=(5, 3, 1), P=im.scattered_points((5, 3, 2), 50))
    refused("m >= 1", m=0, rows=0)
    refused("dimension", ndims=1)
    refused("dimension", ndims=4, P=np.zeros((4, 50)))
    for bad in (np.nan, np.inf, -np.inf):
        Q = P.copy()
        Q[1, 17] = bad
        refused("finite", P=Q)
    box = im.inner_box(P)
    for bad in (np.nan, np.inf):
        b = box.copy()
        b[3] = bad
        refused("finite", box=b)
    Q = P.copy()
    Q[0, :] = 2.5
    refused("extent", P=Q)                                   # every point at the same coordinate
    Q = P.copy()
    Q[0, 0], Q[0, 1] = 1.5e308, -1.5e308
    refused("extent", P=Q)                                   # hi - lo overflows
    refused("extent", box=np.array([0.0, 1.0, 0.0, 2.0]))    # lo_0 = hi_0
    refused("hi >= lo", box=np.array([0.0, 1.0, 1.0, 0.5]))
    refused("rows", row0=40, rows=11)
    refused("rows", row0=-1, rows=5)


# ---- 4. shape errors of the Python entry points -------------------------------------------------------------------------
def test_shape_errors_come_before_any_library_call(gsi, monkeypatch):
    from gsi_amd import context as cx_mod
    monkeypatch.setattr(cx_mod, "_default_ctx", None)
    F = gsi.FFTRF
    Ns, args = (5, 4), (0.0, 1.0, -3.5)
    good = np.zeros((2, 9))
    for bad in (np.zeros((3, 9)), np.zeros((9, 2)), np.zeros(9), np.zeros((2, 0))):
        with pytest.raises(ValueError):
            F.powerlaw_unstructuredgrid(bad, Ns, *args)
        with pytest.raises(ValueError):
            F.powerlaw_fields_at(None, bad, Ns, *args, 3)
        with pytest.raises(ValueError):
            F.interpolate(None, bad, np.zeros((20, 1)), Ns)
        with pytest.raises(ValueError):
            gsi.lowrank_fftrf_operator(None, Ns, *args, 8, points=bad)
        with pytest.raises(ValueError):
            gsi.getxis_fftrf(Ns, *args, 8, 3, 2, points=bad)
    for bad_box in ([0.0, 1.0, 2.0], np.zeros(6), np.zeros((2, 3))):
        with pytest.raises(ValueError):
            F.powerlaw_unstructuredgrid(good, Ns, *args, box=bad_box)
        with pytest.raises(ValueError):
            F.powerlaw_fields_at(None, good, Ns, *args, 3, box=bad_box)
        with pytest.raises(ValueError):
            F.interpolate(None, good, np.zeros((20, 1)), Ns, box=bad_box)
        with pytest.raises(ValueError):
            gsi.lowrank_fftrf_operator(None, Ns, *args, 8, points=good, box=bad_box)
        with pytest.raises(ValueError):
            gsi.getxis_fftrf(Ns, *args, 8, 3, 2, points=good, box=bad_box)
    with pytest.raises(ValueError):
        gsi.getxis_fftrf(Ns, *args, 8, 3, 2, box=np.zeros(4))           # a box without points
    with pytest.raises(ValueError):
        F.powerlaw_unstructuredgrid(np.zeros((3, 9)), (5, 4, 3, 2), *args)
    assert cx_mod._default_ctx is None                                  # nothing created a context
