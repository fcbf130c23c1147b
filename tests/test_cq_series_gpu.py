"""The series form of a refinement round's Cholesky (cq_series_kernel, cholqr.hip).

cq_gram_round, the round of the sample-space tail, gets the Gram matrix of a panel that a first CholeskyQR round has made
orthonormal: I + E.  Where |E|_F <= 6e-6 one workgroup writes R = I + R1 + R2 and X = I - R1 + R1 R1 - R2 (R1 = Phi(E),
R2 = -Phi(R1'R1)) and the Cholesky kernel returns at once; above the gate, and with GSI_CQ_SERIES=0, the Cholesky runs as
before.  Through gsi_cq_gram_round (one round on a host matrix):

  * l = 1, 31, 32, 33, 320, 384 (one lane, under / at / over a 32-column block and a 4-column group, the headline width, the
    kernel's limit), E symmetric random at |E|_F = 1e-14 (first order only), 1e-7, 5.9e-6 (series) and 6.1e-6 (Cholesky);
  * in long double: |R'R - Gram|max and |X R - I|max <= 8 l eps, and R within that of a long-double Cholesky factor; R and X
    upper triangular with exact zeros below; the verdict 0; the branch that ran; |E|_F as the device measured it; two calls
    bit for bit;
  * with GSI_CQ_SERIES=0 (a child process: the switch is read once) the series never runs, and what the Cholesky branch gives
    here -- the 6.1e-6 cases and matrices far from I (which the series kernel looks at and leaves alone) -- is bit for bit what
    it gives there.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(np.float64).eps
LS = [1, 31, 32, 33, 320, 384]
NORMS = [1e-14, 1e-7, 5.9e-6, 6.1e-6]
GATE = 6e-6


def gram_near_identity(l, norm):
    rng = np.random.default_rng(1000 * l + int(-np.log10(norm) * 10))
    E = rng.standard_normal((l, l))
    E = E + E.T
    E *= norm / np.linalg.norm(E)
    return np.asfortranarray(np.eye(l) + E)


def gram_far(l):
    rng = np.random.default_rng(l)
    Y = rng.standard_normal((4 * l + 8, l)) * (np.arange(1, l + 1) ** -0.5)
    return np.asfortranarray(Y.T @ Y)


def cases():
    out = {f"l{l}_e{norm:g}": gram_near_identity(l, norm) for l in LS for norm in NORMS}
    out.update({f"l{l}_far": gram_far(l) for l in (33, 320)})
    return out


CHILD = r'''
import sys, numpy as np
import gsi_amd as gsi
src, dst = sys.argv[1], sys.argv[2]
ctx = gsi.Context(0)
data = np.load(src)
out = {}
for name in data.files:
    R, X, flag, series, norm = gsi.cq_gram_round(data[name], check=True, ctx=ctx)
    R2, X2, flag2, series2, norm2 = gsi.cq_gram_round(data[name], check=True, ctx=ctx)
    out[name + "/R"], out[name + "/X"] = R, X
    out[name + "/info"] = np.array([flag, series, norm, float(np.array_equal(R, R2) and np.array_equal(X, X2) and
                                                              (flag, series, norm) == (flag2, series2, norm2))])
np.savez(dst, **out)
'''


@pytest.fixture(scope="module")
def legs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("cq_series")
    grams = cases()
    np.savez(tmp / "in.npz", **grams)
    procs = {}
    for leg, value in (("on", None), ("off", "0")):
        env = dict(os.environ)
        env.pop("GSI_CQ_SERIES", None)
        if value is not None:
            env["GSI_CQ_SERIES"] = value
        procs[leg] = subprocess.Popen([sys.executable, "-c", CHILD, str(tmp / "in.npz"), str(tmp / (leg + ".npz"))],
                                      stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env, cwd=ROOT)
    out = {"gram": grams}
    for leg, pr in procs.items():
        so, se = pr.communicate(timeout=300)
        assert pr.returncode == 0, (leg, so[-2000:] + se[-4000:])
        out[leg] = dict(np.load(tmp / (leg + ".npz")))
    return out


def chol_longdouble(G):
    A = np.array(G, dtype=np.longdouble)
    l = A.shape[0]
    R = np.zeros_like(A)
    for j in range(l):                                    # row j of R from the rows above it
        v = A[j, j:] - R[:j, j].dot(R[:j, j:])
        R[j, j:] = v / np.sqrt(v[0])
    return R


@pytest.mark.parametrize("norm", NORMS)
@pytest.mark.parametrize("l", LS)
def test_round_near_identity(legs, l, norm):
    name = f"l{l}_e{norm:g}"
    G = legs["gram"][name]
    R, X = legs["on"][name + "/R"], legs["on"][name + "/X"]
    flag, series, dev_norm, same = legs["on"][name + "/info"]
    Rl, Xl, Gl = R.astype(np.longdouble), X.astype(np.longdouble), G.astype(np.longdouble)
    back = float(np.max(np.abs(Rl.T @ Rl - Gl)))
    inv = float(np.max(np.abs(Xl @ Rl - np.eye(l, dtype=np.longdouble))))
    fwd = float(np.max(np.abs(Rl - chol_longdouble(G))))
    host_norm = float(np.linalg.norm(G - np.eye(l)))
    bar = 8 * l * EPS
    print(f"\nl = {l}, |E|_F = {norm:g}: series {int(series)}, |R'R - G| {back:.2e}, |X R - I| {inv:.2e}, |R - chol| {fwd:.2e} "
          f"(bar {bar:.2e}); device |E|_F {dev_norm:.6e} (host {host_norm:.6e})")
    assert flag == 0 and same == 1.0
    assert int(series) == (1 if norm <= GATE else 0)
    assert abs(dev_norm - host_norm) <= 1e-12 * host_norm
    assert back <= bar and inv <= bar and fwd <= bar
    assert np.all(np.tril(R, -1) == 0.0) and np.all(np.tril(X, -1) == 0.0)
    assert np.all(np.isfinite(R)) and np.all(np.isfinite(X))


def test_switched_off_is_the_cholesky_everywhere(legs):
    for name in legs["gram"]:
        flag, series, dev_norm, same = legs["off"][name + "/info"]
        assert series == 0 and dev_norm == 0.0 and same == 1.0, name
        ran_cholesky = legs["on"][name + "/info"][1] == 0
        if ran_cholesky:                                  # above the gate and far from I: the parent's bits
            assert np.array_equal(legs["on"][name + "/R"], legs["off"][name + "/R"]), name
            assert np.array_equal(legs["on"][name + "/X"], legs["off"][name + "/X"]), name
            assert legs["on"][name + "/info"][0] == flag, name


@pytest.mark.parametrize("l", [33, 320])
def test_far_from_identity_runs_the_cholesky(legs, l):
    name = f"l{l}_far"
    G = legs["gram"][name]
    flag, series, dev_norm, same = legs["on"][name + "/info"]
    assert series == 0 and flag == 2 and same == 1.0          # (2: the refinement round's |G - I| <= 0.1 test, as before)
    assert dev_norm > GATE
    R = legs["on"][name + "/R"]
    Rl = R.astype(np.longdouble)
    rel = float(np.max(np.abs(Rl.T @ Rl - G.astype(np.longdouble)))) / float(np.max(np.abs(G)))
    assert rel <= 8 * l * EPS
    assert np.array_equal(R, legs["off"][name + "/R"]) and np.array_equal(legs["on"][name + "/X"], legs["off"][name + "/X"])
