"""The single-rank LU updates its 64-column blocks LEFT-looking (panel_lu_blocks.hip: lu_leftlook_kernel, lu_urows_kernel):
block i's columns are brought up to date once, before its leaves, with every finished block to their left.  The factors must
be bit for bit those of the right-looking row-sharded form (lus_u12_block / lus_rankk, the reference) and the pivots dgetrf's.
Shapes here: the headline panel (five full blocks) with ties, several full blocks plus a ragged last block, an overflow-row
panel with five blocks, and 32-column blocks."""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import oracle as orc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _panel(m, l, ties):
    rng = np.random.default_rng(m + l)
    Y = rng.standard_normal((m, l))
    if ties:                        # equal-magnitude maxima far apart, across workgroups: the lowest row must win
        for j in range(0, l, 3):
            r = rng.choice(m, size=3, replace=False)
            Y[r, j] = [7.5, -7.5, 7.5]
    return Y


def _child(code, env_extra, out):
    env = dict(os.environ)
    env.update(env_extra)
    r = subprocess.run([sys.executable, "-c", code, out], capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
    assert r.returncode == 0 and "lu-ok" in r.stdout, str(env_extra) + "\n" + r.stdout[-2000:] + r.stderr[-4000:]
    return np.load(out)


def test_lu_headline_panel_bit_identical_to_sharded(gsi):
    Y = _panel(1000000, 320, True)
    ctx = gsi.default_context()
    L, p = gsi.lu_L(Y, return_pivots=True, ctx=ctx)
    Ls, ps = gsi.lu_L_sharded(Y, return_pivots=True, ctx=ctx)
    assert np.array_equal(p, ps)
    assert np.array_equal(L, Ls)
    assert np.array_equal(p, orc.lu_pivots(Y))


_CODE = r"""
import os, sys, numpy as np
sys.path.insert(0, os.getcwd()); sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
import gsi_amd as gsi
from test_lu_leftlook_gpu import _panel
ctx = gsi.Context(0)
res = {}
for idx, (m, l, sharded) in enumerate([(300000, 200, True), (1100000, 320, False)]):
    Y = _panel(m, l, True)
    L, piv = gsi.lu_L(Y, return_pivots=True, ctx=ctx)
    if sharded and os.environ.get("GSI_LU_TALL") != "1":
        Ls, ps = gsi.lu_L_sharded(Y, return_pivots=True, ctx=ctx)
        assert np.array_equal(ps, piv) and np.array_equal(Ls, L), (m, l)
    res["L%d" % idx] = L
    res["p%d" % idx] = piv
np.savez(sys.argv[1], **res)
print("lu-ok")
"""


def test_lu_ragged_and_overflow_panels_streamed_equals_resident(tmp_path):
    """300 000 x 200 (64 + 64 + 64 + 8 columns) and 1 100 000 x 320 (resident kernel with overflow rows, five blocks): the
    streamed leaves (GSI_LU_TALL=1) and the resident kernel give the same bits; the first also equals the sharded form."""
    res = _child(_CODE, {}, str(tmp_path / "resident.npz"))
    stm = _child(_CODE, {"GSI_LU_TALL": "1"}, str(tmp_path / "streamed.npz"))
    for k in res.files:
        assert np.array_equal(res[k], stm[k]), k
    Y = _panel(300000, 200, True)
    assert np.array_equal(res["p0"], orc.lu_pivots(Y))


def test_lu_32_column_blocks_match_lapack(tmp_path):
    code = r"""
import os, sys, numpy as np
sys.path.insert(0, os.getcwd()); sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
import gsi_amd as gsi
from oracle import oracle as orc
from test_lu_leftlook_gpu import _panel
Y = _panel(70001, 160, True)
L, piv = gsi.lu_L(Y, return_pivots=True, ctx=gsi.Context(0))
assert np.array_equal(piv, orc.lu_pivots(Y))
Lref = orc.lu_L(Y)
assert np.abs(L - Lref).max() < 1e-10 * max(1.0, np.abs(Lref).max())
np.savez(sys.argv[1], L=L)
print("lu-ok")
"""
    _child(code, {"GSI_LU_NB": "32"}, str(tmp_path / "nb32.npz"))
