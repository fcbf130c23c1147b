"""Numpy model of the adjoint of a sparse forward model (csrc/fwd_adjoint_plan.hpp, csrc/fwd_adjoint.hip)
and the shared inputs of its tests (test_fwd_adjoint_model.py, test_fwd_cov_cpu.py, test_fwd_adjoint_gpu.py,
test_fwd_cov_gpu.py).  Not a test module.

`plan` restates the C++ planner array for array; `adjoint` sums in the plan's order in float64 -- numpy rounds every product
and every sum on its own, which is what the kernels and the host path do -- and is what the device is held to bit for bit;
`adjoint_ld` is the same sum in longdouble, `adjoint_abs` the sum of the absolute terms, the scale of the rounding bound
    |G - G_ref|[j, c] <= (k_j + 4) 2^-53 sum_t |h_t| |V[r_t, c]|
(k_j - 1 additions, one product, the one rounding of vals * w; the rest is second-order slack)."""
import functools
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "geostatinversion.jl_amd", "csrc")
EPS = 2.0 ** -53
LD = np.longdouble
# the planner's chunk limit and the kernels' column group, from the sources
CHUNK = int(re.search(r"FADJ_CHUNK\s*=\s*(\d+)", open(os.path.join(CSRC, "fwd_adjoint_plan.hpp")).read()).group(1))
COLS = int(re.search(r"FADJ_COLS\s*=\s*(\d+)", open(os.path.join(CSRC, "fwd_adjoint.hip")).read()).group(1))


def plan(indptr, indices, data, n, w=None, chunk=CHUNK):
    """The arrays of `fwd_adjoint_plan`, as a dict of numpy arrays."""
    indptr = np.asarray(indptr, dtype=np.int64)
    nnz = int(indptr[-1])
    indices = np.asarray(indices, dtype=np.int64)[:nnz]
    data = np.asarray(data, dtype=np.float64)[:nnz]
    nobs = len(indptr) - 1
    rows = np.repeat(np.arange(nobs, dtype=np.int64), np.diff(indptr))
    order = np.argsort(indices, kind="stable")              # by cell; within a cell in storage order = ascending row
    colptr = np.zeros(n + 1, dtype=np.int64)
    np.add.at(colptr, indices + 1, 1)
    colptr = np.cumsum(colptr)
    val = data if w is None else data * np.asarray(w, dtype=np.float64)[indices]      # one rounding
    lens = np.diff(colptr)
    long_col = np.flatnonzero(lens > chunk)
    long_chunk0, chunk_off, chunk_len = [0], [], []
    for j in long_col:
        for o in range(0, int(lens[j]), chunk):
            chunk_off.append(int(colptr[j]) + o)
            chunk_len.append(min(chunk, int(lens[j]) - o))
        long_chunk0.append(len(chunk_off))
    return dict(n=n, nobs=nobs, nnz=nnz, chunk=chunk, colptr=colptr, row=rows[order].astype(np.int32), val=val[order],
                long_col=long_col.astype(np.int32), long_chunk0=np.array(long_chunk0, dtype=np.int64),
                chunk_off=np.array(chunk_off, dtype=np.int64), chunk_len=np.array(chunk_len, dtype=np.int32),
                maxlen=int(lens.max()) if n else 0)


def _list_sum(pl, e0, e1, V, dtype, absolute):
    acc = np.zeros(V.shape[1], dtype=dtype)
    for e in range(e0, e1):
        h, v = dtype(pl["val"][e]), V[pl["row"][e]]
        acc = acc + (abs(h) * np.abs(v) if absolute else h * v)
    return acc


def _adjoint(pl, V, dtype, absolute=False):
    V = np.asarray(V, dtype=np.float64).reshape(pl["nobs"], -1).astype(dtype)
    G = np.zeros((pl["n"], V.shape[1]), dtype=dtype)
    cp, ch = pl["colptr"], pl["chunk"]
    for j in np.flatnonzero(np.diff(cp) > 0):
        e0, e1 = int(cp[j]), int(cp[j + 1])
        if e1 - e0 <= ch:
            G[j] = _list_sum(pl, e0, e1, V, dtype, absolute)
            continue
        s = None
        for o in range(e0, e1, ch):                           # each chunk from zero, the chunk sums in chunk order
            part = _list_sum(pl, o, min(o + ch, e1), V, dtype, absolute)
            s = part if s is None else s + part
        G[j] = s
    return G


def adjoint(pl, V):
    """H' V in the plan's order, float64: the bits the device and the host path return."""
    return _adjoint(pl, V, np.float64)


def adjoint_ld(pl, V):
    return _adjoint(pl, V, LD)


def adjoint_abs(pl, V):
    return _adjoint(pl, V, LD, absolute=True)


def dense(indptr, indices, data, n, w=None):
    """H with the weights folded in, dense; repeated indices add."""
    nobs = len(indptr) - 1
    nnz = int(indptr[-1])
    rows = np.repeat(np.arange(nobs), np.diff(indptr))
    H = np.zeros((nobs, n))
    np.add.at(H, (rows, np.asarray(indices)[:nnz]), np.asarray(data)[:nnz])
    return H if w is None else H * np.asarray(w)[None, :]


# ---------------------------------------------------------------- inputs
def _csr_from_triples(nobs, r, j, v, rng):
    """CSR with the entries of every row in random (unsorted) storage order."""
    key = rng.permutation(len(r))
    r, j, v = np.asarray(r)[key], np.asarray(j)[key], np.asarray(v)[key]
    order = np.argsort(r, kind="stable")
    indptr = np.zeros(nobs + 1, dtype=np.int64)
    np.add.at(indptr, r + 1, 1)
    return np.cumsum(indptr), j[order].astype(np.int64), v[order].astype(np.float64)


FAN_LENGTHS = [0, 1, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK, 2 * CHUNK + 1, 3 * CHUNK + 5]


@functools.lru_cache(maxsize=None)
def fan(n, values="randn", seed=0):
    """The crafted H of the tests: nobs = 3 CHUNK + 5 rows over n cells.  Eight cells, the first and the last of the grid
    among them, have lists of exactly FAN_LENGTHS contributions; the others 0 to 3.  Rows 5 and nobs - 2 are empty, so the
    longest list reaches its 3 CHUNK + 5 contributions through repeated indices inside a row; entries of a row are stored
    unsorted.  values: "randn", or "int" (+-2^k, k in 0..3).  Returns (indptr, indices, data, lengths per cell)."""
    rng = np.random.default_rng([n, seed, len(values)])
    nobs = 3 * CHUNK + 5
    live = np.array([r for r in range(nobs) if r not in (5, nobs - 2)])
    special = np.unique(np.concatenate([[0, n - 1], rng.choice(np.arange(1, n - 1), size=len(FAN_LENGTHS) - 2, replace=False)]))
    lengths = rng.integers(0, 4, size=n)
    lengths[special] = rng.permutation(FAN_LENGTHS)
    r, j = [], []
    for cell in np.flatnonzero(lengths):
        ln = int(lengths[cell])
        rows = rng.choice(live, size=min(ln, len(live)), replace=False)
        if ln > len(live):                                   # repeats inside a row
            rows = np.concatenate([rows, rng.choice(live, size=ln - len(live), replace=False)])
        elif ln >= 3:
            rows[-1] = rows[0]
        r.append(rows)
        j.append(np.full(ln, cell))
    r, j = np.concatenate(r), np.concatenate(j)
    v = (rng.choice([-1.0, 1.0], size=len(r)) * 2.0 ** rng.integers(0, 4, size=len(r))) if values == "int" \
        else rng.standard_normal(len(r))
    indptr, indices, data = _csr_from_triples(nobs, r, j, v, rng)
    for a in (indptr, indices, data, lengths):
        a.setflags(write=False)
    return indptr, indices, data, lengths


def weights(n, seed=3):
    return 1.0 + 0.1 * np.random.default_rng(seed).standard_normal(n)


@functools.lru_cache(maxsize=None)
def rays(Ns, nrays=40, nsamp=64, npoints=20, seed=0):
    """The H of the operator tests on the grid Ns (vec() order): `nrays` straight rays of `nsamp` samples each (a ray is the average of
    its samples: the cell a sample falls in gets 1 / nsamp; samples in one cell repeat its index and add), `npoints` point samples, one
    row that repeats row 0, one empty row.  Returns (indptr, indices, data)."""
    rng = np.random.default_rng([seed, *Ns])
    d = len(Ns)
    strides = np.cumprod([1] + list(Ns[:-1]))
    top = np.array(Ns, dtype=float) - 1e-9
    rows = []
    for _ in range(nrays):
        a, b = rng.random(d) * top, rng.random(d) * top
        t = (np.arange(nsamp) + 0.5) / nsamp
        pts = a[:, None] + (b - a)[:, None] * t[None, :]
        cells = (np.floor(pts).astype(np.int64) * strides[:, None]).sum(axis=0)
        rows.append((cells, np.full(nsamp, 1.0 / nsamp)))
    n = int(np.prod(Ns))
    for c in rng.choice(n, size=npoints, replace=False):
        rows.append((np.array([c], dtype=np.int64), np.array([1.0])))
    rows.append(rows[0])
    rows.append((np.zeros(0, dtype=np.int64), np.zeros(0)))
    indptr = np.zeros(len(rows) + 1, dtype=np.int64)
    indptr[1:] = np.cumsum([len(c) for c, _ in rows])
    indices = np.concatenate([c for c, _ in rows])
    data = np.concatenate([v for _, v in rows])
    for a in (indptr, indices, data):
        a.setflags(write=False)
    return indptr, indices, data
