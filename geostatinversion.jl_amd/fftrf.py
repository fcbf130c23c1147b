"""Host-side mirror of `FFTRF.powerlaw_structuredgrid` (FFTRF.jl:83-100) and `FFTRF.powerlaw_unstructuredgrid`
(FFTRF.jl:102-129) with the fields sampled, and read at scattered points, on the device (`gsi_fftrf_fields`,
csrc/fftrf_sample.hip; `gsi_fftrf_fields_at`, `gsi_fftrf_interpolate`, csrc/fftrf_interp.hip).  The reference's own
functions stay what they are, and a caller's own `samplefield` closure keeps working with `getxis`; this is the path for
grids and meshes whose fields should never leave HBM."""
import ctypes as C

import numpy as np

from . import _lib as L
from . import randmatfact as RMF
from .context import DeviceMatrix, Operator, default_context


def _grid(Ns):
    Ns = [int(v) for v in Ns]
    return Ns, (C.c_int64 * len(Ns))(*Ns)


def _points_args(points, box, ndims):
    """`points` as an ndims x m column-major array and `box` as 2 ndims doubles (lo then hi) or None; ValueError on a wrong
    shape, before any library call."""
    P = np.asarray(points, dtype=np.float64)
    if ndims not in (2, 3) or P.ndim != 2 or P.shape[0] != ndims or P.shape[1] < 1:
        raise ValueError(f"points must be ndims x m = {ndims} x m with m >= 1 (one column per point), ndims 2 or 3")
    P = np.asfortranarray(P)
    B = None
    if box is not None:
        B = np.ascontiguousarray(np.asarray(box, dtype=np.float64).reshape(-1))
        if B.size != 2 * ndims:
            raise ValueError(f"box must hold 2 ndims = {2 * ndims} values: lo of every axis, then hi of every axis")
    return P, B


def _box_ptr(B):
    return L.dptr(B) if B is not None else None


def phi_shape(Ns):
    """`size(S)` of `mulbyphi` (FFTRF.jl:75): (2 N_2, 2 N_1[, 2 N_3]) -- the reference's axis swap."""
    Ns = [int(v) for v in Ns]
    return tuple(2 * N for N in ([Ns[1], Ns[0]] + Ns[2:] if len(Ns) >= 2 else Ns))


def _phi_matrix(phi, Ns, numfields):
    shp = phi_shape(Ns)
    if len(phi) != int(numfields):
        raise ValueError("phi must hold one array per field")
    ph = np.empty((int(np.prod(shp)), int(numfields)), order="F")
    for c in range(int(numfields)):
        pc = np.asarray(phi[c], dtype=np.float64)
        if pc.shape != shp:
            raise ValueError(f"phi[{c}] must have the reference's size(S) = {shp}")
        ph[:, c] = pc.reshape(-1, order="F")          # vec()
    return ph


def powerlaw_fields(ctx, Ns, k0, dk, beta, numfields, *, seed=0, field0=0, phi=None):
    """`numfields` fields of `powerlaw_structuredgrid(Ns, k0, dk, beta)` as a `DeviceMatrix` of n x numfields, column c =
    vec() of field `field0 + c`.  `phi`: a sequence of `numfields` arrays of shape `phi_shape(Ns)` (what `randn(size(S))`
    returns for each field); without it field f draws the stream
    `DeviceMatrix(ctx, Mtot, 1).randn(seed + f)`."""
    Ns, arr = _grid(Ns)
    n = int(np.prod(Ns))
    F = DeviceMatrix(ctx, n, int(numfields))
    try:
        if phi is None:
            L.check(ctx.lib.gsi_fftrf_fields(ctx.h, F.h, len(Ns), arr, float(k0), float(dk), float(beta), None, 0,
                                             int(seed) % (1 << 64), int(field0)), ctx.lib)
        else:
            ph = _phi_matrix(phi, Ns, numfields)
            L.check(ctx.lib.gsi_fftrf_fields(ctx.h, F.h, len(Ns), arr, float(k0), float(dk), float(beta), L.dptr(ph),
                                             ph.shape[0], 0, 0), ctx.lib)
    except Exception:
        F.close()
        raise
    return F


def powerlaw_structuredgrid(Ns, k0, dk, beta, *, phi=None, seed=None, ctx=None):
    """`FFTRF.powerlaw_structuredgrid(Ns, k0, dk, beta)` -> ndarray of shape `Ns`.  `phi`: the `randn(size(S))` array of
    `mulbyphi`; `seed`: the device stream of `powerlaw_fields(..., seed=seed)`, field 0; neither: phi is drawn from
    `RandMatFact.randn`, the package's host stream, so `RandMatFact.seed` governs it as `Random.seed!` does in Julia."""
    ctx = ctx or default_context()
    Ns = [int(v) for v in Ns]
    if phi is None and seed is None:
        shp = phi_shape(Ns)
        phi = RMF.randn(int(np.prod(shp)), 1).reshape(shp, order="F")
    if phi is not None:
        F = powerlaw_fields(ctx, Ns, k0, dk, beta, 1, phi=[np.asarray(phi, dtype=np.float64)])
    else:
        F = powerlaw_fields(ctx, Ns, k0, dk, beta, 1, seed=seed)
    try:
        return F.to_host()[:, 0].reshape(Ns, order="F")
    finally:
        F.close()


def powerlaw_fields_at(ctx, points, Ns, k0, dk, beta, numfields, *, seed=0, field0=0, phi=None, box=None, row0=0, rows=None):
    """`numfields` fields of `powerlaw_unstructuredgrid(points, Ns, k0, dk, beta)` as a `DeviceMatrix` of m x numfields
    (`gsi_fftrf_fields_at`): the fields of `powerlaw_fields` (same `phi` / `seed` / `field0`) interpolated at `points`
    (ndims x m, one column per point) without the n x numfields structured matrix ever being formed.  `box` (lo of every
    axis, then hi) replaces the points' own extrema; `row0`, `rows`: only the points [row0, row0 + rows)."""
    Ns, arr = _grid(Ns)
    P, B = _points_args(points, box, len(Ns))
    m = P.shape[1]
    rows = m - int(row0) if rows is None else int(rows)
    F = DeviceMatrix(ctx, rows, int(numfields))
    try:
        if phi is None:
            L.check(ctx.lib.gsi_fftrf_fields_at(ctx.h, F.h, len(Ns), arr, float(k0), float(dk), float(beta), None, 0,
                                                int(seed) % (1 << 64), int(field0), L.dptr(P), m, _box_ptr(B), int(row0)),
                    ctx.lib)
        else:
            ph = _phi_matrix(phi, Ns, numfields)
            L.check(ctx.lib.gsi_fftrf_fields_at(ctx.h, F.h, len(Ns), arr, float(k0), float(dk), float(beta), L.dptr(ph),
                                                ph.shape[0], 0, 0, L.dptr(P), m, _box_ptr(B), int(row0)), ctx.lib)
    except Exception:
        F.close()
        raise
    return F


def interpolate(ctx, points, F, Ns, *, box=None, row0=0, rows=None):
    """`FFTRF.interpolate(points, field, Val{ndims})` (FFTRF.jl:107-129) for every column of `F` (`gsi_fftrf_interpolate`):
    `F` is a `DeviceMatrix` of n x nf, column c = vec() of a field of shape `Ns` (or a host array of that shape, uploaded);
    returns a `DeviceMatrix` of m x nf.  Linear interpolation on the grid spanned by the points' extrema (or `box`), flat
    beyond it."""
    Ns, arr = _grid(Ns)
    P, B = _points_args(points, box, len(Ns))
    m = P.shape[1]
    rows = m - int(row0) if rows is None else int(rows)
    own = not isinstance(F, DeviceMatrix)
    G = DeviceMatrix.from_host(ctx, np.asarray(F, dtype=np.float64).reshape(int(np.prod(Ns)), -1, order="F")) if own else F
    try:
        out = DeviceMatrix(ctx, rows, G.shape[1])
        try:
            L.check(ctx.lib.gsi_fftrf_interpolate(ctx.h, out.h, G.h, len(Ns), arr, L.dptr(P), m, _box_ptr(B), int(row0)),
                    ctx.lib)
        except Exception:
            out.close()
            raise
        return out
    finally:
        if own:
            G.close()


def powerlaw_unstructuredgrid(points, Ns, k0, dk, beta, *, phi=None, seed=None, box=None, ctx=None):
    """`FFTRF.powerlaw_unstructuredgrid(points, Ns, k0, dk, beta)` -> ndarray of m values, one per column of `points`.
    `phi`, `seed`: as in `powerlaw_structuredgrid`; `box`: the grid's extent instead of the points' extrema."""
    Ns = [int(v) for v in Ns]
    _points_args(points, box, len(Ns))
    ctx = ctx or default_context()
    if phi is None and seed is None:
        shp = phi_shape(Ns)
        phi = RMF.randn(int(np.prod(shp)), 1).reshape(shp, order="F")
    if phi is not None:
        F = powerlaw_fields_at(ctx, points, Ns, k0, dk, beta, 1, phi=[np.asarray(phi, dtype=np.float64)], box=box)
    else:
        F = powerlaw_fields_at(ctx, points, Ns, k0, dk, beta, 1, seed=seed, box=box)
    try:
        return F.to_host()[:, 0].copy()
    finally:
        F.close()


def lowrank_fftrf_operator(ctx, Ns, k0, dk, beta, numfields, seed=0, *, points=None, box=None):
    """`LowRankCovMatrix` over `numfields` device-sampled FFTRF fields (`gsi_op_lowrank_fftrf`): generated, centred and
    kept in HBM.  Row-sharded like every operator: each rank generates every field and keeps its own rows.  With `points`
    (ndims x m) the fields are those of `powerlaw_unstructuredgrid` and the operator is m x m (`gsi_op_lowrank_fftrf_at`);
    every rank holds all points."""
    Ns, arr = _grid(Ns)
    h = C.c_void_p()
    if points is None:
        if box is not None:
            raise ValueError("box applies to points: pass points as well")
        row0, nloc = ctx.shard(int(np.prod(Ns)))
        L.check(ctx.lib.gsi_op_lowrank_fftrf(ctx.h, C.byref(h), len(Ns), arr, float(k0), float(dk), float(beta), int(numfields),
                                             int(seed) % (1 << 64), row0, nloc), ctx.lib)
    else:
        P, B = _points_args(points, box, len(Ns))
        m = P.shape[1]
        row0, mloc = ctx.shard(m)
        L.check(ctx.lib.gsi_op_lowrank_fftrf_at(ctx.h, C.byref(h), len(Ns), arr, float(k0), float(dk), float(beta),
                                                int(numfields), int(seed) % (1 << 64), L.dptr(P), m, _box_ptr(B), row0, mloc),
                ctx.lib)
    return Operator(ctx, h)
