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


def spread(ctx, points, V, Ns, *, box=None):
    """The adjoint of `interpolate` (`gsi_fftrf_spread`): `V` is a `DeviceMatrix` of m x nf (or a host array, uploaded) of
    values at the m `points`; returns a `DeviceMatrix` of n x nf, n = prod(Ns), whose entry (g, c) is the sum over the points
    that have node g as a corner of their cell of weight * V[p, c], with `interpolate`'s weights: W' V where
    `interpolate` applies W.  Bins point data onto the grid; every entry is written, untouched nodes are exactly 0.0, and
    the result is bit-identical from call to call (no atomics: fixed summation order per node)."""
    Ns, arr = _grid(Ns)
    P, B = _points_args(points, box, len(Ns))
    m = P.shape[1]
    own = not isinstance(V, DeviceMatrix)
    if own:
        Vh = np.asarray(V, dtype=np.float64)
        X = DeviceMatrix.from_host(ctx, Vh.reshape(Vh.shape[0], -1))
    else:
        X = V
    try:
        if X.shape[0] < m:
            raise ValueError(f"V must have one row per point: {m} rows, not {X.shape[0]}")
        out = DeviceMatrix(ctx, int(np.prod(Ns)), X.shape[1])
        try:
            L.check(ctx.lib.gsi_fftrf_spread(ctx.h, out.h, X.h, len(Ns), arr, L.dptr(P), m, _box_ptr(B), 0), ctx.lib)
        except Exception:
            out.close()
            raise
        return out
    finally:
        if own:
            X.close()


def _host_plan(P, Ns, B):
    """fftrf_points.hpp in numpy, operation for operation: (lo, hi, base index per axis, frac per axis) of the points."""
    d, m = P.shape
    lo = P.min(axis=1) if B is None else B[:d].copy()
    hi = P.max(axis=1) if B is None else B[d:].copy()
    cell = np.empty((d, m), dtype=np.int64)
    frac = np.empty((d, m))
    for a in range(d):
        step = (hi[a] - lo[a]) / float(Ns[a] - 1)
        top = float(Ns[a] - 1)
        t = np.minimum(np.maximum((P[a] - lo[a]) / step, 0.0), top)
        fl = np.minimum(np.floor(t), top - 1.0)
        cell[a] = fl.astype(np.int64)
        frac[a] = t - fl
    return lo, hi, cell, frac


class FFTOperatorAt(Operator):
    """`fft_operator_at`'s result: the m x m operator W C W' (`gsi_op_fft_at`).  `grid_op` stays referenced; `steps` is the
    physical size of a grid spacing per axis, (hi - lo) / (N - 1): the grid operator's `ell` is in GRID SPACINGS, so a
    physical length L along axis a is L / steps[a] spacings (a grid whose steps differ per axis needs per-axis `ell`)."""

    def __init__(self, ctx, h, grid_op, Ns, P, B):
        super().__init__(ctx, h)
        self.grid_op = grid_op
        self.Ns = tuple(Ns)
        self._P, self._B = P, B
        d = len(self.Ns)
        self.lo = P.min(axis=1) if B is None else B[:d].copy()
        self.hi = P.max(axis=1) if B is None else B[d:].copy()
        self.steps = (self.hi - self.lo) / (np.asarray(Ns, dtype=np.float64) - 1.0)

    def diagonal(self):
        """diag(W C W'), the prior variances at the points (what `posterior_variance(..., prior_variance=...)` wants), on
        the host.  C is block Toeplitz, so a point's variance is the sum over pairs of corners of its cell of
        w_a w_b c(a - b) and needs c at the lags {-1, 0, 1}^d only: they are read from 2^(d-1) unit-vector columns of the
        grid operator (c(-t) = c(t) gives the rest).  Nothing m x m or n x n is formed.  A nugget of the grid operator is
        part of c(0) and is interpolated like everything else."""
        Ns, d = self.Ns, len(self.Ns)
        n = int(np.prod(Ns))
        strides = np.cumprod([1] + list(Ns[:-1]))
        # unit vectors at the nodes (0, j1[, j2]), j in {0, 1}: column j holds c(i - j) for every node i
        js = [(0,) + tuple((k >> a) & 1 for a in range(d - 1)) for k in range(1 << (d - 1))]
        E = np.zeros((n, len(js)), order="F")
        for k, j in enumerate(js):
            E[int(np.dot(j, strides)), k] = 1.0
        Ccols = self.grid_op.matmul(E)
        lag = np.zeros((3,) * d)                       # lag[t + 1] = c(t), t in {-1, 0, 1}^d
        for k, j in enumerate(js):
            for i in np.ndindex(*((2,) * d)):
                t = tuple(int(ia - ja) for ia, ja in zip(i, j))
                v = Ccols[int(np.dot(i, strides)), k]
                lag[tuple(ta + 1 for ta in t)] = v
                lag[tuple(1 - ta for ta in t)] = v   # central symmetry
        _, _, _, frac = _host_plan(self._P, Ns, self._B)
        corners = list(np.ndindex(*((2,) * d)))
        W = [np.prod([frac[a] if c[a] else 1.0 - frac[a] for a in range(d)], axis=0) for c in corners]
        out = np.zeros(self._P.shape[1])
        for ka, a in enumerate(corners):
            for kb, b in enumerate(corners):
                out += W[ka] * W[kb] * lag[tuple(a[x] - b[x] + 1 for x in range(d))]
        return out


def fft_operator_at(ctx, grid_op, points=None, *, box=None, like=None):
    """An FFT covariance operator read at scattered points (`gsi_op_fft_at`): A = W C W', m x m, with C the covariance of
    `grid_op` (from `fft_gridcov_operator` or `fft_powerlaw_operator`, 2 or 3 axes of at least 2 points) and W the
    interpolation matrix of `interpolate` at `points` (ndims x m) on that grid, spanned by the points' extrema or `box`.
    It is exactly the covariance of a field with covariance C read at the points: matrix-free, no rank cap, no sampling
    noise; one product is a spread, a grid product and a gather, and the points plan stays in HBM.  One GPU only.
    The grid operator's `ell` is in grid spacings (see `steps` of the result; steps that differ per axis need per-axis
    `ell`).  A `nugget` on the grid operator is interpolated with everything else: noise at the points is the caller's R.
    Usable wherever an `Operator` is: `randsvd`, `rangefinder`, `eig_nystrom`, `getxis_device`.
    `like`: an `FFTOperatorAt` of the same grid shape instead of `points` and `box` -- the new operator shares its points plan
    and inverted index on the device (`gsi_op_fft_at_like`): nothing is planned or uploaded, and the product is bit-identical
    to that of a freshly planned operator.  The operators may be closed in any order."""
    Ns = getattr(grid_op, "Ns", None)
    h = C.c_void_p()
    if like is not None:
        if points is not None or box is not None:
            raise ValueError("like replaces points and box: pass one or the other")
        L.check(ctx.lib.gsi_op_fft_at_like(ctx.h, C.byref(h), grid_op.h, like.h), ctx.lib)
        return FFTOperatorAt(ctx, h, grid_op, like.Ns, like._P, like._B)
    if points is None:
        raise ValueError("fft_operator_at needs points or like")
    if Ns is None or len(Ns) not in (2, 3):
        # not an FFT grid operator of 2 or 3 axes: the library names the limit
        P = np.asfortranarray(np.asarray(points, dtype=np.float64))
        if P.ndim != 2:
            raise ValueError("points must be ndims x m (one column per point)")
        L.check(ctx.lib.gsi_op_fft_at(ctx.h, C.byref(h), grid_op.h, L.dptr(P), P.shape[1], None), ctx.lib)
        ctx.lib.gsi_op_destroy(h)
        raise ValueError("grid_op is not an FFT covariance operator made by this package")
    P, B = _points_args(points, box, len(Ns))
    L.check(ctx.lib.gsi_op_fft_at(ctx.h, C.byref(h), grid_op.h, L.dptr(P), P.shape[1], _box_ptr(B)), ctx.lib)
    return FFTOperatorAt(ctx, h, grid_op, Ns, P, B)


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
