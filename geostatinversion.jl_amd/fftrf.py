"""Host-side mirror of `FFTRF.powerlaw_structuredgrid` (FFTRF.jl:83-100) with the fields sampled on the device
(`gsi_fftrf_fields`, csrc/fftrf_sample.hip).  The reference's own function stays what it is, and a caller's own
`samplefield` closure keeps working with `getxis`; this is the path for grids whose fields should never leave HBM."""
import ctypes as C

import numpy as np

from . import _lib as L
from . import randmatfact as RMF
from .context import DeviceMatrix, Operator, default_context


def _grid(Ns):
    Ns = [int(v) for v in Ns]
    return Ns, (C.c_int64 * len(Ns))(*Ns)


def phi_shape(Ns):
    """`size(S)` of `mulbyphi` (FFTRF.jl:75): (2 N_2, 2 N_1[, 2 N_3]) -- the reference's axis swap."""
    Ns = [int(v) for v in Ns]
    return tuple(2 * N for N in ([Ns[1], Ns[0]] + Ns[2:] if len(Ns) >= 2 else Ns))


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
            shp = phi_shape(Ns)
            if len(phi) != int(numfields):
                raise ValueError("phi must hold one array per field")
            ph = np.empty((int(np.prod(shp)), int(numfields)), order="F")
            for c in range(int(numfields)):
                pc = np.asarray(phi[c], dtype=np.float64)
                if pc.shape != shp:
                    raise ValueError(f"phi[{c}] must have the reference's size(S) = {shp}")
                ph[:, c] = pc.reshape(-1, order="F")          # vec()
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


def lowrank_fftrf_operator(ctx, Ns, k0, dk, beta, numfields, seed=0):
    """`LowRankCovMatrix` over `numfields` device-sampled FFTRF fields (`gsi_op_lowrank_fftrf`): generated, centred and
    kept in HBM.  Row-sharded like every operator: each rank generates every field and keeps its own rows."""
    Ns, arr = _grid(Ns)
    row0, nloc = ctx.shard(int(np.prod(Ns)))
    h = C.c_void_p()
    L.check(ctx.lib.gsi_op_lowrank_fftrf(ctx.h, C.byref(h), len(Ns), arr, float(k0), float(dk), float(beta), int(numfields),
                                         int(seed) % (1 << 64), row0, nloc), ctx.lib)
    return Operator(ctx, h)
