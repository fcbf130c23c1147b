"""Gaussian fields with a covariance FUNCTION on a regular grid, sampled on the device by circulant embedding
(`gsi_gridcov_sampler_*`, `gsi_gridcov_fields`, csrc/gridcov_sample.hip): the sampler that belongs to
`fft_gridcov_operator` as `FFTRF.powerlaw_fields` belongs to `fft_powerlaw_operator`.  The fields have the operator's matrix
as their covariance -- exactly where the torus covariance is non-negative definite, and to `neg_mass * (sigma2 + nugget)`
where its negative eigenvalues were clamped.

Fields at the points of a mesh need no entry of their own: `FFTRF.interpolate(ctx, points, sampler.fields(...), Ns)` takes
the device matrix as it is."""
import ctypes as C

import numpy as np

from . import _lib as L
from .context import POINTCOV_KINDS, DeviceMatrix, Operator, _Handle, default_context


class GridCovSampler(_Handle):
    """The plan of one grid and covariance function (`gsi_sampler`): `.M` the torus, `.neg_mass`, `.lam_min`, `.lam_max`,
    `.clamped` what creation found of the spectrum."""
    _destroy = "gsi_gridcov_sampler_destroy"

    def __init__(self, ctx, h, Ns):
        super().__init__(ctx, h)
        self.Ns = tuple(int(v) for v in Ns)
        M = (C.c_int64 * 3)()
        info = (C.c_double * 4)()
        L.check(ctx.lib.gsi_gridcov_sampler_info(h, M, info), ctx.lib)
        self.M = tuple(int(M[a]) for a in range(len(self.Ns)))
        self.neg_mass, self.lam_min, self.lam_max = float(info[0]), float(info[1]), float(info[2])
        self.clamped = int(info[3])

    @property
    def Mtot(self):
        return int(np.prod(self.M))

    def spectrum(self):
        """lambda on the torus (shape `M`, unclamped, nugget included)."""
        lam = np.empty(self.Mtot)
        L.check(self.ctx.lib.gsi_gridcov_sampler_spectrum(self.ctx.h, self.h, L.dptr(lam)), self.ctx.lib)
        return lam.reshape(self.M, order="F")

    def fields(self, numfields, seed=0, field0=0, eps=None):
        """`numfields` fields as a `DeviceMatrix` of n x numfields, column c = vec() of field `field0 + c` (`field0` even:
        fields 2 j and 2 j + 1 are the real and imaginary part of one transform).  `eps`: an Mtot x 2 ceil(numfields / 2)
        array, column c the N(0,1) noise of role c in torus order (even columns the real, odd the imaginary part of the
        pair's noise); without it role f draws the stream `DeviceMatrix(ctx, Mtot, 1).randn(seed + f)`."""
        numfields = int(numfields)
        F = DeviceMatrix(self.ctx, int(np.prod(self.Ns)), numfields)
        try:
            if eps is None:
                L.check(self.ctx.lib.gsi_gridcov_fields(self.ctx.h, self.h, F.h, None, 0, int(seed) % (1 << 64), int(field0)),
                        self.ctx.lib)
            else:
                e = L.fmat(eps, "eps")
                if e.shape != (self.Mtot, 2 * ((numfields + 1) // 2)):
                    raise ValueError(f"eps must be Mtot x 2 ceil(numfields / 2) = {self.Mtot} x {2 * ((numfields + 1) // 2)}")
                L.check(self.ctx.lib.gsi_gridcov_fields(self.ctx.h, self.h, F.h, L.dptr(e), e.shape[0], 0, 0), self.ctx.lib)
        except Exception:
            F.close()
            raise
        return F


def _create(ctx, Ns, k, ells, theta, sigma2, nugget, embed, neg_tol):
    arr = (C.c_int64 * len(Ns))(*Ns)
    earr = (C.c_double * len(ells))(*ells)
    marr = (C.c_int64 * len(Ns))(*[int(v) for v in embed]) if embed is not None else None
    h = C.c_void_p()
    L.check(ctx.lib.gsi_gridcov_sampler_create(ctx.h, C.byref(h), len(Ns), arr, marr, k, earr, float(theta), float(sigma2),
                                               float(nugget), float(neg_tol), None), ctx.lib)
    return GridCovSampler(ctx, h, Ns)


def default_embedding(Ns):
    """The operator's torus: per axis the next power of two >= 2 N."""
    return tuple(max(2, 1 << int(2 * int(N) - 1).bit_length()) for N in Ns)


def gridcov_sampler(ctx, Ns, kind="exponential", ell=1.0, theta=0.0, sigma2=1.0, nugget=0.0, embed=None, neg_tol=1e-12):
    """The sampler of the covariance of `fft_gridcov_operator(ctx, Ns, kind, ell, theta, sigma2, nugget)` (2-D or 3-D).
    `embed`: the torus, per axis a power of two with 2 N <= M <= 8192 (None: the next power of two >= 2 N, the operator's
    own); "auto": start there and, while the covariance is refused as not non-negative definite on the torus (code 7),
    double every axis still below 8192, until Mtot would reach 2^31 or no axis can grow -- the last refusal is raised then.
    `neg_tol`: the largest accepted `neg_mass` (the covariance error of the clamped spectrum, relative to sigma2 + nugget)."""
    Ns = [int(v) for v in Ns]
    k = POINTCOV_KINDS[kind] if isinstance(kind, str) else int(kind)
    ells = [float(ell)] * len(Ns) if np.ndim(ell) == 0 else [float(v) for v in ell]
    if len(ells) != len(Ns):
        raise ValueError("ell must be one length or one per axis")
    if not (isinstance(embed, str) and embed == "auto"):
        if embed is not None and len(embed) != len(Ns):
            raise ValueError("embed must be None, \"auto\" or one torus length per axis")
        return _create(ctx, Ns, k, ells, theta, sigma2, nugget, embed, neg_tol)
    M = list(default_embedding(Ns))
    while True:
        try:
            return _create(ctx, Ns, k, ells, theta, sigma2, nugget, M, neg_tol)
        except L.GsiError as e:
            if e.code != 7:
                raise
            grown = [m * 2 if m < 8192 else m for m in M]
            if grown == M or int(np.prod(grown)) >= (1 << 31):
                raise
            M = grown


def lowrank_gridcov_operator(ctx, sampler, numfields, seed=0):
    """`LowRankCovMatrix` over `numfields` device-sampled fields of `sampler` (`gsi_op_lowrank_gridcov`): generated, centred
    and kept in HBM.  Row-sharded like every operator: each rank generates every field and keeps its own rows."""
    h = C.c_void_p()
    row0, nloc = ctx.shard(int(np.prod(sampler.Ns)))
    L.check(ctx.lib.gsi_op_lowrank_gridcov(ctx.h, C.byref(h), sampler.h, int(numfields), int(seed) % (1 << 64), row0, nloc),
            ctx.lib)
    return Operator(ctx, h)


def gridcov_structuredgrid(Ns, kind="exponential", ell=1.0, theta=0.0, sigma2=1.0, nugget=0.0, embed=None, neg_tol=1e-12,
                           seed=None, ctx=None):
    """One field of that covariance as an ndarray of shape `Ns`.  `seed`: the device stream of
    `gridcov_sampler(...).fields(1, seed=seed)`; None: the noise is drawn from `RandMatFact.randn`, the package's host
    stream."""
    from . import randmatfact as RMF
    ctx = ctx or default_context()
    s = gridcov_sampler(ctx, Ns, kind, ell, theta, sigma2, nugget, embed, neg_tol)
    try:
        F = s.fields(1, seed=seed) if seed is not None else s.fields(1, eps=RMF.randn(s.Mtot, 2))
        try:
            return F.to_host()[:, 0].reshape(s.Ns, order="F")
        finally:
            F.close()
    finally:
        s.close()
