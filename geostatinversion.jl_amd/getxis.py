"""Host-side mirror of `getxis` / `randsvdwithseed`  (src/GeostatInversion.jl:20-70)."""
import numpy as np

from . import randmatfact as RMF
from .lowrank import LowRankCovMatrix


def randsvdwithseed(Q, numxis, p, q, seed=None, *, Omega=None):
    """`randsvdwithseed(Q, numxis, p, q, seed::Nothing|Int)`  (GeostatInversion.jl:20-27)."""
    if seed is not None:
        if not isinstance(seed, (int, np.integer)):
            raise TypeError("seed must be an Int or None")      # the reference has no other method
        RMF.seed(int(seed))                                      # Random.seed!(seed)   :25
    return RMF.randsvd(Q, numxis, p, q, Omega=Omega)


def getxis_iwantfields(samplefield, numfields, numxis, p, q=3, seed=None, *, Omega=None, ctx=None):
    """`getxis(Val{:iwantfields}, samplefield, numfields, numxis, p, q=3, seed)`  (:29-38) -> (xis, fields)."""
    fields = [np.asarray(samplefield(), dtype=np.float64) for _ in range(numfields)]   # rpmap   :30
    lrcm = LowRankCovMatrix(fields, ctx=ctx)                     # :31
    try:
        Z = randsvdwithseed(lrcm, numxis, p, q, seed, Omega=Omega)   # :32
    finally:
        lrcm.close()
    xis = [np.ascontiguousarray(Z[:, i]) for i in range(numxis)]     # :33-36
    return xis, fields


def getxis(first, *args, **kwargs):
    """Both reference methods (GeostatInversion.jl:58-70):

    `getxis(samplefield::Function, numfields, numxis, p, q=3, seed=nothing)`
    `getxis(Q::Matrix, numxis, p, q=3, seed=nothing)`
    """
    if callable(first):
        xis, _ = getxis_iwantfields(first, *args, **kwargs)      # :58-61
        return xis
    return _getxis_matrix(first, *args, **kwargs)


def _getxis_matrix(Q, numxis, p, q=3, seed=None, *, Omega=None):
    Z = randsvdwithseed(Q, numxis, p, q, seed, Omega=Omega)     # :65
    return [np.ascontiguousarray(Z[:, i]) for i in range(numxis)]   # :66-68


def getxis_device(Q, numxis, p, q=3, seed=None, *, Omega=None, ctx=None, precision=64):
    """`getxis` whose result stays in HBM: returns a `DeviceBasis` usable wherever the
    reference takes `xis` (`pcgadirect`, `pcgalsqr`, `rga`).  Q: a matrix, a `LowRankCovMatrix` or a device
    `Operator`.  `precision=32`: the basis is kept in fp32 (mixed precision, BASELINE configs[4])."""
    import ctypes as C
    from . import _lib as L
    from .context import DeviceMatrix, Operator, dense_operator, default_context
    from .pcga import DeviceBasis
    if seed is not None:
        RMF.seed(int(seed))
    owned = False
    if isinstance(Q, Operator):
        op = Q
    elif hasattr(Q, "_device_operator"):
        op = Q._device_operator(ctx)
    else:
        op, owned = dense_operator(ctx or default_context(), Q), True
    try:
        cx = op.ctx
        m, n = op.shape
        l = int(numxis) + int(p)
        Om = RMF.randn(n, l) if Omega is None else Omega
        Omd = DeviceMatrix.from_host(cx, Om)
        Z = DeviceMatrix(cx, n, l)
        L.check(cx.lib.gsi_randsvd_dev(cx.h, op.h, Omd.h, int(numxis), int(p), int(q), Z.h, None), cx.lib)
        Omd.close()
        return DeviceBasis(Z, numxis, precision=precision)
    finally:
        if owned:
            op.close()


def getxis_pivchol(Q, numxis, tol=0.0, *, principal=True, precision=64, ctx=None):
    """A xi-basis from the diagonal-pivoted Cholesky factor of Q (`RandMatFact.pivoted_cholesky`; no operator product): a
    `DeviceBasis`, as `getxis_device` returns, of the columns that were reached -- `numxis`, or fewer by `tol` or where Q is
    exhausted.  Q: a host matrix, or a dense / implicit grid-covariance / implicit point-covariance `Operator`.
    `principal=True` turns the factor into its principal form (`RandMatFact.principal_factor`: orthogonal columns in
    descending order of norm, as `randsvd` returns them); with `False` the columns are those of L, in pivot order.  The PCGA
    consumers only use sum xi xi' = L L', which both forms share."""
    from .context import Operator, dense_operator, default_context
    from .pcga import DeviceBasis
    owned = not isinstance(Q, Operator)
    op = dense_operator(ctx or default_context(), Q) if owned else Q
    try:
        Ld, piv, _ = RMF._pivoted_cholesky_dev(op, numxis, tol)
    finally:
        if owned:
            op.close()
    K = len(piv)
    if K == 0:
        Ld.close()
        raise ValueError("pivoted_cholesky found rank 0: Q has no positive diagonal entry")
    if principal:
        try:
            Z, _ = RMF.principal_factor(Ld, K)
        finally:
            Ld.close()
    else:
        Z = Ld
    return DeviceBasis(Z, K, precision=precision)


def getxis_fftrf(Ns, k0, dk, beta, numfields, numxis, p, q=3, seed=None, *, field_seed=0, Omega=None, ctx=None, device=False,
                 points=None, box=None):
    """`getxis(() -> FFTRF.powerlaw_structuredgrid(Ns, k0, dk, beta), numfields, numxis, p, q, seed)` with the fields sampled
    on the device and never leaving HBM (`gsi_op_lowrank_fftrf`; field f draws the device stream `field_seed + f`).  `seed`
    governs Omega exactly as in `getxis`.  Returns the list of xi-vectors, or with `device=True` a `DeviceBasis`.  With
    `points` (ndims x m; `box` optional) the sample function is `() -> FFTRF.powerlaw_unstructuredgrid(points, Ns, k0, dk,
    beta)` and the xi-vectors have m entries (`gsi_op_lowrank_fftrf_at`)."""
    from .context import default_context
    from .fftrf import lowrank_fftrf_operator, _points_args
    if points is not None or box is not None:
        if points is None:
            raise ValueError("box applies to points: pass points as well")
        _points_args(points, box, len(list(Ns)))
    op = lowrank_fftrf_operator(ctx or default_context(), Ns, k0, dk, beta, numfields, seed=field_seed, points=points, box=box)
    try:
        if device:
            return getxis_device(op, numxis, p, q, seed, Omega=Omega)
        Z = randsvdwithseed(op, numxis, p, q, seed, Omega=Omega)
        return [np.ascontiguousarray(Z[:, i]) for i in range(numxis)]
    finally:
        op.close()
