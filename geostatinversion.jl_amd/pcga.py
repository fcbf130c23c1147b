"""Host-side mirror of the consumers of the xi-basis: `pcgadirect` (src/direct.jl), `pcgalsqr`
(src/lsqr.jl) and `rga` (src/GeostatInversion.jl:101-103).  The forward model is user code and runs
on the host exactly as the reference's `pmap` does; the package's own n-sized algebra (the
perturbation batch and the update s = X*beta + sum xis[i]*dot(eta_i, xi_bar)) and pcgalsqr's
saddle-point LSQR (PCGALowRankMatrix products, IterativeSolvers defaults) run on the GPU.  One class of forward models
can run there too: a `LinearForwardModel` (sparse H, optional weights and exp link) beside a `DeviceBasis` is evaluated on
the device straight from the resident basis, and the perturbation batch is never formed."""
import numpy as np

from . import _lib as L
from .context import default_context, Operator
from .lowrank import PCGALowRankMatrix

SQRT_EPS = float(np.sqrt(np.finfo(np.float64).eps))


class DeviceBasis:
    """The xi-basis resident in HBM: the n x (K+p) matrix Z a device-side randsvd left
    there; `xis[i]` is its column i.  Pass it to `pcgadirect` / `pcgalsqr` / `rga` in place of the
    reference's `xis::Array{Array{Float64,1},1}`: the basis then crosses PCIe never (only the n x (K+3)
    perturbation batch and the updated s do, because the forward model is host code).
    `precision=32` keeps an fp32 copy of the K columns instead (BASELINE configs[4], "fp32 mixed precision": half
    the HBM bytes of every iteration's own algebra; all sums in fp64)."""

    def __init__(self, Zmat, K, precision=64):
        import ctypes as C
        self.Zmat = Zmat
        self.ctx = Zmat.ctx
        self.n = Zmat.shape[0]
        self.K = int(K)
        self.precision = int(precision)
        if not 1 <= self.K <= Zmat.shape[1]:
            raise ValueError("K out of range for this basis")
        h = C.c_void_p()
        L.check(self.ctx.lib.gsi_basis_create(self.ctx.h, C.byref(h), Zmat.h, self.K, self.precision), self.ctx.lib)
        self.h = h
        self.ctx._children.append(self)   # destroyed before the context is
        if self.precision == 32:
            self.Zmat = None            # the fp64 matrix is no longer needed by this basis

    def close(self):
        if getattr(self, "h", None):
            self.ctx.lib.gsi_basis_destroy(self.h)
            self.h = None
            if self in self.ctx._children:
                self.ctx._children.remove(self)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __len__(self):
        return self.K

    def __getitem__(self, i):
        """xis[i] on the host (one column)."""
        if not 0 <= i < self.K:
            raise IndexError(i)
        out = np.empty(self.n)
        L.check(self.ctx.lib.gsi_basis_download_col(self.ctx.h, self.h, i, out.ctypes.data_as(L.c_dp)), self.ctx.lib)
        return out

    def params(self, s, X, delta):
        out = np.empty((self.n, self.K + 3), order="F")
        s = np.ascontiguousarray(s, dtype=np.float64)
        X = np.ascontiguousarray(X, dtype=np.float64)
        L.check(self.ctx.lib.gsi_pcga_params_basis(self.ctx.h, self.h, s.ctypes.data_as(L.c_dp),
                                                   X.ctypes.data_as(L.c_dp), float(delta), L.dptr(out)), self.ctx.lib)
        return out

    def forward(self, fwd, s, X, delta):
        """The nobs x (K+3) results of direct.jl:38-46 / lsqr.jl:36-51 for a `LinearForwardModel`: column c is the model on
        column c of `params(s, X, delta)`, computed on the device from s, X and the resident basis -- the batch is never formed
        and only the results cross the host link (`gsi_pcga_forward_basis`)."""
        if fwd.ctx is not self.ctx:
            raise ValueError("the forward model and the basis live on different contexts")
        out = np.empty((fwd.nobs, self.K + 3), order="F")
        s = np.ascontiguousarray(s, dtype=np.float64)
        X = np.ascontiguousarray(X, dtype=np.float64)
        if s.shape != (self.n,) or X.shape != (self.n,):
            raise ValueError("s and X must have the basis' n entries")
        L.check(self.ctx.lib.gsi_pcga_forward_basis(self.ctx.h, self.h, fwd.h, s.ctypes.data_as(L.c_dp),
                                                    X.ctypes.data_as(L.c_dp), float(delta), L.dptr(out)), self.ctx.lib)
        return out

    def update(self, X, beta_bar, etas, xi_bar):
        E = np.asfortranarray(np.stack(etas, axis=1))
        X = np.ascontiguousarray(X, dtype=np.float64)
        xb = np.ascontiguousarray(xi_bar, dtype=np.float64)
        out = np.empty(self.n)
        L.check(self.ctx.lib.gsi_pcga_update_basis(self.ctx.h, self.h, X.ctypes.data_as(L.c_dp), float(beta_bar),
                                                   L.dptr(E), E.shape[0], xb.ctypes.data_as(L.c_dp),
                                                   out.ctypes.data_as(L.c_dp)), self.ctx.lib)
        return out

    def quadform(self, W, u=None, *, upper=False, return_info=False):
        """`(a, q, t)` over the rows z_i of the basis in one pass on the device (`gsi_basis_quadform`; DESIGN.md section
        4.7d): a[i] = |W' z_i|^2 for the host matrix W (K x ncols), q[i] = |z_i|^2, t[i] = u' z_i (None without `u`).  Z W is
        never formed.  `upper=True` promises W[k, j] = 0 for k > j: those entries are not read.  Both precisions; every sum
        is fp64.  `return_info=True` also returns `[0, path]`, path 1 for the device kernel and 3 for the host path."""
        import ctypes as C
        W = np.asarray(W, dtype=np.float64)
        if W.ndim != 2 or W.shape[0] != self.K or W.shape[1] < 1:
            raise ValueError("W must be K x ncols with ncols >= 1")
        colmajor = W.strides[0] == 8 and (W.shape[1] == 1 or (W.strides[1] % 8 == 0 and W.strides[1] >= 8 * self.K))
        if not colmajor:                                               # the leading K rows of a column-major parent pass as they are
            W = np.asfortranarray(W)
        ldw = W.strides[1] // 8 if W.shape[1] > 1 else self.K
        a, q = np.empty(self.n), np.empty(self.n)
        uv = t = None
        if u is not None:
            uv = np.ascontiguousarray(u, dtype=np.float64)
            if uv.shape != (self.K,):
                raise ValueError("u must have K entries")
            t = np.empty(self.n)
        info = (C.c_int64 * 2)()
        L.check(self.ctx.lib.gsi_basis_quadform(self.ctx.h, self.h, L.dptr(W), ldw, W.shape[1], 1 if upper else 0,
                                                L.dptr(uv) if uv is not None else None, L.dptr(a), L.dptr(q),
                                                L.dptr(t) if t is not None else None, info), self.ctx.lib)
        return (a, q, t, [int(info[0]), int(info[1])]) if return_info else (a, q, t)


class ShardedDeviceBasis(DeviceBasis):
    """A ROW-SHARDED xi-basis (BASELINE configs[4]): this rank's rows of Z as `gsi_randsvd_rows` left them,
    one process per GPU.  `params` / `update` act on this rank's rows of s, X and paramstorun (nothing of size n x K is
    replicated); `gather(rows) -> whole` is the host-side all-gather of row blocks the caller's launcher provides
    (torch.distributed, MPI, Julia's Distributed ...), used only to hand whole parameter vectors to the forward model
    (user code on the host, as the reference's pmap does) and for the convergence norm."""

    def __init__(self, Zmat_rows, K, gather, precision=64):
        super().__init__(Zmat_rows, K, precision=precision)
        self.gather = gather


class _Basis:
    """xis given on the host (the reference's Vector{Vector{Float64}}) as one n x K column-major block."""

    def __init__(self, xis, ctx):
        self.ctx = ctx or default_context()
        self.Z = np.asfortranarray(np.stack([np.asarray(x, dtype=np.float64) for x in xis], axis=1))
        self.n, self.K = self.Z.shape

    def params(self, s, X, delta):
        out = np.empty((self.n, self.K + 3), order="F")
        lib, cx = self.ctx.lib, self.ctx
        s = np.ascontiguousarray(s, dtype=np.float64)
        X = np.ascontiguousarray(X, dtype=np.float64)
        L.check(lib.gsi_pcga_params(cx.h, L.dptr(self.Z), self.n, self.K, s.ctypes.data_as(L.c_dp),
                                    X.ctypes.data_as(L.c_dp), float(delta), L.dptr(out)), lib)
        return out

    def update(self, X, beta_bar, etas, xi_bar):
        E = np.asfortranarray(np.stack(etas, axis=1))
        X = np.ascontiguousarray(X, dtype=np.float64)
        xb = np.ascontiguousarray(xi_bar, dtype=np.float64)
        out = np.empty(self.n)
        lib, cx = self.ctx.lib, self.ctx
        L.check(lib.gsi_pcga_update(cx.h, L.dptr(self.Z), self.n, self.K, X.ctypes.data_as(L.c_dp), float(beta_bar),
                                    L.dptr(E), E.shape[0], xb.ctypes.data_as(L.c_dp), out.ctypes.data_as(L.c_dp)),
                lib)
        return out


class LinearForwardModel:
    """A forward model that lives on the device: h(s)[r] = sum_t H.data[t] g(w[j_t] s[j_t]) over the nonzeros of row r of the
    sparse matrix H (nobs x n), with g the identity (`link="identity"`) or exp (`link="exp"`) and w the optional `weights`.
    Point samples, block averages, ray integrals, the reference's `p .* x` test model (test/testrpcga.jl:110-112), and the
    same on exp(s).  H: anything with `.tocsr()` giving `.indptr`, `.indices`, `.data`, `.shape`, or the tuple
    `(indptr, indices, data, shape)`.

    Passed to `pcgadirect` / `pcgalsqr` / `rga` with a `DeviceBasis` on the same context, the K+3 model runs of an iteration
    are computed on the device from the resident basis (`DeviceBasis.forward`).  It is also an ordinary callable on a host
    vector, `fwd(s)`, so every other path takes it as it takes any forward model."""

    LINKS = {"identity": 0, "exp": 1, 0: 0, 1: 1}
    FORMS = ["none", "lane", "wave", "host"]

    def __init__(self, H, weights=None, link="identity", ctx=None):
        import ctypes as C
        if isinstance(H, tuple):
            indptr, indices, data, shape = H
        else:
            H = H.tocsr()
            indptr, indices, data, shape = H.indptr, H.indices, H.data, H.shape
        if link not in self.LINKS:
            raise ValueError("link must be 'identity' or 'exp'")
        self.ctx = ctx or default_context()
        nobs, n = int(shape[0]), int(shape[1])
        indptr = np.ascontiguousarray(indptr, dtype=np.int64)
        indices = np.ascontiguousarray(indices, dtype=np.int64)
        data = np.ascontiguousarray(data, dtype=np.float64)
        if indptr.shape != (max(nobs, 0) + 1,):
            raise ValueError("indptr must have nobs + 1 entries")
        if indices.shape != data.shape or indices.ndim != 1 or indices.size < int(indptr[-1]):
            raise ValueError("indices and data must be 1-D, of equal length, and hold indptr[-1] entries")
        w = None
        if weights is not None:
            w = np.ascontiguousarray(weights, dtype=np.float64)
            if w.shape != (n,):
                raise ValueError("weights must have n entries")
        p64 = C.POINTER(C.c_int64)
        h = C.c_void_p()
        L.check(self.ctx.lib.gsi_fwd_linear_create(self.ctx.h, C.byref(h), nobs, n, indptr.ctypes.data_as(p64),
                                                   indices.ctypes.data_as(p64), L.dptr(data),
                                                   L.dptr(w) if w is not None else None, self.LINKS[link]), self.ctx.lib)
        self.h = h
        self.nobs, self.n, self.nnz = nobs, n, int(indptr[-1])
        self.link = "exp" if self.LINKS[link] else "identity"
        self.ctx._children.append(self)   # destroyed before the context is

    def close(self):
        if getattr(self, "h", None):
            self.ctx.lib.gsi_fwd_destroy(self.h)
            self.h = None
            if self in self.ctx._children:
                self.ctx._children.remove(self)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def info(self):
        """`gsi_fwd_info`: [nobs, n, nnz, segments, split rows, form of the last product (0 none yet, 1 lane-per-output,
        2 wave-per-segment, 3 host path), products on the host path, products in total]."""
        import ctypes as C
        out = (C.c_int64 * 8)()
        L.check(self.ctx.lib.gsi_fwd_info(self.h, out, 8), self.ctx.lib)
        return [int(v) for v in out]

    def apply(self, P):
        """h of every column of the host matrix P (n x ncols): nobs x ncols."""
        P = L.fmat(P, "P")
        if P.shape[0] != self.n:
            raise ValueError("P must have n rows")
        out = np.empty((self.nobs, P.shape[1]), order="F")
        L.check(self.ctx.lib.gsi_fwd_apply(self.ctx.h, self.h, L.dptr(P), self.n, P.shape[1], L.dptr(out), self.nobs),
                self.ctx.lib)
        return out

    def __call__(self, s):
        return self.apply(np.asarray(s, dtype=np.float64).reshape(-1, 1))[:, 0]

    def _dev(self, fn, X, rows_in, rows_out, what):
        """out = fn(X) for a `DeviceMatrix` (a new `DeviceMatrix`) or a host vector / matrix (a host array of the same kind)."""
        from .context import DeviceMatrix
        ctx, lib = self.ctx, self.ctx.lib
        if isinstance(X, DeviceMatrix):
            out = DeviceMatrix(ctx, rows_out, X.shape[1])
            try:
                L.check(fn(ctx.h, self.h, X.h, out.h), lib)
            except Exception:
                out.close()
                raise
            return out
        Xf = L.fmat(X, what)
        if Xf.shape[0] != rows_in:
            raise ValueError(f"{what} must have {rows_in} rows")
        Xd = DeviceMatrix.from_host(ctx, Xf)
        try:
            out = self._dev(fn, Xd, rows_in, rows_out, what)
            try:
                h = out.to_host()
            finally:
                out.close()
        finally:
            Xd.close()
        return h[:, 0].copy() if np.ndim(X) == 1 else h

    def apply_dev(self, P):
        """h of every column of P (n x b) with P and the result (nobs x b) resident on the device (`gsi_fwd_apply_dev`): a
        `DeviceMatrix` gives a new `DeviceMatrix`; a host vector or matrix is uploaded and the result downloaded."""
        return self._dev(self.ctx.lib.gsi_fwd_apply_dev, P, self.n, self.nobs, "P")

    def adjoint(self, V):
        """H' V for V (nobs x b): n x b (`gsi_fwd_adjoint_dev`), H the matrix of this model with its
        weights folded in.  A `DeviceMatrix` gives a new `DeviceMatrix`, a host vector or matrix a host array.  No atomics: the
        sums follow the inverted index built by the first call, so results are bitwise reproducible.  `link="exp"` has no
        adjoint: `GsiError`."""
        return self._dev(self.ctx.lib.gsi_fwd_adjoint_dev, V, self.nobs, self.n, "V")

    def adjoint_info(self):
        """`gsi_fwd_adjoint_info` as a dict: `built` (the inverted index exists), `resident_bytes`, `long_columns`, `chunks`,
        `longest_list`, `products`, `host_products`."""
        import ctypes as C
        out = (C.c_int64 * 7)()
        L.check(self.ctx.lib.gsi_fwd_adjoint_info(self.h, out, 7), self.ctx.lib)
        keys = ["built", "resident_bytes", "long_columns", "chunks", "longest_list", "products", "host_products"]
        d = {k: int(v) for k, v in zip(keys, out)}
        d["built"] = bool(d["built"])
        return d


class LinearDataOperator(Operator):
    """`linear_data_operator`'s result: the nobs x nobs operator H C H' (`gsi_op_fwd_cov`).  `grid_op` and `model` stay
    referenced."""

    def __init__(self, ctx, h, grid_op, model):
        super().__init__(ctx, h)
        self.grid_op, self.model = grid_op, model


def linear_data_operator(grid_op, model):
    """The covariance of the data of a linear forward model under an FFT grid covariance (`gsi_op_fwd_cov`; DESIGN.md
    section 4.6l): A = H C H', nobs x nobs, with C the covariance of `grid_op` (from `fft_gridcov_operator` or
    `fft_powerlaw_operator`, 2 or 3 axes) and H the matrix of `model`, a `LinearForwardModel` with the identity link over the
    cells of that grid in vec() order -- point samples, block averages, ray integrals.  Matrix-free, no rank cap, no sampling
    noise: one product is `model.adjoint`, the grid product and `model.apply_dev`, O(n log n + nnz) per column, with nothing
    crossing the host link.  One GPU only.  Usable wherever an `Operator` is: `solve`, `lowrank_preconditioner`, `logdet`,
    `log_likelihood`, `randsvd`; `Kriging.linear_inversion` builds the exact linear geostatistical inversion on it."""
    import ctypes as C
    ctx = model.ctx
    h = C.c_void_p()
    L.check(ctx.lib.gsi_op_fwd_cov(ctx.h, C.byref(h), grid_op.h, model.h), ctx.lib)
    return LinearDataOperator(ctx, h, grid_op, model)


class _ReducedForwardModel:
    """S @ fwd(.) for `rga` (GeostatInversion.jl:101-103) with the model kept on the device: S multiplies the small results."""

    def __init__(self, fwd, S):
        self.fwd, self.S = fwd, S

    def __call__(self, x):
        return self.S @ self.fwd(x)


def _device_forward(forwardmodel, basis):
    """(model, S or None) if this iteration head can run on the device, else None."""
    S = None
    if isinstance(forwardmodel, _ReducedForwardModel):
        forwardmodel, S = forwardmodel.fwd, forwardmodel.S
    if not isinstance(forwardmodel, LinearForwardModel) or not isinstance(basis, DeviceBasis):
        return None
    if getattr(basis, "gather", None) is not None or forwardmodel.ctx is not basis.ctx:
        return None
    return forwardmodel, S


def _as_basis(xis, ctx):
    return xis if isinstance(xis, DeviceBasis) else _Basis(xis, ctx)


def _iteration_head(forwardmodel, basis, s, X, delta):
    """direct.jl:38-46 / lsqr.jl:36-51."""
    K = basis.K
    dev = _device_forward(forwardmodel, basis)
    if dev is not None:                                               # a sparse model beside a resident basis: no batch
        R = basis.forward(dev[0], s, X, delta)
        if dev[1] is not None:
            R = dev[1] @ R
        results = [np.ascontiguousarray(R[:, i]) for i in range(K + 3)]
        hs = results[K + 2]
        etas = [(results[i] - hs) / delta for i in range(K)]
        return etas, (results[K] - hs) / delta, (results[K + 1] - hs) / delta, hs
    P = basis.params(s, X, delta)                                     # paramstorun
    if getattr(basis, "gather", None) is not None:                    # row-sharded basis: whole vectors for the forward model
        P = basis.gather(P)
    results = [np.asarray(forwardmodel(np.ascontiguousarray(P[:, i])), dtype=np.float64) for i in range(K + 3)]
    hs = results[K + 2]
    etas = [(results[i] - hs) / delta for i in range(K)]
    HX = (results[K] - hs) / delta
    Hs = (results[K + 1] - hs) / delta
    return etas, HX, Hs, hs


def _global_norm(basis, d):
    """norm(s - olds) (direct.jl:29, lsqr.jl:27); over all ranks' rows when the basis is row-sharded"""
    if getattr(basis, "gather", None) is not None:
        d = basis.gather(d)
    return float(np.linalg.norm(d))


def pcgadirect(forwardmodel, s0, X, xis, R, y, *, maxiters=5, delta=SQRT_EPS, xtol=1e-6,
               callback=lambda s, obs_cal: None, ctx=None, solver="pinv"):
    """`pcgadirect(forwardmodel, s0, X, xis, R, y; maxiters=5, delta=sqrt(eps), xtol=1e-6, callback)`
    (direct.jl:21-67).

    `solver="pinv"` (the default) solves the saddle-point system of direct.jl:56-58 as the reference does, with a
    pseudo-inverse of the dense (nobs+1)^2 matrix on the host.  `solver="cholesky"` solves it on the device by a Cholesky
    factorization of HQH + R (`PCGALowRankMatrix.solve`), which needs HQH + R positive definite --
    true whenever R is.  An iteration whose factorization fails (status 7) or whose system is singular (status 3) is solved
    with the pseudo-inverse instead; `pcgadirect.last_fallbacks` counts those iterations of the last call.  Through `rga`:
    `rga(..., pcgafunc=functools.partial(pcgadirect, solver="cholesky"))`."""
    if solver not in ("pinv", "cholesky"):
        raise ValueError("solver must be 'pinv' or 'cholesky'")
    basis = _as_basis(xis, ctx)
    s = np.asarray(s0, dtype=np.float64)
    X = np.asarray(X, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    Rd = R.toarray() if hasattr(R, "toarray") else np.asarray(R, dtype=np.float64)
    converged, it = False, 0
    pcgadirect.last_fallbacks = 0
    while not converged and it < maxiters:
        olds = s
        etas, HX, Hs, hs = _iteration_head(forwardmodel, basis, s, X, delta)
        callback(s, hs)                                               # :47
        b = np.concatenate([y - hs + Hs, np.zeros(1)])                # :56
        x = None
        if solver == "cholesky":
            bigA = PCGALowRankMatrix(etas, HX, R, ctx=basis.ctx)
            try:
                x = bigA.solve(b)
            except L.GsiError as e:
                if e.code not in (3, 7):
                    raise
                pcgadirect.last_fallbacks += 1
            finally:
                bigA.close()
        if x is None:
            E = np.stack(etas, axis=1)
            HQH = E @ E.T                                             # :49-53
            bigA = np.block([[HQH + Rd, HX[:, None]], [HX[None, :], np.zeros((1, 1))]])   # :57
            x = np.linalg.pinv(bigA) @ b                              # :58
        s = basis.update(X, x[-1], etas, x[:-1])                      # :59-65
        if _global_norm(basis, s - olds) < xtol:
            converged = True
        it += 1
    return s


def pcgalsqr(forwardmodel, s0, X, xis, R, y, *, maxiters=5, delta=SQRT_EPS, xtol=1e-6, ctx=None):
    """`pcgalsqr(forwardmodel, s0, X, xis, R, y; maxiters=5, delta=sqrt(eps), xtol=1e-6)`
    (lsqr.jl:20-63).  No `callback` keyword, as in the reference."""
    basis = _as_basis(xis, ctx)
    s = np.asarray(s0, dtype=np.float64)
    X = np.asarray(X, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    converged, it = False, 0
    while not converged and it < maxiters:
        olds = s
        etas, HX, Hs, hs = _iteration_head(forwardmodel, basis, s, X, delta)
        b = np.concatenate([y - hs + Hs, np.zeros(1)])                # :52
        bigA = PCGALowRankMatrix(etas, HX, R, ctx=basis.ctx)          # :53
        x = bigA.lsqr(b)                                              # :54  (LSQR on the device)
        bigA.close()
        s = basis.update(X, x[-1], etas, x[:-1])                      # :55-61
        if _global_norm(basis, s - olds) < xtol:
            converged = True
        it += 1
    return s


def rga(forwardmodel, s0, X, xis, R, y, S, *, maxiters=5, delta=SQRT_EPS, xtol=1e-6, pcgafunc=pcgadirect,
        callback=lambda s, obs_cal: None):
    """`rga(...; pcgafunc=pcgadirect, callback)`  (GeostatInversion.jl:101-103)."""
    S = np.asarray(S, dtype=np.float64)
    Rd = R.toarray() if hasattr(R, "toarray") else np.asarray(R, dtype=np.float64)
    reduced = _ReducedForwardModel(forwardmodel, S) if isinstance(forwardmodel, LinearForwardModel) \
        else (lambda x: S @ forwardmodel(x))
    return pcgafunc(reduced, s0, X, xis, S @ Rd @ S.T, S @ np.asarray(y, dtype=np.float64),
                    maxiters=maxiters, delta=delta, xtol=xtol, callback=callback)


def _posterior_matrix(forwardmodel, basis, s, X, R, delta):
    """The PCGALowRankMatrix of the linearisation at s (direct.jl:38-46): E = H Z, HX and R on the basis' context."""
    etas, HX, _, _ = _iteration_head(forwardmodel, basis, np.asarray(s, dtype=np.float64), X, delta)
    return PCGALowRankMatrix(etas, HX, R, ctx=basis.ctx)


def posterior_variance(forwardmodel, s, X, xis, R, *, delta=SQRT_EPS, prior_variance=None, ctx=None, return_info=False):
    """The posterior variance of the field at the linearisation point `s` (usually the estimate `pcgadirect` returned), for
    the prior s ~ N(X beta, Q), Q ~ Z Z' with Z the xis and beta unknown, and the error covariance R:

        v_i = |W' z_i|^2 + (u' z_i - X_i)^2 / gamma                     (prior variance taken as |z_i|^2, the low-rank one)
        v_i = prior_i - |z_i|^2 + |W' z_i|^2 + (u' z_i - X_i)^2 / gamma  (`prior_variance` = the true prior variances)

    with (W, u, gamma) = `PCGALowRankMatrix.posterior_factor()`.  The n-sized work is one pass over the resident basis on the
    device (`gsi_pcga_posterior_variance`); a host `xis` list is uploaded into a temporary `DeviceBasis`.  A
    `LinearForwardModel` beside a `DeviceBasis` is linearised on the device.  R must be positive definite (`GsiError` code 7
    otherwise) and HX non-zero (code 3).  `return_info=True` also returns `[column, path]`, path 1 for the device kernel and 3
    for the host path.  Row-sharded bases are not supported."""
    import ctypes as C
    if isinstance(xis, DeviceBasis) and getattr(xis, "gather", None) is not None:
        raise NotImplementedError("posterior_variance: a row-sharded basis is not supported")
    X = np.ascontiguousarray(X, dtype=np.float64)
    temp = None
    if isinstance(xis, DeviceBasis):
        basis = xis
    else:
        from .context import DeviceMatrix
        cx = ctx or default_context()
        Zm = DeviceMatrix.from_host(cx, np.stack([np.asarray(x, dtype=np.float64) for x in xis], axis=1))
        basis = DeviceBasis(Zm, Zm.shape[1])
        temp = (basis, Zm)
    bigA = None
    try:
        if X.shape != (basis.n,):
            raise ValueError("X must have the basis' n entries")
        prior = None
        if prior_variance is not None:
            prior = np.ascontiguousarray(prior_variance, dtype=np.float64)
            if prior.shape != (basis.n,):
                raise ValueError("prior_variance must have the basis' n entries")
        bigA = _posterior_matrix(forwardmodel, basis, s, X, R, delta)
        var = np.empty(basis.n)
        info = (C.c_int64 * 2)()
        lib = basis.ctx.lib
        L.check(lib.gsi_pcga_posterior_variance(basis.ctx.h, basis.h, bigA.h, L.dptr(X),
                                                L.dptr(prior) if prior is not None else None, L.dptr(var), info), lib)
    finally:
        if bigA is not None:
            bigA.close()
        if temp is not None:
            temp[0].close()
            temp[1].close()
    return (var, [int(info[0]), int(info[1])]) if return_info else var


def posterior_realizations(forwardmodel, s_hat, X, xis, R, num, *, delta=SQRT_EPS, seed=None, omega=None, ctx=None):
    """`num` conditional realisations around the estimate `s_hat`, as the columns of an n x num array:

        s_c = s_hat + Z (W omega_1 + u omega_2 / sqrt(gamma)) - X omega_2 / sqrt(gamma),   omega_1 ~ N(0, I_K), omega_2 ~ N(0, 1)

    whose covariance is the posterior covariance Z W W' Z' + d d' / gamma.  `omega` ((K + 1) x num: omega_1 over omega_2)
    defaults to `RandMatFact.randn(K + 1, num)` (after `RandMatFact.seed(seed)` when `seed` is given); with `omega` given the
    result is deterministic.  Each column is one pass over the basis (`DeviceBasis.update`)."""
    from . import randmatfact
    basis = _as_basis(xis, ctx)
    if getattr(basis, "gather", None) is not None:
        raise NotImplementedError("posterior_realizations: a row-sharded basis is not supported")
    X = np.ascontiguousarray(X, dtype=np.float64)
    s_hat = np.asarray(s_hat, dtype=np.float64)
    K = basis.K
    num = int(num)
    if omega is None:
        if seed is not None:
            randmatfact.seed(seed)
        omega = randmatfact.randn(K + 1, num)
    omega = np.asarray(omega, dtype=np.float64)
    if omega.shape != (K + 1, num):
        raise ValueError("omega must be (K + 1) x num")
    bigA = _posterior_matrix(forwardmodel, basis, s_hat, X, R, delta)
    try:
        W, u, gamma = bigA.posterior_factor()
    finally:
        bigA.close()
    eye = [np.ascontiguousarray(c) for c in np.eye(K)]
    out = np.empty((basis.n, num), order="F")
    for c in range(num):
        w2 = omega[K, c] / np.sqrt(gamma)
        out[:, c] = s_hat + basis.update(X, -w2, eye, W @ omega[:K, c] + u * w2)
    return out


pcgadirect.last_fallbacks = 0
pcga = pcgadirect     # GeostatInversion.jl:105
