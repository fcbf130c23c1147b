# GeostatInversionHIP.jl -- Julia-side drop-in for the RandMatFact hot path of GeostatInversion.jl,
# calling libgsi_hip.so (hand-written gfx950 HIP kernels) through `ccall`.  It keeps the reference
# signatures (file:line of the reference in comments) so existing PCGA / RGA call sites work
# unchanged:
#
#     import GeostatInversionHIP as GH
#     xis = GH.getxis(Q, numxis, p, q, seed)                  # GeostatInversion.jl:63
#     xis = GH.getxis(samplefield, numfields, numxis, p, q, seed)   # GeostatInversion.jl:58
#     popt = GeostatInversion.pcgadirect(forward, s0, X, xis, R, y) # xis is Vector{Vector{Float64}}
#
# The Gaussian test matrix is drawn HERE with Julia's own `randn`, exactly where the reference
# draws it (RandMatFact.jl:54 after Random.seed! at GeostatInversion.jl:25), so for a given seed the
# GPU path sees the same Omega as the reference.
#
# NOTE: there is no Julia in the build image; this file is the binding a maintainer would add and is
# exercised only where Julia is available.  The same ABI is exercised by the Python ctypes mirror
# (geostatinversion.jl_amd/) in the test-suite.
module GeostatInversionHIP

import Random
import Libdl
import LinearAlgebra
import Distributed
import SparseArrays

const libgsi = get(ENV, "GSI_HIP_LIB", joinpath(@__DIR__, "..", "geostatinversion.jl_amd", "libgsi_hip.so"))

struct GsiError <: Exception
	code::Int
	msg::String
end
Base.showerror(io::IO, e::GsiError) = print(io, "GsiError($(e.code)): $(e.msg)")

function check(status::Cint)
	if status != 0
		msg = unsafe_string(ccall((:gsi_last_error, libgsi), Cstring, ()))
		# the reference raises ErrorException via error(...) (RandMatFact.jl:63, lowrank.jl:58)
		status == 2 && error(msg)
		# lu(Y) on an exactly zero pivot (RandMatFact.jl:60) and cholesky(Hermitian(B2)) of eig_nystrom (:95) throw these in the reference
		status == 3 && throw(LinearAlgebra.SingularException(0))
		status == 7 && throw(LinearAlgebra.PosDefException(0))
		throw(GsiError(Int(status), msg))
	end
	return nothing
end

# ---- context: one per GPU -------------------------------------------------------------------------
mutable struct Context
	h::Ptr{Cvoid}
	function Context(device::Integer=0)
		r = Ref{Ptr{Cvoid}}(C_NULL)
		check(ccall((:gsi_ctx_create, libgsi), Cint, (Ref{Ptr{Cvoid}}, Cint), r, device))
		c = new(r[])
		finalizer(c) do x
			x.h != C_NULL && ccall((:gsi_ctx_destroy, libgsi), Cint, (Ptr{Cvoid},), x.h)
			x.h = C_NULL
		end
		return c
	end
end
"Return the context's cached device memory (released panels, idle workspaces) to the driver."
release_cache!(c::Context) = check(ccall((:gsi_ctx_release_cache, libgsi), Cint, (Ptr{Cvoid},), c.h))
const default_ctx = Ref{Union{Nothing, Context}}(nothing)
"The process-wide default context (GPU 0), created at its first use.  (`something(a, b)` would evaluate `b` -- a new
context -- at every call: the arguments of a function are evaluated before it runs.)"
function ctx()
	default_ctx[] === nothing && (default_ctx[] = Context(0))
	return default_ctx[]::Context
end

"Join `nranks` contexts (one Julia process per GPU) into an RCCL communicator; rank 0 creates the id."
function unique_id()
	id = zeros(UInt8, 128)
	check(ccall((:gsi_comm_unique_id, libgsi), Cint, (Ptr{UInt8},), id))
	return id
end
comm_init!(c::Context, nranks::Integer, rank::Integer, id::Vector{UInt8}) =
	check(ccall((:gsi_ctx_comm_init, libgsi), Cint, (Ptr{Cvoid}, Cint, Cint, Ptr{UInt8}), c.h, nranks, rank, id))

"Every rank's `values` on every rank (`gsi_ctx_host_allgather`): a `nranks x length(values)` matrix, row r = rank r - 1.  Also
the job's barrier (it waits for the context's stream first): what a Distributed.jl host needs around the hot path."
function host_allgather(c::Context, values::Vector{Float64}, nranks::Integer)
	out = Matrix{Float64}(undef, length(values), nranks)
	check(ccall((:gsi_ctx_host_allgather, libgsi), Cint, (Ptr{Cvoid}, Ptr{Float64}, Int64, Ptr{Float64}), c.h, values, length(values), out))
	return Matrix(out')
end

const LU_FORMS = ["none", "replicated", "per-step", "persistent-1hop", "persistent-2hop", "persistent-ov"]
"Which path ran under the communicator (`gsi_ctx_path_info`): LU form, self-test mask of the in-kernel pivot exchange,
collectives since the last phase reset, ranks joined, LU time-outs seen / hidden by a transparent re-run."
function path_info(c::Context)
	out = zeros(Int64, 13)
	check(ccall((:gsi_ctx_path_info, libgsi), Cint, (Ptr{Cvoid}, Ptr{Int64}, Int64), c.h, out, length(out)))
	return (lu_form = LU_FORMS[out[1] + 1], lu_selftest_mask = out[2], collectives = out[3], n_ranks_seen = out[4],
		lu_timeouts = out[5], lu_timeouts_recovered = out[6], svd_sweep_cap_hits = out[13], lu_forms_run = Dict(LU_FORMS[f + 1] => out[7 + f] for f = 1:5 if out[7 + f] > 0))
end

# ---- operators ------------------------------------------------------------------------------------
mutable struct DeviceOperator
	h::Ptr{Cvoid}
	c::Context
	m::Int
	n::Int
end
function finalize_op!(op::DeviceOperator)
	op.h != C_NULL && ccall((:gsi_op_destroy, libgsi), Cint, (Ptr{Cvoid},), op.h)
	op.h = C_NULL
end

"Upload a dense `Matrix{Float64}` (this rank's block of rows when a communicator is attached)."
function DeviceOperator(A::Matrix{Float64}; c::Context=ctx(), row0::Int=0, mlocal::Int=size(A, 1))
	r = Ref{Ptr{Cvoid}}(C_NULL)
	m, n = size(A)
	GC.@preserve A check(ccall((:gsi_op_dense, libgsi), Cint,
		(Ptr{Cvoid}, Ref{Ptr{Cvoid}}, Ptr{Float64}, Int64, Int64, Int64, Int64, Int64),
		c.h, r, pointer(A, row0 + 1), m, n, stride(A, 2), row0, mlocal))
	op = DeviceOperator(r[], c, m, n)
	finalizer(finalize_op!, op)
	return op
end

"`LowRankCovMatrix(samples)` (lowrank.jl:14-30): samples uploaded as an n x N matrix, centred on the device."
function LowRankCovMatrix(samples::Array{Array{Float64, 1}, 1}; c::Context=ctx())
	n, N = length(samples[1]), length(samples)
	S = Matrix{Float64}(undef, n, N)
	for i = 1:N
		S[:, i] = samples[i]
	end
	r = Ref{Ptr{Cvoid}}(C_NULL)
	check(ccall((:gsi_op_lowrank, libgsi), Cint,
		(Ptr{Cvoid}, Ref{Ptr{Cvoid}}, Ptr{Float64}, Int64, Int64, Int64, Cint, Int64, Int64),
		c.h, r, S, n, N, n, 1, 0, n))
	op = DeviceOperator(r[], c, n, n)
	finalizer(finalize_op!, op)
	return op
end

"`A.samples` of a device LowRankCovMatrix (lowrank.jl:14-16; mean-removed, lowrank.jl:25-27) back on the host as the
reference keeps them: a Vector of N sample vectors (`gsi_op_lowrank_samples`)."
function samples(A::DeviceOperator, N::Int)
	S = Matrix{Float64}(undef, A.m, N)
	check(ccall((:gsi_op_lowrank_samples, libgsi), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}, Int64),
		A.c.h, A.h, S, A.m))
	return [S[:, i] for i = 1:N]
end

"`numfields` fields of `FFTRF.powerlaw_structuredgrid(Ns, k0, dk, beta)` (FFTRF.jl:83-100) sampled on the device
(`gsi_fftrf_fields`): an n x numfields `DeviceMatrix`, column c = `vec` of field `field0 + c`.  `phi` (Mtot x numfields,
column c = `vec(randn(size(S)))` of `mulbyphi`, FFTRF.jl:75, for field c) reproduces the reference's field for the same
random numbers; without it field f draws the device stream `seed + f`."
function fftrf_fields(Ns::Vector{Int}, k0::Float64, dk::Float64, beta::Float64, numfields::Int;
		phi::Union{Nothing,Matrix{Float64}}=nothing, seed::Integer=0, field0::Int=0, c::Context=ctx())
	N64 = Int64.(Ns)
	F = DeviceMatrix(prod(Ns), numfields; c=c)
	if phi === nothing
		check(ccall((:gsi_fftrf_fields, libgsi), Cint,
			(Ptr{Cvoid}, Ptr{Cvoid}, Cint, Ptr{Int64}, Cdouble, Cdouble, Cdouble, Ptr{Float64}, Int64, UInt64, Int64),
			c.h, F.h, length(N64), N64, k0, dk, beta, C_NULL, 0, UInt64(seed), field0))
	else
		size(phi, 2) == numfields || error("phi must have one column per field")
		GC.@preserve phi check(ccall((:gsi_fftrf_fields, libgsi), Cint,
			(Ptr{Cvoid}, Ptr{Cvoid}, Cint, Ptr{Int64}, Cdouble, Cdouble, Cdouble, Ptr{Float64}, Int64, UInt64, Int64),
			c.h, F.h, length(N64), N64, k0, dk, beta, phi, stride(phi, 2), UInt64(0), 0))
	end
	return F
end

"`LowRankCovMatrix` over `numfields` device-sampled FFTRF fields (`gsi_op_lowrank_fftrf`): what
`getxis(() -> FFTRF.powerlaw_structuredgrid(Ns, k0, dk, beta), numfields, ...)` builds, with the fields generated, centred
(lowrank.jl:17-27) and kept in HBM."
function lowrank_fftrf_operator(Ns::Vector{Int}, k0::Float64, dk::Float64, beta::Float64, numfields::Int;
		seed::Integer=0, c::Context=ctx())
	r = Ref{Ptr{Cvoid}}(C_NULL)
	N64 = Int64.(Ns)
	n = prod(Ns)
	check(ccall((:gsi_op_lowrank_fftrf, libgsi), Cint,
		(Ptr{Cvoid}, Ref{Ptr{Cvoid}}, Cint, Ptr{Int64}, Cdouble, Cdouble, Cdouble, Int64, UInt64, Int64, Int64),
		c.h, r, length(N64), N64, k0, dk, beta, numfields, UInt64(seed), 0, n))
	op = DeviceOperator(r[], c, n, n)
	finalizer(finalize_op!, op)
	return op
end

"`numfields` fields of `FFTRF.powerlaw_unstructuredgrid(points, Ns, k0, dk, beta)` (FFTRF.jl:102-129) on the device
(`gsi_fftrf_fields_at`): an m x numfields `DeviceMatrix`, the fields of `fftrf_fields` (same `phi` / `seed` / `field0`)
interpolated at `points` (d x m) while they are in the sampler's workspace.  `box` (lo of every axis, then hi) replaces the
points' own extrema."
function fftrf_fields_at(points::Matrix{Float64}, Ns::Vector{Int}, k0::Float64, dk::Float64, beta::Float64, numfields::Int;
		phi::Union{Nothing,Matrix{Float64}}=nothing, seed::Integer=0, field0::Int=0,
		box::Union{Nothing,Vector{Float64}}=nothing, c::Context=ctx())
	N64 = Int64.(Ns)
	size(points, 1) == length(Ns) || error("points must be ndims x m")
	box === nothing || length(box) == 2 * length(Ns) || error("box must hold 2 ndims values")
	m = size(points, 2)
	F = DeviceMatrix(m, numfields; c=c)
	bx = box === nothing ? Ptr{Float64}(C_NULL) : pointer(box)
	if phi === nothing
		GC.@preserve box check(ccall((:gsi_fftrf_fields_at, libgsi), Cint,
			(Ptr{Cvoid}, Ptr{Cvoid}, Cint, Ptr{Int64}, Cdouble, Cdouble, Cdouble, Ptr{Float64}, Int64, UInt64, Int64,
			 Ptr{Float64}, Int64, Ptr{Float64}, Int64),
			c.h, F.h, length(N64), N64, k0, dk, beta, C_NULL, 0, UInt64(seed), field0, points, m, bx, 0))
	else
		size(phi, 2) == numfields || error("phi must have one column per field")
		GC.@preserve phi box check(ccall((:gsi_fftrf_fields_at, libgsi), Cint,
			(Ptr{Cvoid}, Ptr{Cvoid}, Cint, Ptr{Int64}, Cdouble, Cdouble, Cdouble, Ptr{Float64}, Int64, UInt64, Int64,
			 Ptr{Float64}, Int64, Ptr{Float64}, Int64),
			c.h, F.h, length(N64), N64, k0, dk, beta, phi, stride(phi, 2), UInt64(0), 0, points, m, bx, 0))
	end
	return F
end

"`FFTRF.powerlaw_unstructuredgrid(points, Ns, k0, dk, beta)` (FFTRF.jl:102-105): one field at the m points, on the host.
`phi` = the `randn(size(S))` array of `mulbyphi`; without it the device stream `seed`."
function powerlaw_unstructuredgrid(points::Matrix{Float64}, Ns::Vector{Int}, k0::Float64, dk::Float64, beta::Float64;
		phi::Union{Nothing,Array{Float64}}=nothing, seed::Integer=0, box::Union{Nothing,Vector{Float64}}=nothing,
		c::Context=ctx())
	ph = phi === nothing ? nothing : reshape(phi, length(phi), 1)
	F = fftrf_fields_at(points, Ns, k0, dk, beta, 1; phi=ph, seed=seed, box=box, c=c)
	out = Matrix{Float64}(undef, F.rows, 1)
	check(ccall((:gsi_mat_download, libgsi), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}, Int64), c.h, F.h, out, F.rows))
	return vec(out)
end

"`LowRankCovMatrix` over `numfields` such fields at the m points (`gsi_op_lowrank_fftrf_at`): what
`getxis(() -> FFTRF.powerlaw_unstructuredgrid(points, Ns, k0, dk, beta), numfields, ...)` builds, m x m, kept in HBM."
function lowrank_fftrf_operator(points::Matrix{Float64}, Ns::Vector{Int}, k0::Float64, dk::Float64, beta::Float64,
		numfields::Int; seed::Integer=0, box::Union{Nothing,Vector{Float64}}=nothing, c::Context=ctx())
	r = Ref{Ptr{Cvoid}}(C_NULL)
	N64 = Int64.(Ns)
	size(points, 1) == length(Ns) || error("points must be ndims x m")
	box === nothing || length(box) == 2 * length(Ns) || error("box must hold 2 ndims values")
	m = size(points, 2)
	bx = box === nothing ? Ptr{Float64}(C_NULL) : pointer(box)
	GC.@preserve box check(ccall((:gsi_op_lowrank_fftrf_at, libgsi), Cint,
		(Ptr{Cvoid}, Ref{Ptr{Cvoid}}, Cint, Ptr{Int64}, Cdouble, Cdouble, Cdouble, Int64, UInt64, Ptr{Float64}, Int64,
		 Ptr{Float64}, Int64, Int64),
		c.h, r, length(N64), N64, k0, dk, beta, numfields, UInt64(seed), points, m, bx, 0, m))
	op = DeviceOperator(r[], c, m, m)
	finalizer(finalize_op!, op)
	return op
end

"The adjoint of `FFTRF.interpolate` on the device (`gsi_fftrf_spread`): `V` (m x nf, values at the m `points`) spread onto
the grid `Ns` with the interpolation weights; returns the n x nf `DeviceMatrix` W' V.  Every entry is written, untouched
nodes are exactly 0.0, and the result is bit-identical from call to call."
function fftrf_spread(points::Matrix{Float64}, V, Ns::Vector{Int};      # V: a DeviceMatrix (defined below)
		box::Union{Nothing,Vector{Float64}}=nothing, c::Context=ctx())
	N64 = Int64.(Ns)
	size(points, 1) == length(Ns) || error("points must be ndims x m")
	box === nothing || length(box) == 2 * length(Ns) || error("box must hold 2 ndims values")
	m = size(points, 2)
	V.rows == m || error("V must have one row per point")
	G = DeviceMatrix(prod(Ns), V.cols; c=c)
	bx = box === nothing ? Ptr{Float64}(C_NULL) : pointer(box)
	GC.@preserve box check(ccall((:gsi_fftrf_spread, libgsi), Cint,
		(Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Cint, Ptr{Int64}, Ptr{Float64}, Int64, Ptr{Float64}, Int64),
		c.h, G.h, V.h, length(N64), N64, points, m, bx, 0))
	return G
end

"An FFT covariance operator read at scattered points (`gsi_op_fft_at`): W C W', m x m, with C the covariance of `grid_op`
(an `FFTGridCovariance` or power-law FFT operator with 2 or 3 axes of at least 2 points) and W the interpolation at `points`
(d x m) on its grid.  The grid operator's lengths are in grid spacings; its nugget is interpolated with everything else.
The plan of `grid_op` is shared: the two operators may be finalized in either order.  One GPU only."
function fft_operator_at(grid_op::DeviceOperator, points::Matrix{Float64};
		box::Union{Nothing,Vector{Float64}}=nothing, c::Context=ctx())
	r = Ref{Ptr{Cvoid}}(C_NULL)
	box === nothing || length(box) == 2 * size(points, 1) || error("box must hold 2 ndims values")
	m = size(points, 2)
	bx = box === nothing ? Ptr{Float64}(C_NULL) : pointer(box)
	GC.@preserve box check(ccall((:gsi_op_fft_at, libgsi), Cint,
		(Ptr{Cvoid}, Ref{Ptr{Cvoid}}, Ptr{Cvoid}, Ptr{Float64}, Int64, Ptr{Float64}),
		c.h, r, grid_op.h, points, m, bx))
	op = DeviceOperator(r[], c, m, m)
	finalizer(finalize_op!, op)
	return op
end

# ---- Gaussian fields with a grid covariance function (circulant embedding, gsi_gridcov_sampler_*) --
const GRIDCOV_KINDS = Dict("gaussian" => 0, "exponential" => 1, "matern32" => 2, "matern52" => 3)

"The plan of one grid and covariance function (`gsi_sampler`): `M` the torus, `info` = (neg_mass, lambda_min, lambda_max,
clamped count) as creation found them."
mutable struct GridCovSampler
	h::Ptr{Cvoid}
	c::Context
	Ns::Vector{Int}
	M::Vector{Int}
	info::Vector{Float64}
end
function finalize_sampler!(s::GridCovSampler)
	s.h != C_NULL && ccall((:gsi_gridcov_sampler_destroy, libgsi), Cint, (Ptr{Cvoid},), s.h)
	s.h = C_NULL
end

"The sampler of the covariance of `gsi_op_fft_gridcov(Ns, kind, ell, theta, sigma2, nugget)` on a 2-D or 3-D grid
(`gsi_gridcov_sampler_create`).  `embed`: the torus per axis (powers of two, 2 N <= M <= 8192; `nothing`: the next power of
two >= 2 N).  Refused (GSI_ERR_NOT_POSDEF) when the clamped negative part of the spectrum exceeds `neg_tol`."
function gridcov_sampler(Ns::Vector{Int}; kind::String="exponential", ell::Vector{Float64}=ones(length(Ns)), theta::Float64=0.0,
		sigma2::Float64=1.0, nugget::Float64=0.0, embed::Union{Nothing,Vector{Int}}=nothing, neg_tol::Float64=1e-12,
		c::Context=ctx())
	length(ell) == length(Ns) || error("ell must hold one length per axis")
	embed === nothing || length(embed) == length(Ns) || error("embed must hold one torus length per axis")
	N64 = Int64.(Ns)
	M64 = embed === nothing ? Int64[] : Int64.(embed)
	mp = embed === nothing ? Ptr{Int64}(C_NULL) : pointer(M64)
	r = Ref{Ptr{Cvoid}}(C_NULL)
	info = zeros(Float64, 4)
	GC.@preserve M64 check(ccall((:gsi_gridcov_sampler_create, libgsi), Cint,
		(Ptr{Cvoid}, Ref{Ptr{Cvoid}}, Cint, Ptr{Int64}, Ptr{Int64}, Cint, Ptr{Float64}, Cdouble, Cdouble, Cdouble, Cdouble,
		 Ptr{Float64}),
		c.h, r, length(N64), N64, mp, GRIDCOV_KINDS[kind], ell, theta, sigma2, nugget, neg_tol, info))
	M = zeros(Int64, 3)
	check(ccall((:gsi_gridcov_sampler_info, libgsi), Cint, (Ptr{Cvoid}, Ptr{Int64}, Ptr{Float64}), r[], M, info))
	s = GridCovSampler(r[], c, copy(Ns), Int.(M[1:length(Ns)]), info)
	finalizer(finalize_sampler!, s)
	return s
end

"lambda on the torus (size `M`, unclamped, nugget included): `gsi_gridcov_sampler_spectrum`."
function spectrum(s::GridCovSampler)
	lam = Vector{Float64}(undef, prod(s.M))
	check(ccall((:gsi_gridcov_sampler_spectrum, libgsi), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}), s.c.h, s.h, lam))
	return reshape(lam, s.M...)
end

"`numfields` fields of the sampler (`gsi_gridcov_fields`): an n x numfields `DeviceMatrix`, column c = `vec` of field
`field0 + c` (`field0` even).  `eps` (Mtot x 2 ceil(numfields / 2), column c the noise of role c in torus order) fixes the
random numbers; without it role f draws the device stream `seed + f`."
function fields(s::GridCovSampler, numfields::Int; eps::Union{Nothing,Matrix{Float64}}=nothing, seed::Integer=0, field0::Int=0)
	F = DeviceMatrix(prod(s.Ns), numfields; c=s.c)
	if eps === nothing
		check(ccall((:gsi_gridcov_fields, libgsi), Cint,
			(Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}, Int64, UInt64, Int64),
			s.c.h, s.h, F.h, C_NULL, 0, UInt64(seed), field0))
	else
		size(eps) == (prod(s.M), 2 * cld(numfields, 2)) || error("eps must be Mtot x 2 ceil(numfields / 2)")
		GC.@preserve eps check(ccall((:gsi_gridcov_fields, libgsi), Cint,
			(Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}, Int64, UInt64, Int64),
			s.c.h, s.h, F.h, eps, stride(eps, 2), UInt64(0), 0))
	end
	return F
end

"`LowRankCovMatrix` over `numfields` device-sampled fields of the sampler (`gsi_op_lowrank_gridcov`), centred and kept in HBM."
function lowrank_gridcov_operator(s::GridCovSampler, numfields::Int; seed::Integer=0)
	r = Ref{Ptr{Cvoid}}(C_NULL)
	n = prod(s.Ns)
	check(ccall((:gsi_op_lowrank_gridcov, libgsi), Cint,
		(Ptr{Cvoid}, Ref{Ptr{Cvoid}}, Ptr{Cvoid}, Int64, UInt64, Int64, Int64),
		s.c.h, r, s.h, numfields, UInt64(seed), 0, n))
	op = DeviceOperator(r[], s.c, n, n)
	finalizer(finalize_op!, op)
	return op
end

"Gaussian covariance exp(-d^2/(2 ell^2)) of an nx x ny unit grid as a matrix-free operator: entries are regenerated
inside the product kernel, nothing of size n^2 is stored (`gsi_op_gridcov_implicit`).  Usable wherever a Matrix is."
function GridCovImplicit(nx::Int, ny::Int, ell::Float64; c::Context=ctx())
	r = Ref{Ptr{Cvoid}}(C_NULL)
	check(ccall((:gsi_op_gridcov_implicit, libgsi), Cint,
		(Ptr{Cvoid}, Ref{Ptr{Cvoid}}, Int64, Int64, Cdouble, Int64, Int64),
		c.h, r, nx, ny, ell, 0, nx * ny))
	op = DeviceOperator(r[], c, nx * ny, nx * ny)
	finalizer(finalize_op!, op)
	return op
end

"The same operator for another stationary kernel on the nx x ny unit grid: `kind = :gaussian` (exp(-d^2/(2 ell^2))),
`kind = :exponential` (exp(-d/ell)), or any covariance of the grid offsets handed over as a table
`table[dy + 1, dx + 1] = k(dx, dy)` (ny x nx: Matern, anisotropic, nested ...).  `gsi_op_gridcov_implicit_kind`,
`gsi_op_gridcov_implicit_table`; entries are looked up in that 8 n-byte table inside the product kernel."
function GridCovImplicit(nx::Int, ny::Int, ell::Float64, kind::Symbol; c::Context=ctx())
	k = kind == :gaussian ? 0 : kind == :exponential ? 1 : error("GridCovImplicit: kind must be :gaussian or :exponential")
	r = Ref{Ptr{Cvoid}}(C_NULL)
	check(ccall((:gsi_op_gridcov_implicit_kind, libgsi), Cint,
		(Ptr{Cvoid}, Ref{Ptr{Cvoid}}, Int64, Int64, Cdouble, Cint, Int64, Int64),
		c.h, r, nx, ny, ell, k, 0, nx * ny))
	op = DeviceOperator(r[], c, nx * ny, nx * ny)
	finalizer(finalize_op!, op)
	return op
end
function GridCovImplicit(table::Matrix{Float64}; c::Context=ctx())
	ny, nx = size(table)                       # column-major ny x nx  ==  t[dx * ny + dy] of the C ABI
	r = Ref{Ptr{Cvoid}}(C_NULL)
	check(ccall((:gsi_op_gridcov_implicit_table, libgsi), Cint,
		(Ptr{Cvoid}, Ref{Ptr{Cvoid}}, Int64, Int64, Ptr{Float64}, Int64, Int64),
		c.h, r, nx, ny, table, 0, nx * ny))
	op = DeviceOperator(r[], c, nx * ny, nx * ny)
	finalizer(finalize_op!, op)
	return op
end

"The covariance of scattered points as an implicit operator: `A[i, j] = sigma2 * k(|x_i - x_j| / ell)` (+ `nugget` on the
diagonal), `points` d x n as `FFTRF.powerlaw_unstructuredgrid` takes them (FFTRF.jl:102), `kind` in `:gaussian`,
`:exponential`, `:matern32`, `:matern52` (`gsi_op_pointcov_implicit`).  Nothing n x n is stored: row panels of A are
generated on a second stream while the MFMA contraction consumes the previous one.  Usable wherever a Matrix is."
function PointCovImplicit(points::Matrix{Float64}, kind::Symbol=:exponential; ell::Float64=1.0, sigma2::Float64=1.0,
		nugget::Float64=0.0, c::Context=ctx())
	k = Dict(:gaussian=>0, :exponential=>1, :matern32=>2, :matern52=>3)[kind]
	d, n = size(points)
	r = Ref{Ptr{Cvoid}}(C_NULL)
	check(ccall((:gsi_op_pointcov_implicit, libgsi), Cint,
		(Ptr{Cvoid}, Ref{Ptr{Cvoid}}, Ptr{Float64}, Int64, Cint, Cint, Cdouble, Cdouble, Cdouble, Int64, Int64),
		c.h, r, points, n, d, k, ell, sigma2, nugget, 0, n))
	op = DeviceOperator(r[], c, n, n)
	finalizer(finalize_op!, op)
	return op
end

"The covariance of `FFTRF.powerlaw_structuredgrid(Ns, k0, dk, beta)` fields themselves (up to dk^2 and the per-sample
mean / std normalisation, FFTRF.jl:94-98): FFTRF's own embedding of exactly 2N points per axis and its integer
wavenumbers (FFTRF.jl:83-90, computesqrtS_f :40-72), `gsi_op_fft_powerlaw_fftrf`.  Acts on `vec(field)`; every grid
dimension must be a power of two (the exact `getxis(samplefield, ...)` sample estimate becomes this operator as the number
of fields grows: tests/test_fftrf_covariance.py)."
function FFTRFCovariance(Ns::Vector{Int}, beta::Float64; c::Context=ctx())
	r = Ref{Ptr{Cvoid}}(C_NULL)
	N64 = Int64.(Ns)
	check(ccall((:gsi_op_fft_powerlaw_fftrf, libgsi), Cint,
		(Ptr{Cvoid}, Ref{Ptr{Cvoid}}, Cint, Ptr{Int64}, Cdouble),
		c.h, r, length(N64), N64, beta))
	n = prod(Ns)
	op = DeviceOperator(r[], c, n, n)
	finalizer(finalize_op!, op)
	return op
end

"Matrix-free stationary power-law covariance on a structured grid (circulant embedding on the next power of two
>= 2N per axis, spectrum |k|^beta with k in cycles per grid spacing, unit diagonal): `gsi_op_fft_powerlaw`.  Acts on
`vec(field)`.  It is the covariance family FFTRF.powerlaw_structuredgrid samples from; it coincides with the
covariance of those fields (up to the per-sample normalisation) only on power-of-two grids with equal axes --
FFTRF embeds on exactly 2N points and uses integer wavenumbers (FFTRF.jl:83-90), see DESIGN.md section 4.6."
function FFTPowerlawCovariance(Ns::Vector{Int}, beta::Float64; c::Context=ctx())
	r = Ref{Ptr{Cvoid}}(C_NULL)
	N64 = Int64.(Ns)
	check(ccall((:gsi_op_fft_powerlaw, libgsi), Cint,
		(Ptr{Cvoid}, Ref{Ptr{Cvoid}}, Cint, Ptr{Int64}, Cdouble),
		c.h, r, length(N64), N64, beta))
	n = prod(Ns)
	op = DeviceOperator(r[], c, n, n)
	finalizer(finalize_op!, op)
	return op
end

"A covariance function on a regular grid as the matrix-free FFT operator (`gsi_op_fft_gridcov`):
`A[i, j] = sigma2 * k(r) + nugget * (i == j)`, `r^2 = sum_a (u_a / ell[a])^2`, `u` = the lag `i - j` per axis (rotated by
`theta` in 2-D), unit grid spacing, `kind` in `:gaussian`, `:exponential`, `:matern32`, `:matern52`.  Acts on `vec(field)`.
For `Ns = [ny, nx]` it is the matrix of `GridCovImplicit(nx, ny, ...)` in the same point order, at O(n log n) per column."
function FFTGridCovariance(Ns::Vector{Int}, kind::Symbol=:exponential; ell::Union{Float64,Vector{Float64}}=1.0,
		theta::Float64=0.0, sigma2::Float64=1.0, nugget::Float64=0.0, c::Context=ctx())
	k = Dict(:gaussian=>0, :exponential=>1, :matern32=>2, :matern52=>3)[kind]
	r = Ref{Ptr{Cvoid}}(C_NULL)
	N64 = Int64.(Ns)
	ells = ell isa Float64 ? fill(ell, length(Ns)) : ell
	length(ells) == length(Ns) || error("FFTGridCovariance: ell must be one length or one per axis")
	check(ccall((:gsi_op_fft_gridcov, libgsi), Cint,
		(Ptr{Cvoid}, Ref{Ptr{Cvoid}}, Cint, Ptr{Int64}, Cint, Ptr{Float64}, Cdouble, Cdouble, Cdouble),
		c.h, r, length(N64), N64, k, ells, theta, sigma2, nugget))
	n = prod(Ns)
	op = DeviceOperator(r[], c, n, n)
	finalizer(finalize_op!, op)
	return op
end
"The same operator for any stationary kernel given by its lags (`gsi_op_fft_gridcov_table`): `table[t0 + 1, t1 + 1, ...] =
c(t)` for `t >= 0`, an array of the grid's own shape, even along every axis; in 2-D `mirror[t0 + 1, t1 + 1] = c(t0, -t1)`
makes it any centrally symmetric kernel (rotated anisotropy, nested structures)."
function FFTGridCovariance(table::Array{Float64}; mirror::Union{Nothing,Matrix{Float64}}=nothing, nugget::Float64=0.0,
		c::Context=ctx())
	(1 <= ndims(table) <= 3) || error("FFTGridCovariance: the table has 1 to 3 axes")
	(mirror === nothing || size(mirror) == size(table)) || error("FFTGridCovariance: mirror must have the shape of table")
	r = Ref{Ptr{Cvoid}}(C_NULL)
	N64 = Int64[size(table)...]
	check(ccall((:gsi_op_fft_gridcov_table, libgsi), Cint,
		(Ptr{Cvoid}, Ref{Ptr{Cvoid}}, Cint, Ptr{Int64}, Ptr{Float64}, Ptr{Float64}, Cdouble),
		c.h, r, length(N64), N64, table, mirror === nothing ? C_NULL : mirror, nugget))
	n = length(table)
	op = DeviceOperator(r[], c, n, n)
	finalizer(finalize_op!, op)
	return op
end

Base.size(A::DeviceOperator) = (A.m, A.n)
function Base.size(A::DeviceOperator, i::Int)
	(i == 1 || i == 2) || error("there is no $i-th dimension in a DeviceOperator")   # lowrank.jl:58
	return i == 1 ? A.m : A.n
end
Base.eltype(::DeviceOperator) = Float64
function Base.:*(A::DeviceOperator, X::Matrix{Float64})                                   # lowrank.jl:115-121
	Y = Matrix{Float64}(undef, A.m, size(X, 2))
	check(ccall((:gsi_op_mul, libgsi), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Ptr{Float64}, Int64, Int64, Ptr{Float64}, Int64),
		A.c.h, A.h, 0, X, stride(X, 2), size(X, 2), Y, A.m))
	return Y
end

"`adjoint(A) * X`  (RandMatFact.jl:67,85)"
struct AdjointOperator
	parent::DeviceOperator
end
Base.adjoint(A::DeviceOperator) = AdjointOperator(A)
Base.transpose(A::DeviceOperator) = AdjointOperator(A)
Base.size(A::AdjointOperator) = (A.parent.n, A.parent.m)
function Base.size(A::AdjointOperator, i::Int)
	(i == 1 || i == 2) || error("there is no $i-th dimension in a DeviceOperator")   # lowrank.jl:58
	return i == 1 ? A.parent.n : A.parent.m
end
Base.eltype(::AdjointOperator) = Float64
Base.adjoint(At::AdjointOperator) = At.parent
Base.transpose(At::AdjointOperator) = At.parent
Base.:*(At::AdjointOperator, x::Vector{Float64}) = vec(At * reshape(x, :, 1))
function Base.:*(At::AdjointOperator, X::Matrix{Float64})
	A = At.parent
	Y = Matrix{Float64}(undef, A.n, size(X, 2))
	check(ccall((:gsi_op_mul, libgsi), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Ptr{Float64}, Int64, Int64, Ptr{Float64}, Int64),
		A.c.h, A.h, 1, X, stride(X, 2), size(X, 2), Y, A.n))
	return Y
end
Base.:*(A::DeviceOperator, x::Vector{Float64}) = vec(A * reshape(x, :, 1))            # lowrank.jl:135-139

"`mul!(v, A, x)`  (lowrank.jl:75-81): v = A x into the caller's vector -- what IterativeSolvers.lsqr calls on the operator."
function LinearAlgebra.mul!(v::Vector{Float64}, A::DeviceOperator, x::Vector{Float64})
	length(v) == A.m && length(x) == A.n || throw(DimensionMismatch("mul!: A is $(A.m)x$(A.n), x has $(length(x)), v has $(length(v))"))
	check(ccall((:gsi_op_mul, libgsi), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Ptr{Float64}, Int64, Int64, Ptr{Float64}, Int64),
		A.c.h, A.h, 0, x, A.n, 1, v, A.m))
	return v
end
function LinearAlgebra.mul!(v::Vector{Float64}, At::AdjointOperator, x::Vector{Float64})
	A = At.parent
	length(v) == A.n && length(x) == A.m || throw(DimensionMismatch("mul!: A' is $(A.n)x$(A.m), x has $(length(x)), v has $(length(v))"))
	check(ccall((:gsi_op_mul, libgsi), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Ptr{Float64}, Int64, Int64, Ptr{Float64}, Int64),
		A.c.h, A.h, 1, x, A.m, 1, v, A.n))
	return v
end

"`B * A` for a plain matrix B  (lowrank.jl:123-129; `I * lrcm` at test/testrpcga.jl:49,90): B A = (A' B')', one device
product on the transposed panel."
function Base.:*(B::Matrix{Float64}, A::DeviceOperator)
	size(B, 2) == A.m || throw(DimensionMismatch("B has $(size(B, 2)) columns, A has $(A.m) rows"))
	return Matrix((adjoint(A) * Matrix(B'))')
end
"`B' * A` for an adjoint matrix  (lowrank.jl:131-133, RandMatFact.jl:85 `Q' * A`): (A' B)' -- for the symmetric
LowRankCovMatrix this is the reference's `(A * B.parent)'`."
function Base.:*(B::LinearAlgebra.Adjoint{Float64, Matrix{Float64}}, A::DeviceOperator)
	size(B, 2) == A.m || throw(DimensionMismatch("B' has $(size(B, 2)) columns, A has $(A.m) rows"))
	return (adjoint(A) * B.parent)'
end

"`\\(A::LowRankCovMatrix, b::Vector)`  (lowrank.jl:141-144): lsqr(A, b; maxiter=length(A.samples)) on the device."
function Base.:\(A::DeviceOperator, b::Vector{Float64})
	x = Vector{Float64}(undef, A.n)
	check(ccall((:gsi_op_lowrank_solve, libgsi), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Int64}),
		A.c.h, A.h, b, x, C_NULL))
	return x
end

# ---- device-resident matrices and the xi-basis (SURVEY.md 8b last row / 8f f1) -----------------------------
mutable struct DeviceMatrix
	h::Ptr{Cvoid}
	c::Context
	rows::Int
	cols::Int
	function DeviceMatrix(rows::Int, cols::Int; c::Context=ctx())
		r = Ref{Ptr{Cvoid}}(C_NULL)
		check(ccall((:gsi_mat_create, libgsi), Cint, (Ptr{Cvoid}, Ref{Ptr{Cvoid}}, Int64, Int64), c.h, r, rows, cols))
		m = new(r[], c, rows, cols)
		finalizer(m) do x
			x.h != C_NULL && ccall((:gsi_mat_destroy, libgsi), Cint, (Ptr{Cvoid},), x.h)
			x.h = C_NULL
		end
		return m
	end
end
function DeviceMatrix(A::Matrix{Float64}; c::Context=ctx())
	m = DeviceMatrix(size(A, 1), size(A, 2); c=c)
	check(ccall((:gsi_mat_upload, libgsi), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}, Int64), c.h, m.h, A, stride(A, 2)))
	return m
end

# ---- kriging systems: (A + diag) X = B by conjugate gradients, all columns together (gsi_op_solve_cg; no counterpart in
#      the reference, whose only solver is lsqr on a LowRankCovMatrix) -----------------------------------------------------
"`solve(A, B; diag, tol, maxiter)`: `(A + Diagonal(diag)) \\ B` for a square, symmetric positive semidefinite device operator
by conjugate gradients on the device.  `B`: a `Vector`, a `Matrix` or a `DeviceMatrix`; the result is of the same kind.
Returns `(X, info)` with `info = (products, converged, path, breakdown, relres, iters)`; an operator that is not positive
definite along a search direction raises through `check`."
function solve(A::DeviceOperator, B::Matrix{Float64}; diag::Union{Nothing, Vector{Float64}}=nothing, tol::Float64=1e-10,
		maxiter::Int=10 * A.n)
	size(B, 1) == A.n || throw(DimensionMismatch("solve: A is $(A.m)x$(A.n), B has $(size(B, 1)) rows"))
	b = size(B, 2)
	X = Matrix{Float64}(undef, A.n, b)
	info = zeros(Int64, 4)
	relres = zeros(Float64, b)
	iters = zeros(Int64, b)
	check(ccall((:gsi_op_solve, libgsi), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Int64, Int64, Ptr{Float64},
			Int64, Float64, Int64, Ptr{Int64}, Ptr{Float64}, Ptr{Int64}),
		A.c.h, A.h, diag === nothing ? C_NULL : diag, B, stride(B, 2), b, X, A.n, tol, maxiter, info, relres, iters))
	return X, (products=info[1], converged=info[2], path=info[3], breakdown=info[4], relres=relres, iters=iters)
end
function solve(A::DeviceOperator, b::Vector{Float64}; kw...)
	X, info = solve(A, reshape(b, :, 1); kw...)
	return vec(X), info
end
function solve(A::DeviceOperator, B::DeviceMatrix; diag::Union{Nothing, Vector{Float64}}=nothing, tol::Float64=1e-10,
		maxiter::Int=10 * A.n)
	X = DeviceMatrix(B.rows, B.cols; c=A.c)
	info = zeros(Int64, 4)
	relres = zeros(Float64, B.cols)
	iters = zeros(Int64, B.cols)
	check(ccall((:gsi_op_solve_cg, libgsi), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}, Ptr{Cvoid}, Ptr{Cvoid}, Float64, Int64,
			Ptr{Int64}, Ptr{Float64}, Ptr{Int64}),
		A.c.h, A.h, diag === nothing ? C_NULL : diag, B.h, X.h, tol, maxiter, info, relres, iters))
	return X, (products=info[1], converged=info[2], path=info[3], breakdown=info[4], relres=relres, iters=iters)
end
"`solve_trace(A, B, nquad; diag, qmax, tol, maxiter)`: the same solve of the resident `B` with the conjugate-gradient
coefficients of every column kept on the device, and the Gauss rule of stochastic Lanczos quadrature `rho0 * e1' log(T) e1` for
the last `nquad` columns (gsi_op_solve_trace without a preconditioner): with columns `z ~ N(0, I)` the mean of the values
estimates `logdet(A + Diagonal(diag))`.  Returns `(X, info)`, `info` as `solve` plus `truncated`, `quad` and `rho0` per column."
function solve_trace(A::DeviceOperator, B::DeviceMatrix, nquad::Int; diag::Union{Nothing, Vector{Float64}}=nothing,
		qmax::Int=512, tol::Float64=1e-8, maxiter::Int=10 * A.n)
	b = B.cols
	X = DeviceMatrix(B.rows, b; c=A.c)
	info = zeros(Int64, 7)
	relres = zeros(Float64, b)
	iters = zeros(Int64, b)
	quad = zeros(Float64, 2 * b)
	check(ccall((:gsi_op_solve_trace, libgsi), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid},
			Int64, Int64, Float64, Int64, Ptr{Int64}, Ptr{Float64}, Ptr{Int64}, Ptr{Float64}),
		A.c.h, A.h, diag === nothing ? C_NULL : diag, C_NULL, B.h, X.h, nquad, qmax, tol, maxiter, info, relres, iters, quad))
	return X, (products=info[1], converged=info[2], path=info[3], breakdown=info[4], truncated=info[7], relres=relres,
		iters=iters, quad=quad[1:b], rho0=quad[b+1:2b])
end
"`slq_quadrature(alpha, beta, steps, rho0)`: the quadrature alone (gsi_slq_quadrature).  `alpha`, `beta`: b x qmax, column j's
step k at `[j, k]` (the library's step-major layout); `steps`: the entries of each column to use."
function slq_quadrature(alpha::Matrix{Float64}, beta::Matrix{Float64}, steps::Vector{Int64}, rho0::Vector{Float64};
		c::Context=ctx())
	b, qmax = size(alpha)
	size(beta) == (b, qmax) && length(steps) == b && length(rho0) == b || throw(DimensionMismatch("slq_quadrature: shapes differ"))
	out = zeros(Float64, b)
	check(ccall((:gsi_slq_quadrature, libgsi), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Int64}, Ptr{Float64}, Int64,
			Int64, Ptr{Float64}),
		c.h, alpha, beta, steps, rho0, qmax, b, out))
	return out
end
"`pivoted_cholesky(A, K; tol)`: the diagonal-pivoted Cholesky factor `L L' ~ A` of a dense, implicit grid-covariance or implicit
point-covariance device operator from K columns of A and no operator product (gsi_op_pivoted_cholesky).  Returns
`(L, piv, info)`: `L` a `DeviceMatrix` of n x K with zeros from column `rank + 1` on, `piv` the 1-based pivot rows (the rank
entries), `info = (rank, reason, path, form, polls, trace0, trace, dmax)` with reason 1 (rank K reached), 2 (the trace of the
remainder fell to `tol` times the trace of A) or 3 (A is exhausted)."
function pivoted_cholesky(A::DeviceOperator, K::Int; tol::Float64=0.0)
	1 <= K <= min(A.n, 2048) || throw(ArgumentError("pivoted_cholesky: K must lie in 1:min(n, 2048)"))
	L = DeviceMatrix(A.n, K; c=A.c)
	piv = fill(Int64(-1), K)
	info = zeros(Int64, 6)
	err = zeros(Float64, 3)
	check(ccall((:gsi_op_pivoted_cholesky, libgsi), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Int64, Float64, Ptr{Cvoid}, Ptr{Int64},
			Ptr{Int64}, Ptr{Float64}),
		A.c.h, A.h, K, tol, L.h, piv, info, err))
	rank = Int(info[1])
	return L, piv[1:rank] .+ 1, (rank=rank, reason=info[2], path=info[3], form=info[4], polls=info[5], trace0=err[1],
		trace=err[2], dmax=err[3])
end
"`axpy!(alpha, X, Y)` for device matrices of one shape: Y += alpha X."
function LinearAlgebra.axpy!(alpha::Real, X::DeviceMatrix, Y::DeviceMatrix)
	check(ccall((:gsi_mat_axpy, libgsi), Cint, (Ptr{Cvoid}, Float64, Ptr{Cvoid}, Ptr{Cvoid}), Y.c.h, Float64(alpha), X.h, Y.h))
	return Y
end

"The xi-basis resident in HBM: what `getxis_device` returns and what `pcgadirect` / `pcgalsqr` / `rga` accept in place
of `xis::Array{Array{Float64,1},1}`.  `precision = 32` stores the K columns in fp32 (all sums in fp64)."
mutable struct DeviceBasis
	h::Ptr{Cvoid}
	Z::DeviceMatrix            # kept alive: a 64-bit basis points into it
	n::Int
	K::Int
	function DeviceBasis(Z::DeviceMatrix, K::Int; precision::Int=64)
		r = Ref{Ptr{Cvoid}}(C_NULL)
		check(ccall((:gsi_basis_create, libgsi), Cint, (Ptr{Cvoid}, Ref{Ptr{Cvoid}}, Ptr{Cvoid}, Int64, Cint),
			Z.c.h, r, Z.h, K, precision))
		b = new(r[], Z, Z.rows, K)
		finalizer(b) do x
			x.h != C_NULL && ccall((:gsi_basis_destroy, libgsi), Cint, (Ptr{Cvoid},), x.h)
			x.h = C_NULL
		end
		return b
	end
end
Base.length(b::DeviceBasis) = b.K
function Base.getindex(b::DeviceBasis, i::Int)                                           # xis[i] on the host
	x = Vector{Float64}(undef, b.n)
	check(ccall((:gsi_basis_download_col, libgsi), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Int64, Ptr{Float64}), b.Z.c.h, b.h, i - 1, x))
	return x
end
"paramstorun as an n x (K+3) matrix: columns s + delta*xis[i], s + delta*X, s + delta*s, s   (direct.jl:39-45)"
function paramstorun(b::DeviceBasis, s::Vector{Float64}, X::Vector{Float64}, delta::Float64)
	P = Matrix{Float64}(undef, b.n, b.K + 3)
	check(ccall((:gsi_pcga_params_basis, libgsi), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Cdouble, Ptr{Float64}),
		b.Z.c.h, b.h, s, X, delta, P))
	return P
end
"s = X*beta_bar + sum_i xis[i]*dot(etas[i], xi_bar)   (direct.jl:59-65, lsqr.jl:55-61)"
function update(b::DeviceBasis, X::Vector{Float64}, beta_bar::Float64, etas::Matrix{Float64}, xi_bar::Vector{Float64})
	s = Vector{Float64}(undef, b.n)
	check(ccall((:gsi_pcga_update_basis, libgsi), Cint,
		(Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}, Cdouble, Ptr{Float64}, Int64, Ptr{Float64}, Ptr{Float64}),
		b.Z.c.h, b.h, X, beta_bar, etas, size(etas, 1), xi_bar, s))
	return s
end

"A forward model resident on the device: h(s)[r] = sum_t H[r, j_t] g(w[j_t] s[j_t]) over the nonzeros of row r of the sparse H
(nobs x n), g = identity (`link = :identity`) or exp (`link = :exp`), w = `weights` (nothing: ones).  With a `DeviceBasis` the
`pcgadirect` / `pcgalsqr` / `rga` methods below compute the K+3 model runs of an iteration (direct.jl:38-46, lsqr.jl:36-51) on
the device from the resident basis; `fwd(s)` applies it to a host vector like any forward model.  The library wants CSR: it is
the CSC of the transpose, with the 1-based indices made 0-based."
mutable struct LinearForwardModel
	h::Ptr{Cvoid}
	c::Context
	nobs::Int
	n::Int
	function LinearForwardModel(H::SparseArrays.SparseMatrixCSC; weights::Union{Nothing,Vector{Float64}}=nothing,
			link::Symbol=:identity, c::Context=ctx())
		Ht = SparseArrays.sparse(transpose(H))                                          # n x nobs: column r = row r of H
		rowptr = Vector{Int64}(Ht.colptr .- 1)
		colidx = Vector{Int64}(Ht.rowval .- 1)
		vals = Vector{Float64}(Ht.nzval)
		w = weights === nothing ? C_NULL : weights                                      # NULL: ones
		r = Ref{Ptr{Cvoid}}(C_NULL)
		check(ccall((:gsi_fwd_linear_create, libgsi), Cint,
			(Ptr{Cvoid}, Ref{Ptr{Cvoid}}, Int64, Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Float64}, Ptr{Float64}, Cint),
			c.h, r, size(H, 1), size(H, 2), rowptr, colidx, vals, w, link == :exp ? 1 : 0))
		f = new(r[], c, size(H, 1), size(H, 2))
		finalizer(f) do x
			x.h != C_NULL && ccall((:gsi_fwd_destroy, libgsi), Cint, (Ptr{Cvoid},), x.h)
			x.h = C_NULL
		end
		return f
	end
end
"[nobs, n, nnz, segments, split rows, form of the last product, products on the host path, products in total]"
function info(f::LinearForwardModel)
	out = zeros(Int64, 8)
	check(ccall((:gsi_fwd_info, libgsi), Cint, (Ptr{Cvoid}, Ptr{Int64}, Int64), f.h, out, length(out)))
	return out
end
"h of every column of the host matrix P (n x ncols)"
function apply(f::LinearForwardModel, P::Matrix{Float64})
	out = Matrix{Float64}(undef, f.nobs, size(P, 2))
	check(ccall((:gsi_fwd_apply, libgsi), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}, Int64, Int64, Ptr{Float64}, Int64),
		f.c.h, f.h, P, stride(P, 2), size(P, 2), out, f.nobs))
	return out
end
(f::LinearForwardModel)(s::Vector{Float64}) = vec(apply(f, reshape(s, :, 1)))
"The nobs x (K+3) results of direct.jl:38-46 / lsqr.jl:36-51, computed on the device; the batch is never formed."
function forward(b::DeviceBasis, f::LinearForwardModel, s::Vector{Float64}, X::Vector{Float64}, delta::Float64)
	out = Matrix{Float64}(undef, f.nobs, b.K + 3)
	check(ccall((:gsi_pcga_forward_basis, libgsi), Cint,
		(Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Cdouble, Ptr{Float64}),
		b.Z.c.h, b.h, f.h, s, X, delta, out))
	return out
end
"S * fwd(.) for `rga` with the model kept on the device: S multiplies the small results"
struct ReducedForwardModel
	fwd::LinearForwardModel
	S::Matrix{Float64}
end
(r::ReducedForwardModel)(s::Vector{Float64}) = r.S * r.fwd(s)
const DeviceForwardModel = Union{LinearForwardModel, ReducedForwardModel}

"`PCGALowRankMatrix(etas, HX, R)` (lowrank.jl:32-36) resident on the device; `A * x` and `lsqr(A, b)` run there."
mutable struct PCGALowRankMatrix
	h::Ptr{Cvoid}
	c::Context
	nobs::Int
	function PCGALowRankMatrix(etas::Matrix{Float64}, HX::Vector{Float64}, R::AbstractMatrix; c::Context=ctx())
		nobs, K = size(etas)
		isdiag = R == LinearAlgebra.Diagonal(LinearAlgebra.diag(R))
		Rv = isdiag ? collect(Float64, LinearAlgebra.diag(R)) : vec(Matrix{Float64}(R))
		r = Ref{Ptr{Cvoid}}(C_NULL)
		check(ccall((:gsi_pcgamat_create, libgsi), Cint,
			(Ptr{Cvoid}, Ref{Ptr{Cvoid}}, Ptr{Float64}, Int64, Int64, Ptr{Float64}, Ptr{Float64}, Cint),
			c.h, r, etas, nobs, K, HX, Rv, isdiag ? 1 : 0))
		A = new(r[], c, nobs)
		finalizer(A) do x
			x.h != C_NULL && ccall((:gsi_pcgamat_destroy, libgsi), Cint, (Ptr{Cvoid},), x.h)
			x.h = C_NULL
		end
		return A
	end
end
Base.size(A::PCGALowRankMatrix) = (A.nobs + 1, A.nobs + 1)
function Base.size(A::PCGALowRankMatrix, i::Int)
	(i == 1 || i == 2) || error("there is no $i-th dimension in a PCGALowRankMatrix")     # lowrank.jl:71
	return A.nobs + 1
end
function Base.:*(A::PCGALowRankMatrix, x::Vector{Float64})                                # lowrank.jl:83-97, 109-113
	y = Vector{Float64}(undef, A.nobs + 1)
	check(ccall((:gsi_pcgamat_mul, libgsi), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}), A.c.h, A.h, x, y))
	return y
end
"`IterativeSolvers.lsqr(A, b)` with that package's defaults, on the device   (lsqr.jl:54)"
function lsqr(A::PCGALowRankMatrix, b::Vector{Float64})
	x = Vector{Float64}(undef, A.nobs + 1)
	check(ccall((:gsi_pcgamat_lsqr, libgsi), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Int64}),
		A.c.h, A.h, b, x, C_NULL))
	return x
end
"`A \\ b` by Cholesky of HQH + R on the device (`gsi_pcgamat_solve`; direct.jl:56-58 for a positive definite HQH + R).
Throws `PosDefException` when HQH + R is not positive definite and `SingularException` when HX = 0."
function solve(A::PCGALowRankMatrix, b::Vector{Float64})
	x = Vector{Float64}(undef, A.nobs + 1)
	info = zeros(Int64, 2)
	check(ccall((:gsi_pcgamat_solve, libgsi), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Int64}),
		A.c.h, A.h, b, x, info))
	return x
end
"`cholesky(Symmetric(A, :L)).L` by the blocked device factorization (`gsi_chol_lower`)"
function chol_lower(A::Matrix{Float64}; c::Context=ctx())
	n = size(A, 1)
	Lout = Matrix{Float64}(undef, n, n)
	info = zeros(Int64, 2)
	check(ccall((:gsi_chol_lower, libgsi), Cint, (Ptr{Cvoid}, Ptr{Float64}, Int64, Int64, Ptr{Float64}, Ptr{Int64}),
		c.h, A, n, stride(A, 2), Lout, info))
	return Lout
end

# ---- RandMatFact ------------------------------------------------------------------------------------
module RandMatFact
import Random
import ..DeviceOperator, ..libgsi, ..check, ..ctx

"`rangefinder(A, l::Int64, numiterations::Int64)`  (RandMatFact.jl:50-80)"
function rangefinder(A::DeviceOperator, l::Int64, numiterations::Int64)
	Omega = randn(A.n, l)                                                            # RandMatFact.jl:54
	Q = Matrix{Float64}(undef, A.m, l)
	check(ccall((:gsi_rangefinder, libgsi), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}, Int64, Int64, Ptr{Float64}),
		A.c.h, A.h, Omega, l, numiterations, Q))
	return Q
end
"The same for a host `Matrix{Float64}`: uploaded in row blocks, the sketch `A * Omega` (RandMatFact.jl:55) runs under the upload."
function rangefinder(A::Matrix{Float64}, l::Int64, numiterations::Int64; c=ctx())
	m, n = size(A)
	Omega = randn(n, l)                                                              # RandMatFact.jl:54
	Q = Matrix{Float64}(undef, m, l)
	check(ccall((:gsi_rangefinder_dense_host, libgsi), Cint,
		(Ptr{Cvoid}, Ptr{Float64}, Int64, Int64, Int64, Ptr{Float64}, Int64, Int64, Ptr{Float64}, Ptr{Cvoid}),
		c.h, A, m, n, stride(A, 2), Omega, l, numiterations, Q, C_NULL))
	return Q
end

"`rangefinder(A; epsilon=1e-8, r=10)`  (RandMatFact.jl:15-48): the library pulls Julia's randn stream through a callback."
function rangefinder(A::Matrix{Float64}; epsilon=1e-8, r=10)
	op = DeviceOperator(A)
	fill!(_user::Ptr{Cvoid}, buf::Ptr{Float64}, count::Int64) = (Random.randn!(unsafe_wrap(Array, buf, count)); nothing)
	cb = @cfunction($fill!, Cvoid, (Ptr{Cvoid}, Ptr{Float64}, Int64))
	Q = Matrix{Float64}(undef, op.m, min(op.m, op.n))
	ncols = Ref{Int64}(0)
	GC.@preserve cb check(ccall((:gsi_rangefinder_adaptive, libgsi), Cint,
		(Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Float64, Int64, Ptr{Float64}, Ref{Int64}),
		op.c.h, op.h, cb, C_NULL, epsilon, r, Q, ncols))
	return Q[:, 1:ncols[]]
end

"`randsvd(A, K::Int, p::Int, q::Int)`  (RandMatFact.jl:83-90)"
function randsvd(A::DeviceOperator, K::Int, p::Int, q::Int)
	Omega = randn(A.n, K + p)                                                        # drawn inside rangefinder in the reference
	Z = Matrix{Float64}(undef, A.n, K + p)
	check(ccall((:gsi_randsvd, libgsi), Cint,
		(Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}, Int64, Int64, Int64, Ptr{Float64}, Ptr{Float64}),
		A.c.h, A.h, Omega, K, p, q, Z, C_NULL))
	return Z
end
"`randsvd(Q::Matrix, numxis, p, q)` as `getxis(Q::Matrix, ...)` calls it (GeostatInversion.jl:63-70 -> :20-27): the matrix is
still on the host; it is uploaded in row blocks through the library's pinned staging ring and the first pass runs under the upload."
function randsvd(A::Matrix{Float64}, K::Int, p::Int, q::Int; c=ctx())
	m, n = size(A)
	Omega = randn(n, K + p)
	Z = Matrix{Float64}(undef, n, K + p)
	check(ccall((:gsi_randsvd_dense_host, libgsi), Cint,
		(Ptr{Cvoid}, Ptr{Float64}, Int64, Int64, Int64, Ptr{Float64}, Int64, Int64, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Cvoid}),
		c.h, A, m, n, stride(A, 2), Omega, K, p, q, Z, C_NULL, C_NULL))
	return Z
end

"`eig_nystrom(A, Q)`  (RandMatFact.jl:92-102)"
function eig_nystrom(A::Matrix{Float64}, Q::Matrix{Float64})
	op = DeviceOperator(A)
	j = size(Q, 2)
	U = Matrix{Float64}(undef, op.m, j)
	Sigmavec = Vector{Float64}(undef, j)
	check(ccall((:gsi_eig_nystrom, libgsi), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}, Int64, Ptr{Float64}, Ptr{Float64}),
		op.c.h, op.h, Q, j, U, Sigmavec))
	return U, Sigmavec
end
end # module RandMatFact

# ---- panel primitives: what the reference takes from LinearAlgebra (RandMatFact.jl:57-61, 86) ----------------------
"`LinearAlgebra.lu(Y).L` in pivoted row order (`gsi_lu_L`): returns (L, p) with p the 1-based LAPACK pivot rows."
function lu_L(Y::Matrix{Float64}; c::Context=ctx())
	m, l = size(Y)
	Lout = Matrix{Float64}(undef, m, l)
	piv = Vector{Int32}(undef, l)
	check(ccall((:gsi_lu_L, libgsi), Cint, (Ptr{Cvoid}, Ptr{Float64}, Int64, Int64, Ptr{Float64}, Ptr{Int32}),
		c.h, Y, m, l, Lout, piv))
	return Lout, piv .+ Int32(1)
end
"`lu(Y).L` of a device-resident panel, in place (`gsi_lu_L_dev`): returns the 1-based pivot rows."
function lu_L!(Y::DeviceMatrix)
	piv = Vector{Int32}(undef, Y.cols)
	check(ccall((:gsi_lu_L_dev, libgsi), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Int32}), Y.c.h, Y.h, piv))
	return piv .+ Int32(1)
end
"`Matrix(qr(Y, Val(true)).Q)` up to an orthogonal change of basis (`gsi_qr_thinQ`): returns (Q, R) with Y = Q R."
function qr_thinQ(Y::Matrix{Float64}; c::Context=ctx())
	m, l = size(Y)
	Q = Matrix{Float64}(undef, m, l)
	R = Matrix{Float64}(undef, l, l)
	check(ccall((:gsi_qr_thinQ, libgsi), Cint, (Ptr{Cvoid}, Ptr{Float64}, Int64, Int64, Ptr{Float64}, Ptr{Float64}),
		c.h, Y, m, l, Q, R))
	return Q, R
end
"(S, V) of `svd(W')` for a tall W (`gsi_svd_tall`): what RandMatFact.jl:86 takes from `svd(B)`."
function svd_tall(W::Matrix{Float64}; c::Context=ctx())
	n, l = size(W)
	V = Matrix{Float64}(undef, n, l)
	S = Vector{Float64}(undef, l)
	check(ccall((:gsi_svd_tall, libgsi), Cint, (Ptr{Cvoid}, Ptr{Float64}, Int64, Int64, Ptr{Float64}, Ptr{Float64}),
		c.h, W, n, l, V, S))
	return S, V
end

# ---- getxis (GeostatInversion.jl:20-70) ---------------------------------------------------------------
randsvdwithseed(Q, numxis, p, q, seed::Nothing) = RandMatFact.randsvd(Q, numxis, p, q)
function randsvdwithseed(Q, numxis, p, q, seed::Int)
	Random.seed!(seed)                                                               # GeostatInversion.jl:25
	return RandMatFact.randsvd(Q, numxis, p, q)
end

# columns of Z as the reference's Vector{Vector{Float64}}
xis_from(Z::Matrix{Float64}, numxis::Int) = [Z[:, i] for i in 1:numxis]

function getxis(::Type{Val{:iwantfields}}, samplefield::Function, numfields::Int, numxis::Int, p::Int, q::Int=3, seed=nothing)
	# sampling fans out over the workers like the reference's RobustPmap.rpmap (GeostatInversion.jl:30)
	fields = convert(Vector{Vector{Float64}}, Distributed.pmap(i->samplefield(), 1:numfields))
	Z = randsvdwithseed(LowRankCovMatrix(fields), numxis, p, q, seed)                 # :31-32
	return xis_from(Z, numxis), fields
end

getxis(samplefield::Function, numfields::Int, numxis::Int, p::Int, q::Int=3, seed=nothing) =
	first(getxis(Val{:iwantfields}, samplefield, numfields, numxis, p, q, seed))      # :58-61

getxis(Q::Matrix, numxis::Int, p::Int, q::Int=3, seed=nothing) =
	xis_from(randsvdwithseed(convert(Matrix{Float64}, Q), numxis, p, q, seed), numxis)   # :63-70

"`getxis` whose result stays in HBM: a `DeviceBasis` for the `pcgadirect` / `pcgalsqr` methods below."
function getxis_device(A::DeviceOperator, numxis::Int, p::Int, q::Int=3, seed=nothing; precision::Int=64)
	seed === nothing || Random.seed!(seed)
	Omega = DeviceMatrix(randn(A.n, numxis + p); c=A.c)
	Z = DeviceMatrix(A.n, numxis + p; c=A.c)
	check(ccall((:gsi_randsvd_dev, libgsi), Cint,
		(Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64, Int64, Ptr{Cvoid}, Ptr{Cvoid}),
		A.c.h, A.h, Omega.h, numxis, p, q, Z.h, C_NULL))
	return DeviceBasis(Z, numxis; precision=precision)
end

"`randsvd` with ROW-SHARDED panels over the ranks of `A.c`'s communicator (`gsi_randsvd_rows`): `Omega_rows` = this rank's rows
of Omega (`nloc x (K+p)`, the block layout `row0 = rank*ceil(n/nranks)`); returns this rank's rows of Z as a `DeviceMatrix`
-- nothing n x (K+p) is gathered for LowRankCovMatrix / FFT operators -- and S.  `DeviceBasis(Zrows, K)` over the result is a
row-sharded xi-basis: `paramstorun` / `update` then act on this rank's rows of s and X."
function randsvd_rows(A::DeviceOperator, Omega_rows::Matrix{Float64}, K::Int, p::Int, q::Int)
	Om = DeviceMatrix(Omega_rows; c=A.c)
	Z = DeviceMatrix(size(Omega_rows, 1), K + p; c=A.c)
	S = DeviceMatrix(K + p, 1; c=A.c)
	check(ccall((:gsi_randsvd_rows, libgsi), Cint,
		(Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64, Int64, Ptr{Cvoid}, Ptr{Cvoid}),
		A.c.h, A.h, Om.h, K, p, q, Z.h, S.h))
	Sh = Matrix{Float64}(undef, K + p, 1)
	check(ccall((:gsi_mat_download, libgsi), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}, Int64), A.c.h, S.h, Sh, K + p))
	return Z, vec(Sh)
end

# ---- pcgadirect / pcgalsqr with a device-resident basis (same positional / keyword shape as direct.jl:21, lsqr.jl:20) ----
function iterationhead(forwardmodel::Function, s::Vector, X::Vector, xis::DeviceBasis, delta)
	K = length(xis)
	P = paramstorun(xis, s, X, delta)                                                   # direct.jl:39-45
	results = Distributed.pmap(i->forwardmodel(P[:, i]), 1:K + 3)                       # :46
	hs = results[K + 3]
	etas = hcat([(results[i] - hs) / delta for i in 1:K]...)                            # :49-50
	HX = (results[K + 1] - hs) / delta
	Hs = (results[K + 2] - hs) / delta
	return etas, HX, Hs, hs
end

function headfromresults(results::Matrix{Float64}, K::Int, delta)
	hs = results[:, K + 3]
	etas = (results[:, 1:K] .- hs) ./ delta
	return etas, (results[:, K + 1] - hs) / delta, (results[:, K + 2] - hs) / delta, hs
end
iterationhead(f::LinearForwardModel, s::Vector, X::Vector, xis::DeviceBasis, delta) =
	headfromresults(forward(xis, f, s, X, delta), length(xis), delta)
iterationhead(r::ReducedForwardModel, s::Vector, X::Vector, xis::DeviceBasis, delta) =
	headfromresults(r.S * forward(xis, r.fwd, s, X, delta), length(xis), delta)

"Iterations of the last `pcgadirect(...; solver=:cholesky)` call that fell back to the pseudo-inverse."
const last_fallbacks = Ref(0)
"`pcgadirect(...; solver=:pinv)` as the reference (direct.jl:21-67); `solver=:cholesky` solves the saddle-point system on the
device (`solve(::PCGALowRankMatrix, b)`).  Through `rga`: `rga(...; pcgafunc=pcgadirect, solver=:cholesky)` (keywords are passed on)."
function pcgadirect(forwardmodel::Union{Function, DeviceForwardModel}, s0::Vector, X::Vector, xis::DeviceBasis, R, y::Vector;
		maxiters::Int=5, delta::Float64=sqrt(eps(Float64)), xtol::Float64=1e-6, callback=(s, obs_cal)->nothing,
		solver::Symbol=:pinv)
	solver in (:pinv, :cholesky) || error("solver must be :pinv or :cholesky")
	s, converged, iters = s0, false, 0
	last_fallbacks[] = 0
	while !converged && iters < maxiters
		etas, HX, Hs, hs = iterationhead(forwardmodel, s, X, xis, delta)
		callback(s, hs)
		b = [y - hs + Hs; 0.0]                                                          # direct.jl:56
		x = nothing
		if solver == :cholesky                # Cholesky of HQH + R on the device; a failed iteration falls back to pinv
			try
				x = solve(PCGALowRankMatrix(etas, HX, R; c=xis.Z.c), b)
			catch e
				(e isa LinearAlgebra.PosDefException || e isa LinearAlgebra.SingularException) || rethrow()
				last_fallbacks[] += 1
			end
		end
		if x === nothing
			bigA = [(etas * etas' + R) HX; transpose(HX) 0.0]                           # direct.jl:57
			x = LinearAlgebra.pinv(Matrix(bigA)) * b                                    # :58
		end
		snew = update(xis, X, x[end], etas, x[1:end - 1])                                # :59-65
		converged = LinearAlgebra.norm(snew - s) < xtol
		s = snew
		iters += 1
	end
	return s
end

function pcgalsqr(forwardmodel::Union{Function, DeviceForwardModel}, s0::Vector, X::Vector, xis::DeviceBasis, R, y::Vector;
		maxiters::Int=5, delta::Float64=sqrt(eps(Float64)), xtol::Float64=1e-6)
	s, converged, iters = s0, false, 0
	while !converged && iters < maxiters
		etas, HX, Hs, hs = iterationhead(forwardmodel, s, X, xis, delta)
		x = lsqr(PCGALowRankMatrix(etas, HX, R; c=xis.Z.c), [y - hs + Hs; 0.0])         # lsqr.jl:52-54
		snew = update(xis, X, x[end], etas, x[1:end - 1])                                # :55-61
		converged = LinearAlgebra.norm(snew - s) < xtol
		s = snew
		iters += 1
	end
	return s
end

const pcga = pcgadirect                                                                  # GeostatInversion.jl:105

"`(a, q, t)` over the rows z_i of the basis in one pass on the device: a[i] = |W' z_i|^2, q[i] = |z_i|^2, t[i] = u' z_i
(`gsi_basis_quadform`).  `upper = true` promises W[k, j] = 0 for k > j: those entries are not read."
function quadform(b::DeviceBasis, W::Matrix{Float64}, u::Vector{Float64}; upper::Bool=false)
	a, q, t = Vector{Float64}(undef, b.n), Vector{Float64}(undef, b.n), Vector{Float64}(undef, b.n)
	info = zeros(Int64, 2)
	check(ccall((:gsi_basis_quadform, libgsi), Cint,
		(Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}, Int64, Int64, Cint, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int64}),
		b.Z.c.h, b.h, W, stride(W, 2), size(W, 2), upper ? 1 : 0, u, a, q, t, info))
	return a, q, t
end
"`(W, u, gamma)` of the posterior covariance Z W W' Z' + d d' / gamma, d = Z u - X (`gsi_pcgamat_posterior`)."
function posteriorfactor(A::PCGALowRankMatrix, K::Int)
	W, u, gamma = Matrix{Float64}(undef, K, K), Vector{Float64}(undef, K), Ref{Float64}(0.0)
	info = zeros(Int64, 2)
	check(ccall((:gsi_pcgamat_posterior, libgsi), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int64}),
		A.c.h, A.h, W, u, gamma, info))
	return W, u, gamma[]
end
"The posterior variance of the field at the linearisation point `s`, for the prior s ~ N(X beta, Z Z') with beta unknown and
the error covariance R: v_i = |W' z_i|^2 + (u' z_i - X_i)^2 / gamma, plus priorvariance_i - |z_i|^2 when the true prior
variances are given.  One pass over the resident basis on the device (`gsi_pcga_posterior_variance`)."
function posteriorvariance(forwardmodel::Union{Function, DeviceForwardModel}, s::Vector, X::Vector, xis::DeviceBasis, R;
		delta::Float64=sqrt(eps(Float64)), priorvariance::Union{Nothing, Vector{Float64}}=nothing)
	etas, HX, Hs, hs = iterationhead(forwardmodel, s, X, xis, delta)
	A = PCGALowRankMatrix(etas, HX, R; c=xis.Z.c)
	v = Vector{Float64}(undef, xis.n)
	info = zeros(Int64, 2)
	check(ccall((:gsi_pcga_posterior_variance, libgsi), Cint,
		(Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int64}),
		xis.Z.c.h, xis.h, A.h, X, priorvariance === nothing ? C_NULL : priorvariance, v, info))
	return v
end

"`rga(forwardmodel, s0, X, xis, R, y, S; ...)`  (GeostatInversion.jl:101-103)"
rga(forwardmodel::Function, s0::Vector, X::Vector, xis::DeviceBasis, R, y::Vector, S; pcgafunc=pcgadirect, kwargs...) =
	pcgafunc(x->S * forwardmodel(x), s0, X, xis, S * R * S', S * y; kwargs...)
rga(forwardmodel::LinearForwardModel, s0::Vector, X::Vector, xis::DeviceBasis, R, y::Vector, S; pcgafunc=pcgadirect, kwargs...) =
	pcgafunc(ReducedForwardModel(forwardmodel, Matrix{Float64}(S)), s0, X, xis, S * R * S', S * y; kwargs...)

end # module
