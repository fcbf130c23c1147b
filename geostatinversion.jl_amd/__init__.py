"""geostatinversion.jl_amd -- MI355X (gfx950) implementation of the randomized low-rank
factorization hot path of GeostatInversion.jl (RandMatFact.jl reached through getxis()).

Product = libgsi_hip.so (hand-written HIP kernels behind the C ABI of include/gsi_hip.h).
This package is the host-side mirror of the reference's interface for that path -- the same
function names and argument meaning as the Julia module -- and is nothing but ctypes calls
into the library.  Importing it never silently degrades: no library, or no gfx950 GPU, raises.

The directory name contains a dot, so import it through the `gsi_amd` alias at the repo root:
    import gsi_amd as gsi
"""
from . import _lib
from ._lib import GsiError, load, LIB_PATH
from .context import (Context, Operator, DeviceMatrix, dense_operator, gridcov_operator,
                      gridcov_implicit_operator, pointcov_implicit_operator, fft_powerlaw_operator, fft_gridcov_operator, lowrank_synthetic_operator,
                      default_context, fft_gridcov_derivative)
from . import randmatfact as RandMatFact
from .randmatfact import rangefinder, randsvd, randsvd_rows, eig_nystrom, colnorms, lu_L, lu_L_dev, lu_L_sharded, lu_L_sharded_virtual, qr_thinQ, svd_tall, gemm, gemm_view, cq_gram_round, pivoted_cholesky, principal_factor
from .lowrank import LowRankCovMatrix, PCGALowRankMatrix, device_samples
from .getxis import getxis, getxis_iwantfields, getxis_device, getxis_fftrf, getxis_pivchol, randsvdwithseed
from . import fftrf as FFTRF
from .fftrf import lowrank_fftrf_operator, fft_operator_at, FFTOperatorAt
from . import gridcov as GridCov
from .gridcov import GridCovSampler, gridcov_sampler, lowrank_gridcov_operator, gridcov_structuredgrid
from . import kriging as Kriging
from .kriging import (solve, kriging_weights, krige_to_grid, condition_fields, mat_axpy, lowrank_preconditioner,
                      Preconditioner, logdet, log_likelihood, solve_trace, estimate_field, linear_inversion,
                      condition_on_linear_data, posterior_variance_exact, mat_rowdot_acc, mat_bilinear,
                      op_bilinear_terms, log_likelihood_grad, covariance_family, CovarianceFamily, fit_covariance)
from .pcga import (pcgadirect, pcgalsqr, rga, pcga, DeviceBasis, ShardedDeviceBasis, LinearForwardModel, posterior_variance,
                   posterior_realizations, LinearDataOperator, linear_data_operator)

__all__ = [
    "GsiError", "load", "LIB_PATH", "Context", "Operator", "DeviceMatrix", "dense_operator",
    "gridcov_operator", "gridcov_implicit_operator", "pointcov_implicit_operator", "fft_powerlaw_operator", "fft_gridcov_operator", "lowrank_synthetic_operator", "default_context", "RandMatFact", "rangefinder", "randsvd", "randsvd_rows", "eig_nystrom",
    "colnorms", "lu_L", "lu_L_dev", "lu_L_sharded", "lu_L_sharded_virtual", "qr_thinQ", "svd_tall", "gemm", "gemm_view", "cq_gram_round", "LowRankCovMatrix", "PCGALowRankMatrix", "device_samples",
    "getxis", "getxis_iwantfields", "getxis_device", "getxis_fftrf", "randsvdwithseed", "FFTRF", "lowrank_fftrf_operator", "fft_operator_at", "FFTOperatorAt", "GridCov", "GridCovSampler",
    "gridcov_sampler", "lowrank_gridcov_operator", "gridcov_structuredgrid", "pcgadirect", "pcgalsqr", "rga", "pcga",
    "DeviceBasis", "ShardedDeviceBasis", "LinearForwardModel", "posterior_variance", "posterior_realizations",
    "Kriging", "solve", "kriging_weights", "krige_to_grid", "condition_fields", "mat_axpy",
    "lowrank_preconditioner", "Preconditioner", "logdet", "log_likelihood", "solve_trace", "pivoted_cholesky", "principal_factor", "getxis_pivchol",
    "LinearDataOperator", "linear_data_operator", "estimate_field", "linear_inversion", "condition_on_linear_data",
    "posterior_variance_exact", "mat_rowdot_acc",
    "fft_gridcov_derivative", "mat_bilinear", "op_bilinear_terms", "log_likelihood_grad", "covariance_family", "CovarianceFamily",
    "fit_covariance",
]
