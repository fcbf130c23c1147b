"""The circulant-embedding sampler for grid covariance functions (gsi_gridcov_sampler_*), without a GPU:

  * header, ctypes table and Julia shim carry the six symbols; the Python entry points are exported;
  * the argument checks of api.cpp through the CPU reference build of the same C ABI: every bad argument is status 1
    (GSI_ERR_ARG) with a message that names it, a valid call ends in the backend's "not supported by this backend", and
    nothing stays allocated;
  * the numpy model of the contract (tests/gridcov_sample_model.py) against the dense matrix of gsi_op_fft_gridcov, by
    impulses: the fields of the noise (e_k, 0), k < Mtot, have F F' = the covariance of the sampler's fields;
  * the case list of the GPU tests reaches every instantiation of the line kernel.
"""
import ctypes as C

import numpy as np
import pytest

import cpuref
import gridcov_sample_model as gm
from test_binding_signatures_static import JULIA_FILES, header_prototypes, julia_ccalls

NEW = ("gsi_gridcov_sampler_create", "gsi_gridcov_sampler_info", "gsi_gridcov_sampler_spectrum", "gsi_gridcov_sampler_destroy",
       "gsi_gridcov_fields", "gsi_op_lowrank_gridcov")


# ---------------------------------------------------------------- the three statements of the boundary
def test_header_ctypes_and_julia_shim_carry_the_new_symbols(gsi):
    protos = header_prototypes()
    bound = {c["name"] for c in julia_ccalls(JULIA_FILES[0])}
    for name in NEW:
        assert name in protos, name
        assert name in gsi._lib.SIGNATURES, name
        assert name in bound, f"{name} is not bound in the Julia shim"
    assert protos["gsi_gridcov_sampler_create"] == ("i32", ["ptr", "ptr", "i32", "ptr", "ptr", "i32", "ptr", "f64", "f64", "f64",
                                                            "f64", "ptr"])
    assert protos["gsi_gridcov_fields"] == ("i32", ["ptr", "ptr", "ptr", "ptr", "i64", "u64", "i64"])
    assert protos["gsi_op_lowrank_gridcov"] == ("i32", ["ptr", "ptr", "ptr", "i64", "u64", "i64", "i64"])
    for name in ("gridcov_sampler", "lowrank_gridcov_operator"):
        assert name in gsi.__all__ and callable(getattr(gsi, name)), name
    assert gsi._lib.load is not None and gsi.load().gsi_version() == 100


# ---------------------------------------------------------------- argument checks (api.cpp on the CPU reference backend)
@pytest.fixture(scope="module")
def cx(gsi):
    lib = cpuref.load_cpuref()
    assert lib.gsi_backend_name().startswith(b"cpu-reference")
    c = gsi.Context(0, lib=lib)
    yield c
    c.close()


def _err(gsi, fn):
    with pytest.raises(gsi.GsiError) as ei:
        fn()
    assert ei.value.code == 1, ei.value
    return str(ei.value)


@pytest.mark.parametrize("kwargs,word", [
    (dict(Ns=[8]), "ndims"),
    (dict(Ns=[4, 5, 6, 7]), "ndims"),
    (dict(Ns=[4, 0]), "N[a]"),
    (dict(Ns=[1, 1]), "n = prod(N)"),
    (dict(Ns=[8, 6], embed=[24, 16]), "embed[a] must be a power of two"),
    (dict(Ns=[8, 6], embed=[16, 8]), "embed[a] must be >= 2 N[a]"),
    (dict(Ns=[8, 6], embed=[16384, 16]), "embed[a] must be <= 8192"),
    (dict(Ns=[5000, 6]), "embed[a]"),
    (dict(Ns=[8, 1 << 40]), "embed[a]"),
    (dict(Ns=[512, 512, 512], embed=[2048, 1024, 1024]), "Mtot"),
    (dict(Ns=[8, 6], kind=4), "kind"),
    (dict(Ns=[8, 6], kind=-1), "kind"),
    (dict(Ns=[8, 6], ell=0.0), "ell"),
    (dict(Ns=[8, 6], ell=[2.0, float("nan")]), "ell"),
    (dict(Ns=[8, 6], ell=float("inf")), "ell"),
    (dict(Ns=[8, 6], sigma2=0.0), "sigma2"),
    (dict(Ns=[8, 6], sigma2=float("inf")), "sigma2"),
    (dict(Ns=[8, 6], nugget=-1e-3), "nugget"),
    (dict(Ns=[8, 6], nugget=float("nan")), "nugget"),
    (dict(Ns=[8, 6], theta=float("nan")), "theta"),
    (dict(Ns=[4, 5, 6], theta=0.3), "theta"),
    (dict(Ns=[8, 6], neg_tol=-1e-3), "neg_tol"),
    (dict(Ns=[8, 6], neg_tol=1.5), "neg_tol"),
    (dict(Ns=[8, 6], neg_tol=float("nan")), "neg_tol"),
])
def test_bad_arguments_are_refused_by_name(gsi, cx, kwargs, word):
    before = cx.device_bytes()
    msg = _err(gsi, lambda: gsi.gridcov_sampler(cx, **kwargs))
    assert word in msg, msg
    assert "not supported by this backend" not in msg
    assert cx.device_bytes() == before


def test_null_pointers_are_refused_by_name(gsi, cx):
    lib = cx.lib
    h = C.c_void_p()
    N = (C.c_int64 * 2)(8, 6)
    ell = (C.c_double * 2)(2.0, 2.0)
    assert lib.gsi_gridcov_sampler_create(cx.h, C.byref(h), 2, None, None, 1, ell, 0.0, 1.0, 0.0, 1e-12, None) == 1
    assert b"N is NULL" in lib.gsi_last_error()
    assert lib.gsi_gridcov_sampler_create(cx.h, C.byref(h), 2, N, None, 1, None, 0.0, 1.0, 0.0, 1e-12, None) == 1
    assert b"ell is NULL" in lib.gsi_last_error()
    assert lib.gsi_gridcov_sampler_create(cx.h, None, 2, N, None, 1, ell, 0.0, 1.0, 0.0, 1e-12, None) == 1
    assert b"sampler is NULL" in lib.gsi_last_error()
    assert not h.value
    F = gsi.DeviceMatrix(cx, 48, 2)
    assert lib.gsi_gridcov_fields(cx.h, None, F.h, None, 0, 0, 0) == 1
    assert b"sampler is NULL" in lib.gsi_last_error()
    assert lib.gsi_op_lowrank_gridcov(cx.h, C.byref(h), None, 8, 0, 0, 48) == 1
    assert b"sampler is NULL" in lib.gsi_last_error()
    assert lib.gsi_gridcov_sampler_spectrum(cx.h, None, None) == 1
    assert lib.gsi_gridcov_sampler_info(None, None, None) == 1
    assert b"sampler is NULL" in lib.gsi_last_error()
    assert lib.gsi_gridcov_sampler_destroy(None) == 0
    F.close()
    with pytest.raises(ValueError):
        gsi.gridcov_sampler(cx, [8, 6], ell=[1.0, 2.0, 3.0])
    with pytest.raises(ValueError):
        gsi.gridcov_sampler(cx, [8, 6], embed=[16, 16, 16])


def test_valid_calls_reach_the_backend_which_does_not_have_the_sampler(gsi, cx):
    before = cx.device_bytes()
    info = (C.c_double * 4)(1.0, 2.0, 3.0, 4.0)
    for kw in (dict(Ns=[8, 6], kind="matern52", ell=[2.0, 3.0], theta=0.6, sigma2=1.7, nugget=0.01),
               dict(Ns=[9, 6, 11], kind=0, ell=2.0), dict(Ns=[8, 6], embed=[32, 16], neg_tol=0.0),
               dict(Ns=[8, 6], embed="auto"), dict(Ns=[1, 2]), dict(Ns=[4096, 2], neg_tol=1.0)):
        assert "not supported by this backend" in _err(gsi, lambda: gsi.gridcov_sampler(cx, **kw))
    h = C.c_void_p()
    N = (C.c_int64 * 2)(8, 6)
    ell = (C.c_double * 2)(2.0, 2.0)
    assert cx.lib.gsi_gridcov_sampler_create(cx.h, C.byref(h), 2, N, None, 1, ell, 0.0, 1.0, 0.0, 1e-12, info) == 1
    assert not h.value and all(np.isnan(v) for v in info), "no spectrum was computed: info says so"
    assert cx.device_bytes() == before


# ---------------------------------------------------------------- the model against the dense matrix
def _impulse_error(c, lam=None):
    lam = gm.spectrum(c) if lam is None else lam
    F = gm.fields_from_eps(lam, c.N, gm.impulse_eps(lam.size))
    return F @ F.T - gm.dense_cov(c)


@pytest.mark.parametrize("c", gm.EXACT_CASES, ids=[gm.case_id(c) for c in gm.EXACT_CASES])
def test_model_fields_have_the_dense_covariance(c):
    lam = gm.spectrum(c)
    assert gm.neg_mass(c, lam) == 0.0
    err = np.abs(_impulse_error(c, lam)).max() / (c.sigma2 + c.nugget)
    print(gm.case_id(c), err)
    assert err <= gm.COV_BAR


def test_the_clamp_bound_is_attained_on_the_diagonal():
    c = gm.BOUND_CASE
    lam = gm.spectrum(c)
    nm = gm.neg_mass(c, lam)
    assert abs(nm - gm.BOUND_NEG_MASS) <= 5e-8, nm
    E = _impulse_error(c, lam)
    assert abs(np.abs(E).max() / c.sigma2 - nm) <= 1e-12
    assert abs(np.abs(np.diag(E)).max() / c.sigma2 - nm) <= 1e-12


@pytest.mark.parametrize("c", gm.DEFAULT_CASES, ids=[gm.case_id(c) for c in gm.DEFAULT_CASES])
def test_the_default_embedding_carries_these(c):
    if c.N in gm.DEFAULT_EMBEDS:
        assert c.M == gm.DEFAULT_EMBEDS[c.N]
    assert gm.neg_mass(c, gm.spectrum(c)) == 0.0


def test_this_one_is_not_carried_below_512():
    for m, want in gm.NOT_CARRIED_NEG_MASS.items():
        c = gm.NOT_CARRIED._replace(M=(m, m))
        nm = gm.neg_mass(c, gm.spectrum(c))
        print(m, nm)
        assert (nm == 0.0) if want == 0.0 else abs(nm - want) <= 0.005 * want, (m, nm)
    assert gm.NOT_CARRIED.M == (64, 64)


def test_the_gpu_cases_reach_every_instantiation():
    seen = set()
    for c in gm.GPU_CASES:
        seen.update(gm.pass_instantiations(c))
    assert seen == gm.ALL_INSTANTIATIONS and len(seen) == 21, sorted(gm.ALL_INSTANTIATIONS - seen)
    for c in gm.TRANSFORM_CASES:
        assert all(2 * n <= m for n, m in zip(c.N, c.M)) and int(np.prod(c.M)) <= 1 << 19
