"""The sparse forward model (gsi_fwd, LinearForwardModel) without a GPU: argument checking, the
host path of pcga.cpp on the CPU reference backend against numpy, the counters, pcgadirect / pcgalsqr / rga end to end,
and the segment planner as a stand-alone program under the address and undefined-behaviour sanitizers."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import cpuref
import fwd_cases as fc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cx(gsi):
    lib = cpuref.load_cpuref()
    assert lib.gsi_backend_name().startswith(b"cpu-reference")
    c = gsi.Context(0, lib=lib)
    yield c
    c.close()


def _create(gsi, cx, nobs, n, indptr, indices, data, weights=None, link=0, ctx_handle=None):
    p64 = C.POINTER(C.c_int64)
    indptr = np.ascontiguousarray(indptr, dtype=np.int64)
    indices = np.ascontiguousarray(indices, dtype=np.int64)
    data = np.ascontiguousarray(data, dtype=np.float64)
    h = C.c_void_p()
    st = cx.lib.gsi_fwd_linear_create(ctx_handle or cx.h, C.byref(h), nobs, n, indptr.ctypes.data_as(p64),
                                      indices.ctypes.data_as(p64), gsi._lib.dptr(data),
                                      gsi._lib.dptr(weights) if weights is not None else None, link)
    return st, h, (cx.lib.gsi_last_error() or b"").decode()


GOOD = dict(nobs=2, n=5, indptr=[0, 2, 3], indices=[4, 0, 2], data=[1.0, 2.0, 3.0])


@pytest.mark.parametrize("change,word", [
    (dict(nobs=0, indptr=[0]), "nobs"),
    (dict(n=0), "n = 0"),
    (dict(n=2 ** 31), "2^31"),
    (dict(indptr=[1, 2, 3]), "rowptr[0]"),
    (dict(indptr=[0, 2, 1]), "row 1"),
    (dict(indices=[4, 5, 2]), "entry 1"),
    (dict(indices=[4, 0, -1]), "entry 2"),
    (dict(link=2), "link"),
])
def test_create_refuses_bad_arguments(gsi, cx, change, word):
    args = dict(GOOD, **change)
    st, h, msg = _create(gsi, cx, **args)
    assert st == 1 and not h.value
    assert msg and word in msg, msg
    st, h, _ = _create(gsi, cx, **GOOD)                     # a valid create after a refused one works
    assert st == 0 and h.value
    out = (C.c_int64 * 10)(*([-1] * 10))
    assert cx.lib.gsi_fwd_info(h, out, 10) == 0
    assert list(out) == [2, 5, 3, 2, 0, 0, 0, 0, 0, 0]
    assert cx.lib.gsi_fwd_destroy(h) == 0


def test_handles_of_another_context_and_size_mismatch(gsi, cx):
    other = gsi.Context(0, lib=cx.lib)
    try:
        fwd_other = gsi.LinearForwardModel((GOOD["indptr"], GOOD["indices"], GOOD["data"], (2, 5)), ctx=other)
        fwd_small = gsi.LinearForwardModel((GOOD["indptr"], GOOD["indices"], GOOD["data"], (2, 5)), ctx=cx)
        basis = gsi.DeviceBasis(gsi.DeviceMatrix.from_host(cx, np.ones((7, 3))), 2)
        basis5 = gsi.DeviceBasis(gsi.DeviceMatrix.from_host(cx, np.ones((5, 3))), 2)
        s = np.zeros(7)
        out = np.empty((2, 5), order="F")
        dp = gsi._lib.dptr
        st = cx.lib.gsi_pcga_forward_basis(cx.h, basis5.h, fwd_other.h, dp(s), dp(s), 0.5, dp(out))
        assert st == 1 and b"another context" in cx.lib.gsi_last_error()
        st = cx.lib.gsi_pcga_forward_basis(cx.h, basis.h, fwd_small.h, dp(s), dp(s), 0.5, dp(out))
        assert st == 1 and b"n = 5" in cx.lib.gsi_last_error() and b"n = 7" in cx.lib.gsi_last_error()
        P = np.zeros((5, 1), order="F")
        st = cx.lib.gsi_fwd_apply(cx.h, fwd_other.h, dp(P), 5, 1, dp(out), 2)
        assert st == 1 and b"another context" in cx.lib.gsi_last_error()
        with pytest.raises(ValueError):
            basis5.forward(fwd_other, np.zeros(5), np.zeros(5), 0.5)
        got = basis5.forward(fwd_small, np.zeros(5), np.zeros(5), 0.5)   # and the valid call still works
        assert got.shape == (2, 5)
    finally:
        other.close()


def _basis(gsi, ctx, case, precision):
    Zmat = gsi.DeviceMatrix.from_host(ctx, case["Z"])
    basis = gsi.DeviceBasis(Zmat, case["K"], precision=precision)
    Zs = np.stack([basis[i] for i in range(case["K"])], axis=1)    # the stored (fp32: rounded) columns
    return basis, Zs


@pytest.mark.parametrize("precision", [64, 32])
@pytest.mark.parametrize("link", [0, 1])
def test_forward_basis_against_numpy(gsi, cx, link, precision):
    case = fc.product_case(37, link)
    fwd = gsi.LinearForwardModel((case["indptr"], case["indices"], case["data"], (case["nobs"], case["n"])),
                                 weights=case["w"], link="exp" if link else "identity", ctx=cx)
    basis, Zs = _basis(gsi, cx, case, precision)
    if precision == 32:
        assert np.array_equal(Zs, case["Z"][:, :37].astype(np.float32).astype(np.float64))
    got = basis.forward(fwd, case["s"], case["X"], case["delta"])
    ratio = fc.check_product(got, case, Zs)
    print(f"link {link} precision {precision}: largest error / bound = {ratio:.3g}")
    info = fwd.info()
    assert info[:3] == [case["nobs"], case["n"], int(case["indptr"][-1])]
    assert info[5] == 3 and info[6] == info[7] == 1            # the CPU library has the host path only
    # the model as an ordinary callable, and on a matrix
    one = fwd(case["s"])
    assert np.array_equal(one, fwd.apply(case["s"][:, None])[:, 0])
    assert np.abs(one - got[:, -1]).max() <= 2 * np.asarray(fc.reference(
        case["indptr"], case["indices"], case["data"], case["n"], case["w"], link, case["s"][:, None])[1]).max()
    info = fwd.info()
    assert info[6] == info[7] == 3
    fwd.close()
    basis.close()


def test_no_weights_tuple_and_scipy_inputs_agree(gsi, cx):
    import scipy.sparse as sp
    case = fc.product_case(5, 0)
    shape = (case["nobs"], case["n"])
    H = sp.csr_matrix((case["data"], case["indices"], case["indptr"]), shape=shape)     # scipy keeps duplicates as given
    a = gsi.LinearForwardModel((case["indptr"], case["indices"], case["data"], shape), ctx=cx)
    b = gsi.LinearForwardModel(H.tocoo(), ctx=cx)              # anything with .tocsr()
    assert (a.nobs, a.n, a.nnz) == (shape[0], shape[1], int(case["indptr"][-1]))
    P = np.asfortranarray(case["Z"][:, :3])
    ref, bound = fc.reference(case["indptr"], case["indices"], case["data"], case["n"], None, 0, P)
    assert np.all(np.abs(a.apply(P) - ref) <= bound)
    assert np.all(np.abs(b.apply(P) - ref) <= bound)
    a.close()
    b.close()


@pytest.mark.parametrize("link", [0, 1])
def test_inversions_with_the_model_match_the_host_lambda(gsi, cx, link):
    info, _ = fc.run_inversions(gsi, cx, link)
    assert info[6] == info[7] > 0


def test_plain_callable_takes_the_old_path(gsi, cx):
    """A lambda is never routed to the device entry point, whatever the basis."""
    import sys
    mod = sys.modules["gsi_amd.pcga"]                        # (the package attribute `pcga` is the solver of that name)
    case = fc.product_case(5, 0)
    basis, _ = _basis(gsi, cx, case, 64)
    assert mod._device_forward(lambda x: x, basis) is None
    fwd = gsi.LinearForwardModel((case["indptr"], case["indices"], case["data"], (case["nobs"], case["n"])), ctx=cx)
    assert mod._device_forward(fwd, basis) == (fwd, None)
    assert mod._device_forward(fwd, mod._Basis([case["s"]], cx)) is None
    fwd.close()
    basis.close()


def test_segment_planner_under_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build the planner check"
    exe = str(tmp_path / "fwd_plan_check")
    src = os.path.join(ROOT, "tests", "fwd_plan_check.cpp")
    inc = os.path.join(ROOT, "geostatinversion.jl_amd", "csrc")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", inc, src, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "planner ok" in r.stdout
