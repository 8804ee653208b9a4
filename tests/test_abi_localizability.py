"""CPU-only checks of include/localizability/o3s_localizability.h: both libraries export exactly what the header declares, the header
compiles as C, and the calls refuse bad arguments before any device work (so without a device too) without touching their outputs."""
import ctypes as C
import os
import subprocess

import numpy as np

from open3d_slam_advanced_rss_2024_public_amd import _lib
from open3d_slam_advanced_rss_2024_public_amd import localizability as loc
from test_abi import ROOT, declared_symbols

HEADER = os.path.join("localizability", "o3s_localizability.h")


def test_both_libraries_export_exactly_the_declared_symbols():
    _lib.build()
    syms = declared_symbols([HEADER])
    assert syms == ["o3s_icp_localizability", "o3s_localizability_default_params", "o3s_localizability_estimate", "o3s_localizability_remap"]
    for variant in (None, "hooks"):
        L = _lib.load(variant)
        for s in syms:
            assert hasattr(L, s), (variant, s)
        out = subprocess.run(["nm", "-D", "--defined-only", _lib.variant_path(variant)], capture_output=True, text=True, check=True).stdout
        exported = sorted(ln.split()[-1] for ln in out.splitlines() if "localizability" in ln.split()[-1] and " T " in ln)
        assert exported == syms, (variant, exported)


def test_header_compiles_as_c(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "localizability/o3s_localizability.h"\n'
                   "int use(o3s_icp* h, const float* p, const float* n, const double* Tp, const double* Ti, double* To) {\n"
                   "  o3s_localizability_params q;\n  o3s_localizability r;\n  int32_t k;\n"
                   "  o3s_localizability_default_params(&q);\n"
                   "  if (o3s_icp_localizability(h, &q, &r)) return 1;\n"
                   "  if (o3s_localizability_estimate(h, p, n, 7, &q, &r)) return 2;\n"
                   "  return o3s_localizability_remap(&r, 1, Tp, Ti, To, &k) + (int)sizeof(q) + (int)sizeof(r);\n}\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I" + os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "use.o")])


def test_struct_layouts():
    assert C.sizeof(loc.LocalizabilityParamsC) == 40
    assert C.sizeof(loc.LocalizabilityC) == 8 * (6 + 18 + 6 + 6 + 6) + 24 + 8 + 24 + 8
    assert loc.LocalizabilityC.kept.offset == 8 * 42 + 24 and loc.LocalizabilityC.gpu_ms.offset == 8 * 42 + 24 + 8 + 24
    assert C.sizeof(_lib.IcpConfigC) == 80                                   # the parameters go by call: the configuration is as it was
    c = _lib.IcpConfigC()
    _lib.lib().o3s_icp_default_config(C.byref(c))
    assert list(c.reserved) == [0, 0]


def _params(**kw):
    p = loc.LocalizabilityParams(sum_all_min=100.0, sum_strong_min=50.0, sum_partial_min=10.0)
    for k, v in kw.items():
        setattr(p, k, v)
    return p.to_c()


BAD_PARAMS = [dict(sum_all_min=float("nan")), dict(sum_strong_min=float("nan")), dict(sum_partial_min=float("nan")),      # unset
              dict(sum_all_min=float("inf")), dict(sum_all_min=40.0), dict(sum_partial_min=60.0), dict(sum_partial_min=-1.0),   # unordered
              dict(filter_min=-0.1), dict(filter_min=0.9), dict(strong_min=1.5), dict(filter_min=float("nan")), dict(strong_min=float("nan"))]


def test_bad_arguments_are_refused_before_any_device_work():
    L = loc._L()
    # a NULL handle (a machine without a device cannot create a real one)
    out = loc.LocalizabilityC()
    C.memset(C.byref(out), 0x5A, C.sizeof(out))
    before = bytes(out)
    good = _params()
    p3 = np.zeros((4, 3), np.float32)
    fp = p3.ctypes.data_as(C.POINTER(C.c_float))
    assert L.o3s_icp_localizability(None, C.byref(good), C.byref(out)) == _lib.ERR_BAD_ARGUMENT
    assert L.o3s_localizability_estimate(None, fp, fp, 4, C.byref(good), C.byref(out)) == _lib.ERR_BAD_ARGUMENT
    assert bytes(out) == before
    # the remap: no handle at all
    dp = C.POINTER(C.c_double)
    I = np.eye(4).reshape(16)
    To = np.full(16, 7.0)
    n = C.c_int32(-5)
    r = loc.Localizability().to_c()
    i_, o_ = I.ctypes.data_as(dp), To.ctypes.data_as(dp)
    for min_cat in (0, 3, -1, 2 ** 31 - 1):
        assert L.o3s_localizability_remap(C.byref(r), min_cat, i_, i_, o_, C.byref(n)) == _lib.ERR_BAD_ARGUMENT
    assert L.o3s_localizability_remap(None, 1, i_, i_, o_, C.byref(n)) == _lib.ERR_BAD_ARGUMENT
    assert L.o3s_localizability_remap(C.byref(r), 1, None, i_, o_, C.byref(n)) == _lib.ERR_BAD_ARGUMENT
    assert L.o3s_localizability_remap(C.byref(r), 1, i_, None, o_, C.byref(n)) == _lib.ERR_BAD_ARGUMENT
    assert L.o3s_localizability_remap(C.byref(r), 1, i_, i_, None, C.byref(n)) == _lib.ERR_BAD_ARGUMENT
    assert n.value == -5 and (To == 7.0).all()
    assert L.o3s_localizability_remap(C.byref(r), 1, i_, i_, o_, None) == _lib.OK and np.array_equal(To, I)   # n_replaced is optional
    L.o3s_localizability_default_params(None)   # nothing to write to: returns


def test_unset_and_unordered_thresholds_are_refused_before_the_handle_is_looked_at():
    """The parameters are checked first, so the refusal needs no device: O3S_ERR_BAD_CONFIG even on a NULL handle, outputs untouched."""
    L = loc._L()
    out = loc.LocalizabilityC()
    C.memset(C.byref(out), 0x5A, C.sizeof(out))
    before = bytes(out)
    p3 = np.zeros((4, 3), np.float32)
    fp = p3.ctypes.data_as(C.POINTER(C.c_float))
    d = loc.default_params().to_c()   # the defaults leave the three sums unset
    assert L.o3s_icp_localizability(None, C.byref(d), C.byref(out)) == _lib.ERR_BAD_CONFIG
    for kw in BAD_PARAMS:
        p = _params(**kw)
        assert L.o3s_icp_localizability(None, C.byref(p), C.byref(out)) == _lib.ERR_BAD_CONFIG, kw
        assert L.o3s_localizability_estimate(None, fp, fp, 4, C.byref(p), C.byref(out)) == _lib.ERR_BAD_CONFIG, kw
    good = _params()
    for args in ((None, C.byref(out)), (C.byref(good), None)):
        assert L.o3s_icp_localizability(None, *args) == _lib.ERR_BAD_ARGUMENT
        assert L.o3s_localizability_estimate(None, fp, fp, 4, *args) == _lib.ERR_BAD_ARGUMENT
    assert L.o3s_localizability_estimate(None, None, fp, 4, C.byref(good), C.byref(out)) == _lib.ERR_BAD_ARGUMENT
    assert L.o3s_localizability_estimate(None, fp, None, 4, C.byref(good), C.byref(out)) == _lib.ERR_BAD_ARGUMENT
    assert bytes(out) == before
    for ok in (dict(sum_all_min=50.0), dict(sum_partial_min=0.0), dict(filter_min=0.0, strong_min=1.0), dict(filter_min=0.5, strong_min=0.5)):   # the edges hold
        p = _params(**ok)
        assert L.o3s_icp_localizability(None, C.byref(p), C.byref(out)) == _lib.ERR_BAD_ARGUMENT, ok   # ... so only the NULL handle is left to refuse
