"""CPU-only checks of include/constraints/o3s_constraints.h: the library exports what the header declares, the header compiles as
C, and the call refuses bad arguments before any device work (so without a device too) without touching its outputs."""
import ctypes as C
import os
import subprocess

import numpy as np

from open3d_slam_advanced_rss_2024_public_amd import _lib
from open3d_slam_advanced_rss_2024_public_amd import constraint_builders as cb
from test_abi import ROOT, declared_symbols


def test_library_exports_the_declared_symbol():
    _lib.build()
    syms = declared_symbols([os.path.join("constraints", "o3s_constraints.h")])
    assert syms == ["o3s_submaps_odometry_constraints"]
    for L in (_lib.lib(), _lib.load("hooks")):
        assert hasattr(L, syms[0])


def test_header_compiles_as_c(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "constraints/o3s_constraints.h"\n'
                   "int use(const o3s_submap* const* s, double* infos, int32_t* st) {\n"
                   "  return o3s_submaps_odometry_constraints(1, s, s, 0, 3.0, 1, 0.2, infos, 0, 0, st);\n}\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I" + os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "use.o")])


def test_bad_arguments_are_refused_before_any_device_work():
    L = cb._L()
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    null = (C.c_void_p * 1)(None)
    info, st = np.full(36, 7.0), np.full(1, -5, np.int32)
    i_, s_ = info.ctypes.data_as(dp), st.ctypes.data_as(ip)
    f = L.o3s_submaps_odometry_constraints
    assert f(0, None, None, None, 3.0, 1, 0.2, None, None, None, None) == _lib.OK                 # n == 0 needs nothing
    assert f(-1, null, null, None, 3.0, 1, 0.2, i_, None, None, s_) == _lib.ERR_BAD_ARGUMENT
    assert f(1, None, null, None, 3.0, 1, 0.2, i_, None, None, s_) == _lib.ERR_BAD_ARGUMENT      # NULL arrays with n > 0
    assert f(1, null, None, None, 3.0, 1, 0.2, i_, None, None, s_) == _lib.ERR_BAD_ARGUMENT
    assert f(1, null, null, None, 3.0, 1, 0.2, None, None, None, s_) == _lib.ERR_BAD_ARGUMENT
    assert f(1, null, null, None, 3.0, 1, 0.2, i_, None, None, None) == _lib.ERR_BAD_ARGUMENT
    assert f(1, null, null, None, 3.0, 1, 0.2, i_, None, None, s_) == _lib.ERR_BAD_ARGUMENT      # a NULL submap
    for voxel, min_pts, dist in ((0.0, 1, 0.2), (-1.0, 1, 0.2), (float("nan"), 1, 0.2), (3.0, 0, 0.2), (3.0, 1, 0.0), (3.0, 1, float("nan")),
                                 (3.0, 1, float("inf")), (3.0, 1, 3.0 * 2.0 ** -21)):
        assert f(0, None, None, None, voxel, min_pts, dist, None, None, None, None) == _lib.ERR_BAD_ARGUMENT, (voxel, min_pts, dist)
    assert st[0] == -5 and (info == 7.0).all()
