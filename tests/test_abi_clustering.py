"""CPU-only checks of include/clustering/o3s_clustering.h: the library exports what the header declares, the header compiles as C,
the calls refuse bad arguments before any device work (so without a device too) without touching their outputs, and
min_points 0 is O3S_OK with nothing touched."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from open3d_slam_advanced_rss_2024_public_amd import _lib
from open3d_slam_advanced_rss_2024_public_amd import cloud_ops as co
from test_abi import ROOT, declared_symbols

HEADER = os.path.join("clustering", "o3s_clustering.h")
SYMBOLS = ["o3s_cluster_dbscan", "o3s_remove_small_clusters", "o3s_scan_remove_small_clusters", "o3s_submap_cluster_dbscan",
           "o3s_submap_remove_small_clusters"]


def test_library_exports_the_declared_symbols():
    _lib.build()
    syms = declared_symbols([HEADER])
    assert syms == SYMBOLS
    for L in (_lib.lib(), _lib.load("hooks")):
        for s in syms:
            assert hasattr(L, s), s


def test_header_compiles_as_c(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "clustering/o3s_clustering.h"\n'
                   "int use(o3s_submap* m, o3s_scan* s, const o3s_cropper* c, const double* p, double* o, int64_t* n, int32_t* l) {\n"
                   "  o3s_dbscan_params q; q.eps = 0.5; q.min_points = 10; q.min_cluster_size = 50;\n"
                   "  return o3s_cluster_dbscan(0, &q, p, 4, l, l, 0) + o3s_remove_small_clusters(0, &q, p, 0, 4, o, 0, 0, n, l, 0)\n"
                   "       + o3s_submap_cluster_dbscan(m, &q, l, l) + o3s_submap_remove_small_clusters(m, &q, n, 0)\n"
                   "       + o3s_scan_remove_small_clusters(s, c, &q, n, n);\n}\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I" + os.path.join(ROOT, "include"), "-c", str(src),
                           "-o", str(tmp_path / "use.o")])


def test_params_struct_layout():
    assert C.sizeof(co.DbscanParamsC) == 16
    assert (co.DbscanParamsC.eps.offset, co.DbscanParamsC.min_points.offset, co.DbscanParamsC.min_cluster_size.offset) == (0, 8, 12)
    p = co.dbscan_params(0.5, 10, 50)
    assert (p.eps, p.min_points, p.min_cluster_size) == (0.5, 10, 50)
    z = co.dbscan_params()
    assert bytes(z) == bytes(16)   # off is the zeroed struct


# (eps, min_points, min_cluster_size)
BAD = [(0.5, -1, 0), (0.5, -2 ** 31, 0), (0.0, 3, 0), (-0.5, 3, 0), (float("nan"), 3, 0), (float("inf"), 3, 0), (-float("inf"), 3, 0),
       (0.5, 3, -1), (0.5, 3, -2 ** 31)]


def _fns():
    L = co._L()
    fns = [L.o3s_cluster_dbscan, L.o3s_remove_small_clusters, L.o3s_submap_cluster_dbscan, L.o3s_submap_remove_small_clusters,
           L.o3s_scan_remove_small_clusters]
    for fn in fns:
        fn.restype = C.c_int
        fn.argtypes = None
    return fns


def _host_args(N=4):
    dp, lp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_int32)
    pts = np.arange(3.0 * N).reshape(N, 3)
    out = np.full((N, 3), 7.0)
    idx = np.full(N, -5, np.int64)
    lab = np.full(N, 9, np.int32)
    siz = np.full(N, 11, np.int32)
    n = C.c_int64(-77)
    nc = C.c_int32(-78)
    return dp, lp, ip, pts, out, idx, lab, siz, n, nc


def _untouched(out, idx, lab, siz, n, nc):
    return n.value == -77 and nc.value == -78 and (out == 7.0).all() and (idx == -5).all() and (lab == 9).all() and (siz == 11).all()


@pytest.mark.parametrize("eps,min_points,min_cluster_size", BAD)
def test_bad_parameters_are_refused_before_any_device_work(eps, min_points, min_cluster_size):
    f, g, sc, sr, h = _fns()
    dp, lp, ip, pts, out, idx, lab, siz, n, nc = _host_args()
    q = co.DbscanParamsC(eps, min_points, min_cluster_size)
    assert f(0, C.byref(q), pts.ctypes.data_as(dp), C.c_int64(4), lab.ctypes.data_as(ip), C.byref(nc), siz.ctypes.data_as(ip)) == _lib.ERR_BAD_ARGUMENT
    assert g(0, C.byref(q), pts.ctypes.data_as(dp), None, C.c_int64(4), out.ctypes.data_as(dp), None, idx.ctypes.data_as(lp), C.byref(n),
             lab.ctypes.data_as(ip), C.byref(nc)) == _lib.ERR_BAD_ARGUMENT
    assert _untouched(out, idx, lab, siz, n, nc)
    # the resident entries check the parameters before they look at the handle's device: a handle that could not be read ...
    fake = C.c_void_p(8)
    assert sc(fake, C.byref(q), lab.ctypes.data_as(ip), C.byref(nc)) == _lib.ERR_BAD_ARGUMENT
    assert sr(fake, C.byref(q), C.byref(n), C.byref(nc)) == _lib.ERR_BAD_ARGUMENT
    assert h(fake, fake, C.byref(q), C.byref(n), C.byref(n)) == _lib.ERR_BAD_ARGUMENT
    assert _untouched(out, idx, lab, siz, n, nc)
    # ... and a NULL one
    assert sc(None, C.byref(q), None, None) == _lib.ERR_BAD_ARGUMENT
    assert sr(None, C.byref(q), None, None) == _lib.ERR_BAD_ARGUMENT
    assert h(None, None, C.byref(q), None, None) == _lib.ERR_BAD_ARGUMENT


def test_bad_pointers_and_sizes_are_refused():
    f, g, sc, sr, h = _fns()
    dp, lp, ip, pts, out, idx, lab, siz, n, nc = _host_args()
    q = co.DbscanParamsC(0.5, 3, 0)
    P, O, Lb = pts.ctypes.data_as(dp), out.ctypes.data_as(dp), lab.ctypes.data_as(ip)
    bad = _lib.ERR_BAD_ARGUMENT
    assert f(0, None, P, C.c_int64(4), Lb, C.byref(nc), None) == bad
    assert f(0, C.byref(q), None, C.c_int64(4), Lb, C.byref(nc), None) == bad
    assert f(0, C.byref(q), P, C.c_int64(4), None, C.byref(nc), None) == bad
    assert f(0, C.byref(q), P, C.c_int64(4), Lb, None, None) == bad
    assert f(0, C.byref(q), P, C.c_int64(-1), Lb, C.byref(nc), None) == bad
    assert f(0, C.byref(q), P, C.c_int64(2 ** 31), Lb, C.byref(nc), None) == bad
    assert g(0, None, P, None, C.c_int64(4), O, None, None, C.byref(n), None, None) == bad
    assert g(0, C.byref(q), None, None, C.c_int64(4), O, None, None, C.byref(n), None, None) == bad
    assert g(0, C.byref(q), P, None, C.c_int64(4), None, None, None, C.byref(n), None, None) == bad
    assert g(0, C.byref(q), P, None, C.c_int64(4), O, None, None, None, None, None) == bad
    assert g(0, C.byref(q), P, P, C.c_int64(4), O, None, None, C.byref(n), None, None) == bad   # normals in, nowhere to put them
    assert g(0, C.byref(q), P, None, C.c_int64(-1), O, None, None, C.byref(n), None, None) == bad
    assert g(0, C.byref(q), P, None, C.c_int64(2 ** 31), O, None, None, C.byref(n), None, None) == bad
    assert h(C.c_void_p(8), None, C.byref(q), None, None) == bad   # no cropper
    assert sc(C.c_void_p(8), None, None, None) == bad and sr(C.c_void_p(8), None, None, None) == bad
    assert _untouched(out, idx, lab, siz, n, nc)


def test_off_and_empty_clouds_need_no_device():
    """min_points 0: O3S_OK, nothing touched, nothing launched — on a machine without a GPU too, and with pointers that could not be
    read.  N == 0 with real parameters: O3S_OK, n_clusters = 0 and n_out = 0, also before any device call."""
    f, g, sc, sr, h = _fns()
    dp, lp, ip, pts, out, idx, lab, siz, n, nc = _host_args()
    q = co.DbscanParamsC(float("nan"), 0, -9)   # the other fields mean nothing with min_points 0
    assert f(0, C.byref(q), None, C.c_int64(4), None, None, None) == _lib.OK
    assert f(99, C.byref(q), pts.ctypes.data_as(dp), C.c_int64(4), lab.ctypes.data_as(ip), C.byref(nc), siz.ctypes.data_as(ip)) == _lib.OK
    assert g(0, C.byref(q), None, None, C.c_int64(4), None, None, None, None, None, None) == _lib.OK
    assert g(99, C.byref(q), pts.ctypes.data_as(dp), None, C.c_int64(4), out.ctypes.data_as(dp), None, idx.ctypes.data_as(lp), C.byref(n),
             lab.ctypes.data_as(ip), C.byref(nc)) == _lib.OK
    fake = C.c_void_p(8)   # never dereferenced
    assert sc(fake, C.byref(q), lab.ctypes.data_as(ip), C.byref(nc)) == _lib.OK
    assert sr(fake, C.byref(q), C.byref(n), C.byref(nc)) == _lib.OK
    assert h(fake, None, C.byref(q), C.byref(n), C.byref(n)) == _lib.OK
    assert _untouched(out, idx, lab, siz, n, nc)
    assert sc(None, C.byref(q), None, None) == _lib.ERR_BAD_ARGUMENT and sr(None, C.byref(q), None, None) == _lib.ERR_BAD_ARGUMENT
    assert h(None, None, C.byref(q), None, None) == _lib.ERR_BAD_ARGUMENT
    q = co.DbscanParamsC(0.5, 3, 2)
    assert f(99, C.byref(q), None, C.c_int64(0), None, C.byref(nc), None) == _lib.OK and nc.value == 0
    nc.value = -78
    assert g(99, C.byref(q), None, None, C.c_int64(0), None, None, None, C.byref(n), None, C.byref(nc)) == _lib.OK
    assert n.value == 0 and nc.value == 0
    # the Python entry points on an empty cloud
    lab0, k0, s0 = co.cluster_dbscan(np.zeros((0, 3)), 0.5, 3)
    assert len(lab0) == 0 and k0 == 0 and len(s0) == 0
    op, on, ix, lb = co.remove_small_clusters(np.zeros((0, 3)), 0.5, 3, 2)
    assert len(op) == 0 and on is None and len(ix) == 0 and len(lb) == 0
