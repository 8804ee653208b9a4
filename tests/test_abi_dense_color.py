"""CPU-only checks of include/dense_map/o3s_dense_map_color.h: the header compiles as strict C99, both libraries export every symbol it
declares, and the calls refuse NULL / negative arguments before any device work (so without a device too)."""
import ctypes as C
import os
import subprocess

import numpy as np

from open3d_slam_advanced_rss_2024_public_amd import _lib
from open3d_slam_advanced_rss_2024_public_amd import cloud_ops as co
from open3d_slam_advanced_rss_2024_public_amd import dense_map as dm
from test_abi import ROOT, declared_symbols

HEADER = os.path.join("dense_map", "o3s_dense_map_color.h")
SYMBOLS = ["o3s_color_range_crop", "o3s_dense_map_capacity", "o3s_dense_map_has_colors", "o3s_dense_map_insert_colored",
           "o3s_dense_map_insert_resident_scan_colored", "o3s_dense_map_insert_scan_colored", "o3s_dense_map_to_point_cloud_colored"]


def test_both_libraries_export_every_declared_symbol():
    _lib.build()
    assert declared_symbols([HEADER]) == SYMBOLS
    for variant in (None, "hooks"):
        L = _lib.load(variant)
        out = subprocess.run(["nm", "-D", "--defined-only", _lib.variant_path(variant)], capture_output=True, text=True, check=True).stdout
        exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
        for s in SYMBOLS:
            assert hasattr(L, s) and s in exported, (variant, s)


def test_header_compiles_as_strict_c99(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "dense_map/o3s_dense_map_color.h"\n'
                   "int use(o3s_dense_map* m, const o3s_cropper* c, const o3s_scan* sc, const double* p, double* o, const double* T,\n"
                   "        const o3s_dense_carving_params* cp, int32_t* k) {\n"
                   "  int64_t n = 0;\n  const double lo[3] = {0.0, 0.0, 0.0}, hi[3] = {1.0, 1.0, 1.0};\n"
                   "  if (o3s_color_range_crop(0, lo, hi, p, p, p, p, 4, o, o, o, o, &n)) return 1;\n"
                   "  if (o3s_dense_map_insert_colored(m, p, p, p, 4)) return 2;\n"
                   "  if (o3s_dense_map_insert_scan_colored(m, c, lo, hi, p, p, p, 4, T, cp, &n)) return 3;\n"
                   "  if (o3s_dense_map_insert_resident_scan_colored(m, c, lo, hi, sc, p, 4, T, cp, &n)) return 4;\n"
                   "  if (o3s_dense_map_to_point_cloud_colored(m, o, o, o, k, k, &n)) return 5;\n"
                   "  return o3s_dense_map_has_colors(m) + (int)o3s_dense_map_capacity(m);\n}\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c", str(src),
                           "-o", str(tmp_path / "use.o")])


def test_cpp_shim_offers_the_coloured_overloads_beside_the_old_calls(tmp_path):
    """o3s::DenseMapHip (cpp/o3s_icp.hpp): the coloured overloads resolve, and the calls a host wrote before them still do."""
    src = tmp_path / "shim.cpp"
    src.write_text('#include "o3s_icp.hpp"\n'
                   "std::int64_t use(o3s::DenseMapHip& dm, const o3s_cropper& c, const o3s_scan* sc, const double* p, double* o, std::int64_t N,\n"
                   "                 const o3s_dense_carving_params* cp) {\n"
                   "  const double lo[3] = {0.0, 0.0, 0.0}, hi[3] = {1.0, 1.0, 1.0};\n"
                   "  dm.insert(p, p, N);\n  dm.insert(p, nullptr, p, N);\n"
                   "  std::int64_t r = dm.insertScanDenseMap(c, p, p, N, p, cp) + dm.insertScanDenseMap(c, p, p, N, p);\n"
                   "  r += dm.insertScanDenseMap(c, p, p, p, N, p) + dm.insertScanDenseMap(c, p, nullptr, p, N, p, cp, lo, hi);\n"
                   "  r += dm.insertResidentScanDenseMap(c, sc, p, N, p, cp) + dm.insertResidentScanDenseMap(c, sc, p, N, p, cp, lo, hi);\n"
                   "  return r + dm.toPointCloud(o, o) + dm.toPointCloud(o, o, dm.hasColors() ? o : nullptr);\n}\n")
    pkg = os.path.join(ROOT, "open3d_slam_advanced_rss_2024_public_amd")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(pkg, "cpp"), str(src)])


def test_null_and_negative_arguments_are_refused_without_a_device():
    L = dm._L()
    co._L()
    dp = C.POINTER(C.c_double)
    L.o3s_color_range_crop.argtypes = [C.c_int, dp, dp, dp, dp, dp, dp, C.c_int64, dp, dp, dp, dp, C.POINTER(C.c_int64)]
    a = np.zeros((4, 3))
    cov = np.zeros((4, 9))
    o = np.full((4, 3), 7.0)
    ocov = np.full((4, 9), 7.0)
    d = lambda x: x.ctypes.data_as(dp)
    n = C.c_int64(-5)
    BAD = _lib.ERR_BAD_ARGUMENT
    # o3s_color_range_crop: points, their output and the count are required; an optional input needs its output; N >= 0
    assert L.o3s_color_range_crop(0, None, None, None, None, d(a), None, 4, d(o), None, d(o), None, C.byref(n)) == BAD
    assert L.o3s_color_range_crop(0, None, None, d(a), None, d(a), None, 4, None, None, d(o), None, C.byref(n)) == BAD
    assert L.o3s_color_range_crop(0, None, None, d(a), None, d(a), None, 4, d(o), None, d(o), None, None) == BAD
    assert L.o3s_color_range_crop(0, None, None, d(a), None, d(a), None, -1, d(o), None, d(o), None, C.byref(n)) == BAD
    assert L.o3s_color_range_crop(0, None, None, d(a), d(a), d(a), None, 4, d(o), None, d(o), None, C.byref(n)) == BAD
    assert L.o3s_color_range_crop(0, None, None, d(a), None, d(a), None, 4, d(o), None, None, None, C.byref(n)) == BAD
    assert L.o3s_color_range_crop(0, None, None, d(a), None, d(a), d(cov), 4, d(o), None, d(o), None, C.byref(n)) == BAD
    assert n.value == -5 and (o == 7.0).all()
    # an empty cloud, and a cloud without colours (returned unchanged: a copy), need no device either
    assert L.o3s_color_range_crop(0, None, None, d(a), None, d(a), None, 0, d(o), None, d(o), None, C.byref(n)) == _lib.OK and n.value == 0
    src, srcn = np.arange(12.0).reshape(4, 3), np.arange(12.0).reshape(4, 3) + 50.0
    srcv = np.arange(36.0).reshape(4, 9)
    on = np.full((4, 3), 7.0)
    assert L.o3s_color_range_crop(0, None, None, d(src), d(srcn), None, d(srcv), 4, d(o), d(on), None, d(ocov), C.byref(n)) == _lib.OK
    assert n.value == 4 and np.array_equal(o, src) and np.array_equal(on, srcn) and np.array_equal(ocov, srcv)
    # the map entries: a NULL handle, and what they check before the handle's device is touched
    crop = co.croppingVolumeFactory("MaxRadius", 5.0)
    T = np.eye(4).reshape(16)
    removed = C.c_int64(-5)
    assert L.o3s_dense_map_has_colors(None) == 0 and L.o3s_dense_map_capacity(None) == 0
    assert L.o3s_dense_map_insert_colored(None, d(a), None, d(a), 4) == BAD
    assert L.o3s_dense_map_insert_colored(None, None, None, None, 0) == BAD
    assert L.o3s_dense_map_insert_scan_colored(None, C.byref(crop), None, None, d(a), None, d(a), 4, d(T), None, C.byref(removed)) == BAD
    assert removed.value == 0                                                     # n_removed is cleared first, as by o3s_dense_map_insert_scan
    assert L.o3s_dense_map_insert_scan_colored(None, None, None, None, None, None, None, -1, None, None, None) == BAD
    assert L.o3s_dense_map_insert_resident_scan_colored(None, C.byref(crop), None, None, None, d(a), 4, d(T), None, None) == BAD
    assert L.o3s_dense_map_to_point_cloud_colored(None, d(o), None, d(o), None, None, C.byref(n)) == BAD and n.value == 0


def test_python_entry_refuses_a_colour_array_of_another_length():
    """DenseMap.insert / insertScanDenseMap check the colour shape on the host (the C entries take one N for all arrays)."""
    class Stub(dm.DenseMap):
        def __init__(self):
            pass

        def __del__(self):
            pass

    import pytest

    with pytest.raises(ValueError):
        Stub().insert(np.zeros((4, 3)), None, np.zeros((3, 3)))
    with pytest.raises(ValueError):
        Stub().insertScanDenseMap(np.zeros((4, 3)), np.eye(4), co.croppingVolumeFactory("MaxRadius", 5.0), raw_colors=np.zeros((5, 3)))
