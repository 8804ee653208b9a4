"""CPU-only checks of include/plane_segmentation/o3s_plane_segmentation.h: the library and the hooks build export exactly what the
header declares, the header compiles as C, the struct has the documented layout, the calls refuse bad arguments before any device
work (so without a device too) without touching their outputs, and num_iterations 0 and N == 0 need no device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from open3d_slam_advanced_rss_2024_public_amd import _lib
from open3d_slam_advanced_rss_2024_public_amd import cloud_ops as co
from test_abi import ROOT, declared_symbols

HEADER = os.path.join("plane_segmentation", "o3s_plane_segmentation.h")
SYMBOLS = ["o3s_plane_default_params", "o3s_plane_device_bytes", "o3s_plane_evaluate_samples", "o3s_plane_release", "o3s_plane_reserve",
           "o3s_scan_remove_planes", "o3s_segment_plane", "o3s_segment_planes", "o3s_submap_remove_planes", "o3s_submap_segment_planes"]


def test_libraries_export_exactly_the_declared_symbols():
    _lib.build()
    syms = declared_symbols([HEADER])
    assert syms == SYMBOLS
    for variant in (None, "hooks"):
        L = _lib.lib() if variant is None else _lib.load("hooks")
        for s in syms:
            assert hasattr(L, s), s
        nm = subprocess.run(["nm", "-D", "--defined-only", _lib.variant_path(variant)], capture_output=True, text=True, check=True).stdout
        exported = sorted(set(re.findall(r"\b(o3s_[a-z0-9_]*plane[a-z0-9_]*)\b", nm)))
        assert exported == SYMBOLS, exported


def test_header_compiles_as_c(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "plane_segmentation/o3s_plane_segmentation.h"\n'
                   "int use(o3s_submap* m, o3s_scan* s, const o3s_cropper* c, const double* p, double* o, int64_t* n, int32_t* l) {\n"
                   "  o3s_plane_params q; o3s_plane_default_params(&q); q.distance_threshold = 0.1; q.max_planes = 4;\n"
                   "  return o3s_segment_plane(0, &q, p, 9, 0, 0, o, n, n, n, n, n) + o3s_segment_planes(0, &q, p, 9, l, l, o, n)\n"
                   "       + o3s_plane_evaluate_samples(0, &q, p, 9, 0, 0, 4, l, o, n, o) + o3s_submap_segment_planes(m, &q, l, l, o, n)\n"
                   "       + o3s_submap_remove_planes(m, &q, n, l, o) + o3s_scan_remove_planes(s, c, &q, n, n, l, o)\n"
                   "       + o3s_plane_reserve(0, 1000, 100) + o3s_plane_release(0) + (int)o3s_plane_device_bytes(0) + O3S_PLANE_DEGENERATE;\n}\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I" + os.path.join(ROOT, "include"), "-c", str(src),
                           "-o", str(tmp_path / "use.o")])


def test_params_struct_layout_and_defaults():
    P = co.PlaneParamsC
    assert C.sizeof(P) == 40
    assert (P.distance_threshold.offset, P.confidence.offset, P.seed.offset, P.num_iterations.offset, P.ransac_n.offset, P.max_planes.offset,
            P.min_inliers.offset) == (0, 8, 16, 24, 28, 32, 36)
    assert bytes(co.plane_params()) == bytes(40)   # off is the zeroed struct
    q = co.plane_params(0.1, 4, 500, 0.99, 2 ** 40 + 3, 5, 30)
    assert (q.distance_threshold, q.ransac_n, q.num_iterations, q.confidence, q.seed, q.max_planes, q.min_inliers) == (0.1, 4, 500, 0.99, 2 ** 40 + 3, 5, 30)
    d = P(9.0, 9.0, 9, 9, 9, 9, 9)
    fn = co._L().o3s_plane_default_params
    fn.restype, fn.argtypes = None, [C.POINTER(P)]
    fn(C.byref(d))
    assert (d.distance_threshold, d.confidence, d.seed, d.num_iterations, d.ransac_n, d.max_planes, d.min_inliers) == (0.0, 1.0, 0, 100, 3, 1, 3)
    fn(None)
    assert (co.PLANE_PASS, co.PLANE_REPEATED, co.PLANE_NONFINITE, co.PLANE_DEGENERATE) == (0, 1, 2, 3)


def good(**kw):
    v = dict(distance_threshold=0.1, ransac_n=3, num_iterations=10, confidence=1.0, seed=0, max_planes=1, min_inliers=3)
    v.update(kw)
    return co.plane_params(**v)


BAD = [dict(distance_threshold=0.0), dict(distance_threshold=-0.1), dict(distance_threshold=float("nan")), dict(distance_threshold=float("inf")),
       dict(confidence=0.0), dict(confidence=-0.5), dict(confidence=1.0 + 2.0 ** -40), dict(confidence=float("nan")),
       dict(num_iterations=-1), dict(num_iterations=-2 ** 31), dict(ransac_n=2), dict(ransac_n=0), dict(ransac_n=9), dict(ransac_n=-3),
       dict(max_planes=0), dict(max_planes=17), dict(max_planes=-1), dict(min_inliers=-1), dict(min_inliers=-2 ** 31)]


def _fns():
    L = co._L()
    fns = [L.o3s_segment_plane, L.o3s_segment_planes, L.o3s_plane_evaluate_samples, L.o3s_submap_segment_planes, L.o3s_submap_remove_planes,
           L.o3s_scan_remove_planes]
    for fn in fns:
        fn.restype = C.c_int
        fn.argtypes = None
    return fns


class Host:
    """Arguments of the host-array entries over a cloud of N points, with outputs whose every byte is known"""

    def __init__(self, N=9):
        self.N = N
        self.pts = np.arange(3.0 * N).reshape(N, 3)
        self.model = np.full(64, 7.0)
        self.idx = np.full(N, -5, np.int64)
        self.lab = np.full(max(N, 16), 9, np.int32)
        self.cnt = np.full(16, -6, np.int64)
        self.err = np.full(16, 5.0)
        self.n = [C.c_int64(-77) for _ in range(4)]
        self.k = C.c_int32(-78)

    def untouched(self):
        return (all(v.value == -77 for v in self.n) and self.k.value == -78 and (self.model == 7.0).all() and (self.idx == -5).all() and
                (self.lab == 9).all() and (self.cnt == -6).all() and (self.err == 5.0).all())

    def ptr(self):
        dp, lp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_int32)
        return (self.pts.ctypes.data_as(dp), self.model.ctypes.data_as(dp), self.idx.ctypes.data_as(lp), self.lab.ctypes.data_as(ip),
                self.cnt.ctypes.data_as(lp), self.err.ctypes.data_as(dp))

    def call_all(self, q, want, N=None, samples=None, n_samples=0, device=0):
        """the six entries with well-formed pointers (fake handles for the resident ones) must all return `want`"""
        one, many, ev, sseg, srem, scrm = _fns()
        P, M, I, Lb, Ct, E = self.ptr()
        N = C.c_int64(self.N if N is None else N)
        nn = [C.byref(v) for v in self.n]
        fake = C.c_void_p(8)
        rcs = [one(device, C.byref(q), P, N, samples, C.c_int64(n_samples), M, I, *nn),
               many(device, C.byref(q), P, N, Lb, C.byref(self.k), M, Ct),
               ev(device, C.byref(q), P, N, samples, C.c_int64(0), C.c_int64(n_samples or 4), Lb, M, Ct, E)]
        if samples is None:
            rcs += [sseg(fake, C.byref(q), Lb, C.byref(self.k), M, Ct), srem(fake, C.byref(q), nn[0], C.byref(self.k), M),
                    scrm(fake, fake, C.byref(q), nn[0], nn[1], C.byref(self.k), M)]
        assert rcs == [want] * len(rcs), rcs


@pytest.mark.parametrize("kw", BAD, ids=lambda kw: "%s=%r" % next(iter(kw.items())))
def test_bad_parameters_are_refused_before_any_device_work(kw):
    h = Host()
    q = good(**kw)
    h.call_all(q, _lib.ERR_BAD_ARGUMENT)       # the resident entries: before they look at the handle (it could not be read)
    assert h.untouched()
    _, _, _, sseg, srem, scrm = _fns()
    assert sseg(None, C.byref(q), None, None, None, None) == _lib.ERR_BAD_ARGUMENT
    assert srem(None, C.byref(q), None, None, None) == _lib.ERR_BAD_ARGUMENT
    assert scrm(None, None, C.byref(q), None, None, None, None) == _lib.ERR_BAD_ARGUMENT


def test_bad_sizes_tables_and_pointers_are_refused():
    h = Host()
    one, many, ev, sseg, srem, scrm = _fns()
    P, M, I, Lb, Ct, E = h.ptr()
    nn = [C.byref(v) for v in h.n]
    bad = _lib.ERR_BAD_ARGUMENT
    q = good()
    for N in (-1, 2 ** 31, 2 ** 40):
        assert one(0, C.byref(q), P, C.c_int64(N), None, C.c_int64(0), M, I, *nn) == bad
        assert many(0, C.byref(q), P, C.c_int64(N), Lb, C.byref(h.k), M, Ct) == bad
        assert ev(0, C.byref(q), P, C.c_int64(N), None, C.c_int64(0), C.c_int64(4), Lb, M, Ct, E) == bad
    ip = C.POINTER(C.c_int32)
    ok_rows = np.array([[0, 1, 2], [3, 4, 8]], np.int32)
    for rows in ([[0, 1, 9], [3, 4, 5]], [[0, 1, 2], [-1, 4, 5]], [[0, 1, 2], [3, 4, 2 ** 31 - 1]]):   # an index outside [0, N)
        t = np.array(rows, np.int32)
        assert one(0, C.byref(q), P, C.c_int64(9), t.ctypes.data_as(ip), C.c_int64(2), M, I, *nn) == bad
        assert ev(0, C.byref(q), P, C.c_int64(9), t.ctypes.data_as(ip), C.c_int64(0), C.c_int64(2), Lb, M, Ct, E) == bad
    q4 = good(max_planes=4)                                                                             # a table with a peel
    assert one(0, C.byref(q4), P, C.c_int64(9), ok_rows.ctypes.data_as(ip), C.c_int64(2), M, I, *nn) == bad
    assert ev(0, C.byref(q4), P, C.c_int64(9), ok_rows.ctypes.data_as(ip), C.c_int64(0), C.c_int64(2), Lb, M, Ct, E) == bad
    assert one(0, C.byref(q), P, C.c_int64(9), ok_rows.ctypes.data_as(ip), C.c_int64(-1), M, I, *nn) == bad
    assert ev(0, C.byref(q), P, C.c_int64(9), ok_rows.ctypes.data_as(ip), C.c_int64(1), C.c_int64(1), Lb, M, Ct, E) == bad   # a table starts at row 0
    assert ev(0, C.byref(q), P, C.c_int64(9), None, C.c_int64(-1), C.c_int64(2), Lb, M, Ct, E) == bad
    assert ev(0, C.byref(q), P, C.c_int64(9), None, C.c_int64(0), C.c_int64(-2), Lb, M, Ct, E) == bad
    assert ev(0, C.byref(q), P, C.c_int64(2), None, C.c_int64(0), C.c_int64(2), Lb, M, Ct, E) == bad                        # N < ransac_n
    # pointers
    assert one(0, None, P, C.c_int64(9), None, C.c_int64(0), M, I, *nn) == bad
    assert one(0, C.byref(q), None, C.c_int64(9), None, C.c_int64(0), M, I, *nn) == bad
    assert one(0, C.byref(q), P, C.c_int64(9), None, C.c_int64(0), None, I, *nn) == bad
    assert many(0, None, P, C.c_int64(9), Lb, C.byref(h.k), M, Ct) == bad
    assert many(0, C.byref(q), None, C.c_int64(9), Lb, C.byref(h.k), M, Ct) == bad
    assert many(0, C.byref(q), P, C.c_int64(9), None, C.byref(h.k), M, Ct) == bad
    assert many(0, C.byref(q), P, C.c_int64(9), Lb, None, M, Ct) == bad
    assert many(0, C.byref(q), P, C.c_int64(9), Lb, C.byref(h.k), None, Ct) == bad
    assert ev(0, None, P, C.c_int64(9), None, C.c_int64(0), C.c_int64(2), Lb, M, Ct, E) == bad
    assert ev(0, C.byref(q), None, C.c_int64(9), None, C.c_int64(0), C.c_int64(2), Lb, M, Ct, E) == bad
    assert ev(0, C.byref(q), P, C.c_int64(9), None, C.c_int64(0), C.c_int64(2), None, M, Ct, E) == bad
    fake = C.c_void_p(8)
    assert sseg(fake, None, Lb, C.byref(h.k), M, Ct) == bad and srem(fake, None, None, None, None) == bad
    assert sseg(fake, C.byref(q), Lb, None, M, Ct) == bad and sseg(fake, C.byref(q), Lb, C.byref(h.k), None, Ct) == bad
    assert scrm(fake, None, C.byref(q), None, None, None, None) == bad   # no cropper
    assert scrm(fake, fake, None, None, None, None, None) == bad
    rs = co._L().o3s_plane_reserve
    rs.restype, rs.argtypes = C.c_int, [C.c_int, C.c_int64, C.c_int32]
    assert rs(0, -1, 100) == bad and rs(0, 2 ** 31, 100) == bad and rs(0, 1000, -1) == bad
    assert h.untouched()


def test_off_and_empty_clouds_need_no_device():
    """num_iterations 0: O3S_OK, nothing touched, nothing launched — on a machine without a GPU too, with a device that does not exist
    and pointers that could not be read.  N == 0 (and N < ransac_n) with real parameters: O3S_OK with empty results, also before any
    device call."""
    h = Host()
    q = co.plane_params(float("nan"), -9, 0, 7.0, 0, -9, -9)   # the other fields mean nothing with num_iterations 0
    h.call_all(q, _lib.OK, device=99)
    assert h.untouched()
    one, many, ev, sseg, srem, scrm = _fns()
    fake = C.c_void_p(8)   # never dereferenced
    assert one(99, C.byref(q), None, C.c_int64(9), None, C.c_int64(0), None, None, None, None, None, None) == _lib.OK
    assert many(99, C.byref(q), None, C.c_int64(9), None, None, None, None) == _lib.OK
    assert ev(99, C.byref(q), None, C.c_int64(9), None, C.c_int64(0), C.c_int64(4), None, None, None, None) == _lib.OK
    assert sseg(fake, C.byref(q), None, None, None, None) == _lib.OK and srem(fake, C.byref(q), None, None, None) == _lib.OK
    assert scrm(fake, None, C.byref(q), None, None, None, None) == _lib.OK
    assert sseg(None, C.byref(q), None, None, None, None) == _lib.ERR_BAD_ARGUMENT and srem(None, C.byref(q), None, None, None) == _lib.ERR_BAD_ARGUMENT
    assert scrm(None, None, C.byref(q), None, None, None, None) == _lib.ERR_BAD_ARGUMENT
    # empty and too-small clouds
    q = good(max_planes=3)
    P, M, I, Lb, Ct, E = h.ptr()
    nn = [C.byref(v) for v in h.n]
    for N, pts in ((0, None), (2, P)):
        h2 = Host()
        P2, M2, I2, Lb2, Ct2, E2 = h2.ptr()
        nn2 = [C.byref(v) for v in h2.n]
        assert one(99, C.byref(q), pts and P2, C.c_int64(N), None, C.c_int64(0), M2, I2, *nn2) == _lib.OK
        assert [v.value for v in h2.n] == [0, -1, 10, 0] and not h2.model[:4].any() and (h2.model[4:] == 7.0).all() and (h2.idx == -5).all()
    assert many(99, C.byref(q), None, C.c_int64(0), None, C.byref(h.k), M, Ct) == _lib.OK and h.k.value == 0
    assert ev(99, C.byref(q), P, C.c_int64(9), None, C.c_int64(0), C.c_int64(0), Lb, M, Ct, E) == _lib.OK   # no hypotheses
    # the Python entry points on an empty cloud
    r = co.segment_plane(np.zeros((0, 3)), 0.1, device=99)
    model, inliers = r
    assert not model.any() and len(inliers) == 0 and (r.best_iteration, r.est_k, r.evaluated) == (-1, 100, 0)
    lab, models, counts = co.segment_planes(np.zeros((0, 3)), 0.1, 4, device=99)
    assert len(lab) == 0 and models.shape == (0, 4) and len(counts) == 0
    assert co.plane_device_bytes(0) >= 0 and co.plane_device_bytes(-1) == 0 and co.plane_device_bytes(10 ** 6) == 0


def test_cpp_case_compiles_and_links_with_plain_gxx(tmp_path):
    """tests/cpp/plane_segmentation_case.cpp (run by tests/test_gpu_plane_segmentation_cpp.py) builds against the shim and the C-ABI
    library alone — no HIP header, no Eigen — without a warning, and a run without a case file ends with its usage status."""
    pkg = os.path.join(ROOT, "open3d_slam_advanced_rss_2024_public_amd")
    exe = tmp_path / "plane_segmentation_case"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-pthread", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(pkg, "cpp"), os.path.join(ROOT, "tests", "cpp", "plane_segmentation_case.cpp"), "-L" + pkg,
                           "-lo3dslam_icp_hip", "-Wl,-rpath," + pkg, "-o", str(exe)])
    assert subprocess.run([str(exe)], capture_output=True, timeout=60).returncode == 2
