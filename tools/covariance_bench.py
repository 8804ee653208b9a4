"""GPU-box helper: what the pose covariance (PointToPlaneWithCovErrorMinimizer, o3s_icp_config::error_minimizer = 1) costs.

The icp.yaml chain (it stops by itself) on the C2 pair — a 100 000-point reading against a 2 M-point voxel map — per registration
on the resident reading (o3s_icp_compute_resident), median of CALLS (default 40) calls after WARM (5):

  default     the product library, error_minimizer 0
  covariance  the product library, error_minimizer 1; also the device time of the added pass from its own stamps
              (o3s_icp_covariance_gpu_us: k_cov start -> k_cov_post end, and the chain's final post -> k_cov_post end)
  parent      the same chain on the library of the parent commit, TWICE, when PARENT=<path to its libo3dslam_icp_hip.so> is given
              (default: libo3dslam_icp_hip_parent.so beside the product library, if it is there).  The difference of its two
              runs is the spread a difference between default and parent has to be read against.

Every library is driven through the same few C ABI calls from here (ctypes), so the parent needs none of the newer symbols.
The runs alternate (parent, default, parent, default, covariance); a run is a fresh handle.  wall = host time around the call;
gpu = o3s_icp_stats::gpu_ms (the chain's own stamps).  SCAN / MAP override the sizes; OUT=<path> also writes the JSON there
(profiles/covariance/)."""
import ctypes as C
import gc
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from open3d_slam_advanced_rss_2024_public_amd import _lib, synthetic as syn  # noqa: E402
from open3d_slam_advanced_rss_2024_public_amd.icp import IcpConfig, as_xyzw  # noqa: E402

CALLS = int(os.environ.get("CALLS", "40"))
WARM = int(os.environ.get("WARM", "5"))
SCAN = int(os.environ.get("SCAN", "100000"))
MAP = int(os.environ.get("MAP", "2000000"))
PARENT = os.environ.get("PARENT") or _lib.variant_path("parent")


def fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def open_library(path):
    _lib._preload_torch_runtime(["libamdhip64.so"])
    L = C.CDLL(path)
    vp, f = C.c_void_p, C.POINTER(C.c_float)
    L.o3s_icp_create.argtypes = [C.POINTER(_lib.IcpConfigC), C.c_int, C.POINTER(vp)]
    L.o3s_icp_destroy.argtypes = [vp]
    L.o3s_icp_destroy.restype = None
    L.o3s_icp_init_reference.argtypes = [vp, f, f, C.c_int64]
    L.o3s_icp_set_reading.argtypes = [vp, f, f, C.c_int64]
    L.o3s_icp_compute_resident.argtypes = [vp, f, f, C.POINTER(_lib.IcpStatsC)]
    if hasattr(L, "o3s_icp_covariance_gpu_us"):
        L.o3s_icp_covariance_gpu_us.argtypes = [vp, C.POINTER(C.c_double)]
        L.o3s_icp_get_covariance.argtypes = [vp, C.POINTER(C.c_double)]
    return L


def median(v):
    return float(np.median(np.asarray(v, np.float64)))


def run(L, sp, covariance):
    cfg = IcpConfig(error_minimizer="PointToPlaneWithCovErrorMinimizer" if covariance else "PointToPlaneErrorMinimizer").to_c()
    h = C.c_void_p()
    assert L.o3s_icp_create(C.byref(cfg), 0, C.byref(h)) == 0
    ref, refn = as_xyzw(sp.map_xyz), np.ascontiguousarray(sp.map_normals, np.float32)
    scan, scann = as_xyzw(sp.scan_xyz), np.ascontiguousarray(sp.scan_normals, np.float32)
    assert L.o3s_icp_init_reference(h, fp(ref), fp(refn), len(ref)) == 0
    assert L.o3s_icp_set_reading(h, fp(scan), fp(scann), len(scan)) == 0
    Tin = np.ascontiguousarray(sp.T_init.astype(np.float32).T).reshape(16)
    Tout = np.zeros(16, np.float32)
    st = _lib.IcpStatsC()
    wall, gpu, cov_pass, cov_behind = [], [], [], []
    out2 = (C.c_double * 2)()
    gc.disable()
    for k in range(WARM + CALLS):
        t0 = time.perf_counter()
        rc = L.o3s_icp_compute_resident(h, fp(Tin), fp(Tout), C.byref(st))
        dt = (time.perf_counter() - t0) * 1e6
        assert rc == 0
        if k < WARM:
            continue
        wall.append(dt)
        gpu.append(st.gpu_ms * 1e3)
        if covariance:
            assert L.o3s_icp_covariance_gpu_us(h, out2) == 0
            cov_pass.append(out2[0])
            cov_behind.append(out2[1])
    gc.enable()
    r = {"wall_us_median": median(wall), "wall_us_min": float(min(wall)), "chain_gpu_us_median": median(gpu), "iterations": int(st.iterations),
         "kept_pairs": int(st.kept_pairs), "pose": [float(x) for x in Tout]}
    if covariance:
        c = np.zeros(36)
        assert L.o3s_icp_get_covariance(h, c.ctypes.data_as(C.POINTER(C.c_double))) == 0
        r.update(cov_pass_gpu_us_median=median(cov_pass), cov_behind_chain_gpu_us_median=median(cov_behind),
                 cov_diag=[float(c[7 * k]) for k in range(6)])
    L.o3s_icp_destroy(h)
    return r


def main():
    sp = syn.make_scan_pair(SCAN, MAP, 0.1)
    product = open_library(_lib.variant_path(None))
    parent = open_library(PARENT) if os.path.exists(PARENT) else None
    res = {"workload": f"icp.yaml chain, {SCAN}-point reading vs {MAP}-point map, resident reading, median of {CALLS} calls after {WARM}"}
    if parent:
        res["parent_a"] = run(parent, sp, False)
    res["default_a"] = run(product, sp, False)
    if parent:
        res["parent_b"] = run(parent, sp, False)
    res["default_b"] = run(product, sp, False)
    res["covariance"] = run(product, sp, True)
    res["same_pose_with_and_without"] = res["covariance"]["pose"] == res["default_a"]["pose"]
    if parent:
        res["same_pose_as_parent"] = res["parent_a"]["pose"] == res["default_a"]["pose"]
        for key in ("wall_us_median", "chain_gpu_us_median"):
            pa, pb = res["parent_a"][key], res["parent_b"][key]
            d = min(res["default_a"][key], res["default_b"][key])
            res[f"{key}_parent_spread"] = abs(pa - pb)
            res[f"{key}_default_minus_parent"] = d - min(pa, pb)
    for key in ("wall_us_median", "chain_gpu_us_median"):
        res[f"{key}_covariance_minus_default"] = res["covariance"][key] - min(res["default_a"][key], res["default_b"][key])
    for k in ("parent_a", "parent_b", "default_a", "default_b", "covariance"):
        if k in res:
            res[k].pop("pose")
    line = json.dumps(res)
    print(line)
    out = os.environ.get("OUT")
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
