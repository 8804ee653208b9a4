"""CPU-only checks of the drop-in boundary: the C-ABI library loads, exports every symbol include/*.h declares, and
refuses to run without a gfx950 device (no fallback).  No compute calls."""
import ctypes as C
import glob
import os
import re

import pytest

from open3d_slam_advanced_rss_2024_public_amd import _lib, icp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols(headers):
    syms = []
    for hdr in headers:
        text = open(os.path.join(ROOT, "include", hdr)).read()
        text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
        syms += re.findall(r"\b(o3s_[a-z0-9_]+)\s*\(", text)
    return sorted(set(syms))


def test_library_exports_every_declared_symbol():
    _lib.build()
    headers = sorted(os.path.basename(h) for h in glob.glob(os.path.join(ROOT, "include", "*.h")))
    assert headers == ["o3s_cloud_ops.h", "o3s_dense_map.h", "o3s_icp.h", "o3s_rccl.h", "o3s_registration.h", "o3s_scan.h", "o3s_submap.h"]
    L = _lib.lib()
    syms = declared_symbols(["o3s_icp.h", "o3s_cloud_ops.h", "o3s_submap.h", "o3s_scan.h", "o3s_registration.h", "o3s_dense_map.h"])
    assert len(syms) >= 58 and "o3s_dense_map_carve" in syms and "o3s_dense_map_insert_scan" in syms and "o3s_submap_carve" in syms and "o3s_o3d_registration_icp" in syms and "o3s_o3d_registration_icp_batch" in syms and "o3s_o3d_registration_icp_submaps" in syms and "o3s_scan_preprocess" in syms and "o3s_estimate_normals" in syms and "o3s_icp_shard_configure" in syms and "o3s_submap_set_reference" in syms
    for s in syms:
        assert hasattr(L, s), f"{s} declared in include/ but not exported"
    assert L.o3s_abi_version() == 1
    R = _lib.rccl_lib()   # the RCCL exchange lives in its own library (include/o3s_rccl.h)
    rsyms = declared_symbols(["o3s_rccl.h"])
    assert len(rsyms) == 6
    for s in rsyms:
        assert hasattr(R, s), f"{s} declared in include/o3s_rccl.h but not exported"


def test_product_library_carries_no_test_hook_and_reads_no_environment():
    """The shipped libo3dslam_icp_hip.so: no O3S_* environment name in the binary (test hooks, tuning knobs and the work-skipping
    O3S_DBG switches live in libo3dslam_icp_hip_hooks.so, -DO3S_TEST_HOOKS), and the kernels' symbol names show no `dbg` variant.
    The hooks build exports the same C ABI, so a test can run on either."""
    import subprocess

    _lib.build()
    prod = subprocess.run(["strings", "-a", _lib.variant_path(None)], capture_output=True, text=True, check=True).stdout
    names = sorted(set(re.findall(r"\bO3S_[A-Z0-9_]{3,}\b", prod)))
    env_like = [n for n in names if not n.startswith(("O3S_ERR", "O3S_OK", "O3S_XCHG", "O3S_ABI"))]
    assert env_like == [], env_like
    hooks = subprocess.run(["strings", "-a", _lib.variant_path("hooks")], capture_output=True, text=True, check=True).stdout
    for n in ("O3S_DBG", "O3S_SCATTER_ORDER", "O3S_FUSE", "O3S_SEL_PARTIAL", "O3S_NO_HINT", "O3S_HINT_MISS", "O3S_INSERT_SORT"):
        assert n in hooks, n
    H = _lib.load("hooks")
    for sname in declared_symbols(["o3s_icp.h", "o3s_cloud_ops.h", "o3s_submap.h", "o3s_scan.h", "o3s_registration.h", "o3s_dense_map.h"]):
        assert hasattr(H, sname), f"{sname} missing from the hooks build"


def test_default_config_matches_icp_yaml():
    """open3d_slam_ros/param/icp.yaml:11-35."""
    c = _lib.IcpConfigC()
    _lib.lib().o3s_icp_default_config(C.byref(c))
    assert (c.matcher, c.max_iters, c.smooth_length, c.use_differential, c.counter_first) == (0, 15, 3, 1, 0)
    assert abs(c.max_dist - 0.5) < 1e-7 and abs(c.trim_ratio - 0.9) < 1e-7 and abs(c.max_normal_angle - 1.57) < 1e-6
    assert abs(c.min_diff_rot - 0.001) < 1e-9 and abs(c.min_diff_trans - 0.01) < 1e-9 and c.max_dist_outlier < 0
    py = icp.IcpConfig().to_c()
    for f, _ in _lib.IcpConfigC._fields_:
        if f not in ("reserved",):
            assert getattr(py, f) == getattr(c, f), f


def test_yaml_chain_loader():
    text = """
readingDataPointsFilters:
referenceDataPointsFilters:
matcher:
  KDTreeMatcher:
    knn: 1
    maxDist: 0.5
    epsilon: 0.01
outlierFilters:
  - TrimmedDistOutlierFilter:
     ratio: 0.90
  - SurfaceNormalOutlierFilter:
     maxAngle: 1.57
errorMinimizer:
  PointToPlaneErrorMinimizer
transformationCheckers:
  - DifferentialTransformationChecker:
      minDiffRotErr: 0.001
      minDiffTransErr: 0.01
      smoothLength: 3
  - CounterTransformationChecker:
      maxIterationCount: 15
inspector:
  NullInspector
logger:
  NullLogger
"""
    cfg = icp.IcpConfig.from_yaml(text)
    assert cfg == icp.IcpConfig()
    with pytest.raises(icp.InvalidModuleType):
        icp.IcpConfig.from_yaml("errorMinimizer:\n  PointToPointErrorMinimizer\n")
    c2 = icp.IcpConfig.from_yaml("matcher:\n  MirrorMatcher\nerrorMinimizer:\n  PointToPlaneErrorMinimizer\n"
                                 "transformationCheckers:\n  - CounterTransformationChecker:\n      maxIterationCount: 30\n")
    assert c2.matcher == "MirrorMatcher" and c2.trim_ratio is None and c2.max_iters == 30 and not c2.use_differential


def test_no_gpu_means_loud_failure():
    """The product path must fail loudly when no gfx950 device is usable (there is no CPU fallback)."""
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    with pytest.raises(icp.HipError):
        icp.ICP(icp.IcpConfig())
    c = icp.IcpConfig().to_c()
    c.max_dist = -1.0
    h = C.c_void_p()
    assert _lib.lib().o3s_icp_create(C.byref(c), 0, C.byref(h)) == _lib.ERR_BAD_CONFIG


def test_side_operators_refuse_bad_arguments_and_fail_loudly_without_a_gpu():
    """Argument checks of the submap / dense-map / registration entries come before any device work, so they can be
    exercised here; a well-formed create without a usable gfx950 device must fail (no CPU fallback anywhere)."""
    import numpy as np
    import torch

    from open3d_slam_advanced_rss_2024_public_amd import cloud_ops as co
    from open3d_slam_advanced_rss_2024_public_amd import dense_map as dm
    from open3d_slam_advanced_rss_2024_public_amd import registration as reg
    from open3d_slam_advanced_rss_2024_public_amd import submap as sm

    L = _lib.lib()
    dm._L(), reg._L(), sm._L()   # bind argtypes
    h = C.c_void_p()
    assert L.o3s_dense_map_create(0, 0.0, C.byref(h)) == _lib.ERR_BAD_ARGUMENT and not h.value
    assert L.o3s_dense_map_create(0, float("nan"), C.byref(h)) == _lib.ERR_BAD_ARGUMENT
    assert L.o3s_dense_map_create(0, 0.1, None) == _lib.ERR_BAD_ARGUMENT
    assert L.o3s_dense_map_size(None) == 0 and L.o3s_dense_map_has_normals(None) == 0
    assert L.o3s_dense_map_insert(None, None, None, 0) == _lib.ERR_BAD_ARGUMENT
    assert L.o3s_dense_map_carve(None, None, None, 0, None, None) == _lib.ERR_BAD_ARGUMENT
    assert L.o3s_dense_map_transform(None, None) == _lib.ERR_BAD_ARGUMENT
    assert L.o3s_dense_map_to_point_cloud(None, None, None, None, None, None) == _lib.ERR_BAD_ARGUMENT
    L.o3s_dense_map_destroy(None)   # a no-op
    assert L.o3s_o3d_registration_icp_batch(0, -1, None, 1.0, None, None, None, None) == _lib.ERR_BAD_ARGUMENT
    assert L.o3s_o3d_registration_icp_batch(0, 0, None, 1.0, None, None, None, None) == _lib.OK   # nothing to do
    assert L.o3s_o3d_registration_icp_submaps(None, None, 1.0, None, None, None, None) == _lib.ERR_BAD_ARGUMENT
    assert L.o3s_submap_create(0, 0.1, None, C.byref(h)) == _lib.ERR_BAD_ARGUMENT
    if torch.cuda.is_available():
        return
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        dm.DenseMap(0.1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        sm.Submap(0.1, co.croppingVolumeFactory("MaxRadius", 10.0))
    p = np.zeros((4, 3))
    with pytest.raises(RuntimeError):
        reg.registration_icp(p, p, p, 1.0)
    with pytest.raises(RuntimeError):
        reg.registration_icp_batch([(p, p, p, None)], 1.0)


def test_cpp_shim_compiles_and_links_with_plain_gxx(tmp_path):
    """The header-only C++ shim a catkin package would include (open3d_slam_advanced_rss_2024_public_amd/cpp/o3s_icp.hpp)
    builds with g++ against the C ABI only (no HIP, Eigen or libpointmatcher headers) and maps create failures to
    std::runtime_error."""
    import subprocess

    _lib.build()
    src = tmp_path / "shim.cpp"
    src.write_text('#include "o3s_icp.hpp"\n#include <cstdio>\nint main(){ try { o3s::IcpHip icp(0); o3s_cropper c{}; c.kind = 1; c.p0 = 10.0;'
                   ' o3s::SubmapHip sm(0.1, c, 0); o3s::DenseMapHip dm(0.05, 0); std::puts("created"); }'
                   ' catch (const std::runtime_error& e) { std::printf("runtime_error: %s\\n", e.what()); } return 0; }\n')
    pkg = os.path.join(ROOT, "open3d_slam_advanced_rss_2024_public_amd")
    exe = tmp_path / "shim"
    subprocess.check_call(["g++", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(pkg, "cpp"), str(src),
                           "-L" + pkg, "-lo3dslam_icp_hip", "-Wl,-rpath," + pkg, "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0
    assert ("created" in out.stdout) or ("runtime_error" in out.stdout)


def test_headers_are_plain_c(tmp_path):
    """The boundary is a C ABI: every header under include/ must compile as C99 (what a cgo / JNI / ctypes-free C host sees)."""
    import subprocess

    src = tmp_path / "c_abi.c"
    headers = sorted(os.path.basename(h) for h in glob.glob(os.path.join(ROOT, "include", "*.h")))
    src.write_text("".join(f'#include "{h}"\n' for h in headers) +
                   "int main(void) { o3s_icp_config c; o3s_icp_default_config(&c); return 0; }\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c", str(src),
                           "-o", str(tmp_path / "c_abi.o")])


@pytest.mark.parametrize("order", ["library_first", "torch_first"])
def test_one_rocm_runtime_per_process_whatever_the_import_order(order):
    """PyTorch wheels ship their own libamdhip64 / libhsa-runtime64 / librccl.  Loading this library before torch used to
    leave TWO HIP and two HSA runtimes in the process (the library bound to /opt/rocm's by soname, torch then mapped its
    own by file name) — the cause of the GPU-side initialisation failure round 2 worked around with a child process.
    _lib.lib() now maps torch's runtime first when torch is installed: one runtime of each kind in either order."""
    import subprocess
    import sys

    prog = (
        "import sys; sys.path.insert(0, %r)\n"
        "from open3d_slam_advanced_rss_2024_public_amd import _lib\n"
        + ("_lib.lib(); _lib.rccl_lib(); import torch\n" if order == "library_first" else "import torch; _lib.lib(); _lib.rccl_lib()\n")
        + "import os, collections\n"
        "c = collections.Counter(os.path.basename(p).split('.so')[0] for p in _lib.loaded_rocm_runtimes())\n"
        "print(dict(c)); assert c and all(v == 1 for v in c.values()), _lib.loaded_rocm_runtimes()\n"
    ) % ROOT
    out = subprocess.run([sys.executable, "-c", prog], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.stdout[-500:], out.stderr[-1500:])
    assert "libamdhip64" in out.stdout


def test_bench_refuses_more_gpus_than_the_node_has_with_one_line():
    """`python bench.py --gpus N` starts its own N ranks — after counting the node's GPUs WITHOUT touching the HIP runtime; with
    fewer than N it must stop with one line on stderr and exit code 2 (no traceback, no hang in a rendezvous)."""
    import subprocess
    import sys

    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "64", "--steps", "1", "--warmup", "0"], capture_output=True,
                         text=True, timeout=300)
    assert out.returncode == 2, (out.returncode, out.stderr[-500:])
    lines = [ln for ln in out.stderr.splitlines() if ln.strip()]
    assert len(lines) == 1 and "--gpus 64" in lines[0] and "GPU(s)" in lines[0], out.stderr[-500:]
    assert out.stdout.strip() == ""


def test_bench_refuses_a_run_without_timed_steps():
    """`--steps` is the number of timed steps and `ms_per_step` is divided by it: zero steps is a usage error (exit 2), found before
    anything touches the GPU."""
    import subprocess
    import sys

    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "0", "--warmup", "0"], capture_output=True,
                         text=True, timeout=300)
    assert out.returncode == 2, (out.returncode, out.stderr[-500:])
    assert "--steps" in out.stderr and out.stdout.strip() == ""


def test_bench_keeps_what_lies_beyond_the_headline_behind_full():
    """A plain run prints the headline alone; the roofline, the CPU baseline and the extras are asked for with --full, which `--help`
    lists without anything touching the GPU."""
    import subprocess
    import sys

    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-500:]
    assert "--full" in out.stdout


def test_a_forked_child_does_not_destroy_the_parents_handles():
    """multiprocessing workers forked from a process that holds device handles inherit the wrappers; a garbage collection in
    the worker must not call into the library (the HIP runtime does not survive a fork): close() drops the handle instead."""
    import os
    from open3d_slam_advanced_rss_2024_public_amd import _lib

    class W:
        pass

    w = W()
    assert not _lib.forked_copy(w)          # no pid recorded: treated as ours
    w._pid = os.getpid()
    assert not _lib.forked_copy(w)
    r, wr = os.pipe()
    pid = os.fork()
    if pid == 0:
        os.write(wr, b"1" if _lib.forked_copy(w) else b"0")
        os._exit(0)
    os.waitpid(pid, 0)
    assert os.read(r, 1) == b"1"
    os.close(r)
    os.close(wr)
