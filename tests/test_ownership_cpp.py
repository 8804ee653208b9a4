"""csrc/lease_pool.h and csrc/dev_mem.h as stand-alone programs under sanitizers (tests/cpp/lease_pool_cases.cpp,
tests/cpp/dev_mem_cases.cpp): plain g++, their own main, nothing loaded into Python.  dev_mem.h compiles against the stand-in
<hip/hip_runtime.h> of tests/cpp/fake_hip, which counts allocations and frees and logs every requested size.
tests/cpp/layout_cases.hip is the third: the work-area layouts of the whole implementation, compiled by hipcc as the library is,
calling host functions only (no GPU needed), against the sizes the formulas before them gave."""
import os
import platform
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "open3d_slam_advanced_rss_2024_public_amd", "csrc")
CPP = os.path.join(ROOT, "tests", "cpp")
THREAD = ["-fsanitize=thread"]
ADDRESS = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


def fixed_layout():
    """Command prefix that runs a program without address-space randomisation, where the machine allows it: a ThreadSanitizer
    runtime older than the kernel's mmap entropy refuses to start when a mapping lands outside the ranges it expects."""
    pre = [shutil.which("setarch") or "setarch", platform.machine(), "-R"]
    try:
        return pre if subprocess.run(pre + ["true"], capture_output=True, timeout=30).returncode == 0 else []
    except OSError:
        return []


def build_and_run(tmp_path, source, flags, includes):
    exe = str(tmp_path / os.path.splitext(source)[0])
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-pthread", *flags, *["-I" + i for i in includes],
                           os.path.join(CPP, source), "-o", exe])
    out = subprocess.run((fixed_layout() if flags is THREAD else []) + [exe], capture_output=True, text=True, timeout=120)
    print(out.stdout)
    assert out.returncode == 0, (out.returncode, out.stdout[-2000:], out.stderr[-4000:])
    assert out.stdout.splitlines()[-1] == "ok" and "Sanitizer" not in out.stderr


@pytest.mark.parametrize("flags", [THREAD, ADDRESS], ids=["thread", "address-undefined"])
def test_lease_pool(tmp_path, flags):
    build_and_run(tmp_path, "lease_pool_cases.cpp", flags, [CSRC])


def test_dev_mem(tmp_path):
    build_and_run(tmp_path, "dev_mem_cases.cpp", ADDRESS, [os.path.join(CPP, "fake_hip"), CSRC])


def test_work_area_layouts(tmp_path):
    """Every layout reserves what its formula reserved before (tests/cpp/layout_cases.hip).  The program defines the cloud
    operators itself; what they call in the other translation unit comes from the built library."""
    pkg = os.path.dirname(CSRC)
    assert os.path.exists(os.path.join(pkg, "libo3dslam_icp_hip.so")), "build() first"
    exe = str(tmp_path / "layout_cases")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.check_call([hipcc, "-std=c++17", "-O1", "--offload-arch=gfx950", "-ffp-contract=off", "-Wall", "-Werror", "-Wno-unused-function",
                           *[f for a in ADDRESS for f in ("-Xarch_host", a)], "-I" + CSRC, os.path.join(CPP, "layout_cases.hip"), "-o", exe,
                           "-L" + pkg, "-lo3dslam_icp_hip", "-Wl,-rpath," + pkg])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(out.stdout)
    assert out.returncode == 0, (out.returncode, out.stdout[-2000:], out.stderr[-4000:])
    assert out.stdout.splitlines()[-1] == "ok" and "Sanitizer" not in out.stderr
