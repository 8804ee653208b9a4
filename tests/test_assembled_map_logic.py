"""The host side of the assembled map on the CPU: which submaps SubmapCollection.assembleMap hands to the one device call
(Mapper::getAssembledMapPointCloud's loop, Mapper.cpp:524-535: every submap in index order, the active one not special) and
SubmapCollection::getTotalNumPoints (SubmapCollection.cpp:69-73), with stand-in submaps and a stand-in for the device call; and the
new header under the checks tests/test_abi.py applies to the headers of include/ (plain C99, every declared symbol exported).  The
device work itself is tests/test_gpu_assembled_map.py's."""
import os
import re
import subprocess

from open3d_slam_advanced_rss_2024_public_amd import _lib
from open3d_slam_advanced_rss_2024_public_amd.mapper import Mapper
from open3d_slam_advanced_rss_2024_public_amd.submap_collection import SubmapCollection
from test_submap_collection_logic import FakeScan, FakeSubmap, drive

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class Recorder:
    """Stand-in for AssembledMap.build: keeps what it was called with and answers with the sum of the sizes."""

    def __init__(self):
        self.calls = []

    def __call__(self, out, maps, voxel_size, normals, colors):
        self.calls.append((out, list(maps), voxel_size, normals, colors))
        return sum(len(m) for m in maps)


def make(rec, **kw):
    args = dict(radius=10.0, min_num=2, max_points=10 ** 9, overlap=1)
    args.update(kw)
    return SubmapCollection(args["radius"], args["min_num"], args["max_points"], args["overlap"], 0.1, ("MaxRadius", 30.0), submap_factory=FakeSubmap,
                            scan_factory=FakeScan, assemble_maps=rec)


def test_submaps_are_passed_in_index_order_whichever_is_active():
    rec = Recorder()
    col = make(rec)
    out_and_back = [0, 4, 8, 12, 16, 20, 24, 20, 16, 12, 8, 4, 0]       # three submaps on the way out, adjacent ones revisited on the way back
    log = drive(col, out_and_back)
    assert len(col.maps) == 3 and col.active != len(col.maps) - 1        # the active submap is not the last one
    assert {a for a, _, _ in log} == {0, 1, 2}
    out = object()
    n = col.assembleMap(out, 0.1, True, False)
    assert rec.calls[-1][0] is out and rec.calls[-1][2:] == (0.1, True, False)
    assert all(a is b for a, b in zip(rec.calls[-1][1], col.maps)) and len(rec.calls[-1][1]) == 3
    assert n == sum(len(m) for m in col.maps)
    col.assembleMap(out)                                                 # the defaults: plain concatenation, both attributes wanted
    assert rec.calls[-1][2:] == (0.0, True, True)
    # Mapper::getAssembledMapPointCloud goes through the collection
    mapper = Mapper(None, col, None, None, 0.1, 1.0, 0.0)
    assert mapper.getAssembledMapPointCloud(out, 0.25) == n
    assert rec.calls[-1][0] is out and rec.calls[-1][2:] == (0.25, True, True) and all(a is b for a, b in zip(rec.calls[-1][1], col.maps))


def test_total_num_points_sums_the_sizes():
    col = make(Recorder())
    assert col.getTotalNumPoints() == 0
    drive(col, [0, 4, 8, 12, 16, 20, 24])
    assert len(col.maps) >= 2
    assert col.getTotalNumPoints() == sum(1000 * len(m.scans) for m in col.maps) > 0


def test_an_empty_collection_passes_its_one_empty_submap():
    rec = Recorder()
    col = make(rec)
    assert col.assembleMap(object()) == 0
    assert len(rec.calls[-1][1]) == 1 and rec.calls[-1][1][0] is col.maps[0] and len(col.maps[0]) == 0


HEADER = "assembled_map/o3s_assembled_map.h"


def test_the_header_is_plain_c(tmp_path):
    src = tmp_path / "c_abi.c"
    src.write_text(f'#include "{HEADER}"\n'
                   "int main(void) { o3s_assembled_map* a = 0; return o3s_assembled_map_create(0, &a) == O3S_OK && "
                   "o3s_assembled_map_size(a) == 0 ? (O3S_ASSEMBLE_NORMALS | O3S_ASSEMBLE_COLORS) - 3 : 0; }\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c", str(src),
                           "-o", str(tmp_path / "c_abi.o")])


def test_both_builds_export_every_declared_symbol_and_refuse_bad_arguments():
    _lib.build()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", HEADER)).read(), flags=re.S)
    syms = sorted(set(re.findall(r"\b(o3s_assembled_map_[a-z0-9_]+)\s*\(", text)))
    assert len(syms) == 9
    for L in (_lib.lib(), _lib.load("hooks")):
        for s in syms:
            assert hasattr(L, s), f"{s} declared in include/{HEADER} but not exported"
    # argument checks come before any device work
    from open3d_slam_advanced_rss_2024_public_amd import submap as sm

    L = sm._L()
    assert L.o3s_assembled_map_create(0, None) == _lib.ERR_BAD_ARGUMENT
    assert L.o3s_assembled_map_build(None, 0, None, 0.0, 0, None) == _lib.ERR_BAD_ARGUMENT
    assert L.o3s_assembled_map_download(None, None, None, None) == _lib.ERR_BAD_ARGUMENT
    assert L.o3s_assembled_map_to_submap(None, None) == _lib.ERR_BAD_ARGUMENT
    assert L.o3s_assembled_map_size(None) == 0 and L.o3s_assembled_map_device_bytes(None) == 0
    assert L.o3s_assembled_map_has_normals(None) == 0 and L.o3s_assembled_map_has_colors(None) == 0
    L.o3s_assembled_map_destroy(None)   # a no-op
