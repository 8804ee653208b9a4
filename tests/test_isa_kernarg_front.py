"""The front of a launch, as the compiler emits it (tools/isa_round_trips.py --kernarg-front).

Every address a kernel loads from comes out of a kernel argument.  The library is built with -amdgpu-kernarg-preload-count, so the
leading arguments (14 dwords beside the kernarg pointer on gfx950; the run ends at the first by-value struct) arrive in SGPRs at
wave launch, and the chain kernels' parameters are ordered so that what the first round trip reads through stands inside that
window.  Both are properties that erode silently: a struct moved in front of a pointer, a new leading argument, or a flag lost from
HIPFLAGS still compiles and still computes the same bits.  This test compiles the device code once, as the library is built, and
checks per kernel that
  - the preload length is at least what profiles/r11/NOTES.md records for it, and
  - the first vector load does not sit behind an `s_waitcnt lgkmcnt` with a kernarg scalar load outstanding.
"""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_round_trips as isa  # noqa: E402

pytestmark = pytest.mark.skipif(isa.hipcc() is None, reason="hipcc is not installed")

# dwords of arguments preloaded, per kernel (profiles/r11/NOTES.md, "the window per kernel")
PRELOAD = {
    "k_match2<false,4,2,4,true,true,true>": 14,   # the settle front: launches 2.. of a chain
    "k_match2<false,2,2,4,true,true>": 14,        # launch 1 (and the kernel tests/test_isa_round_trips.py knows)
    "k_match2<false,4,2,4,true,false>": 14,       # the first iteration
    "k_classify": 14,
    "k_sel_ne": 14,
    "k_solve": 14,
    "k_sel_partial": 14,
    "k_sel_finish": 14,
    "k_normal_eq": 13,
    "k_read_prep": 5,
    "k_read_starts": 12,
    "k_read_scatter": 14,
    "k_read_place": 14,
}
# Kernels whose first vector load may wait for a fetched argument, by name and with the reason.  The list may not grow silently:
# test_exempt_list_is_exactly_this pins it.
EXEMPT = {
    "k_read_prep": "its front is not a load: it first clears the sort's counters from PrepInit, and the pose (Mat16, 16 dwords by value), "
                   "the grid and PrepInit alone are more than the 14 preloaded dwords; one launch per registration",
}


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    return isa.parse(isa.compile_asm(str(tmp_path_factory.mktemp("isa_front"))))


def test_makefile_builds_with_kernarg_preloading():
    assert any(f.startswith("-amdgpu-kernarg-preload-count=") for f in isa.makefile_flags()), isa.makefile_flags()


@pytest.mark.parametrize("spec", list(PRELOAD))
def test_preload_length_and_first_load(kernels, spec):
    f = isa.kernarg_front(isa.find(kernels, spec))
    print(f)
    assert f["preload"] >= PRELOAD[spec], (spec, f["preload"])
    if spec in EXEMPT:
        return
    assert f["batch_loads"] > 0, spec
    assert f["first_wait"] is None, f"{spec}: the first vector load waits for a fetched argument ({f['first_wait']}); fetched ahead of it: {f['sloads']}"


def test_exempt_list_is_exactly_this():
    assert sorted(EXEMPT) == ["k_read_prep"]
    assert set(EXEMPT) <= set(PRELOAD) and set(PRELOAD) == set(isa.FRONT_KERNELS)
