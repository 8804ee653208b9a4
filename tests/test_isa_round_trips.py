"""The first round trip of the chain kernels, as the compiler emits it (tools/isa_round_trips.py).

The chain's kernels are one generation of waves each and bound by latency: inside a launch, what costs is the number of DEPENDENT
memory round trips.  Their source requests everything a block needs first in one batch; whether the ISA does is a property of the
compiler's output, and it has been lost without anyone noticing (the 16 level-1 replica loads of k_classify went from one batch to
sixteen waits when their loop moved into a lambda with an early return).  This test compiles the device code once, as the library is
built, and pins what the source is written for: the number of round trips ahead of the first barrier as an upper bound per kernel,
the replicas as one batch on every call site, and the matched-normal gather in flight across the first barrier.

A round trip ends at an `s_waitcnt vmcnt(n)` that retires at least one outstanding load and has another load behind it; the final
drain is the last one.  The bounds are what the source asks for, not what one compiler happened to give:
  k_sel_ne, k_sel_finish, k_match2 (the variant of the converged chain)   1: everything travels together
  k_solve   2: the state word, staged into LDS, then the 27 partials.  Requesting both together was built and measured: 7.83 / 7.64 us
               in two traces of the parent, 7.69 / 7.72 us with it, inside the parent's own spread; it was taken out again.
  k_classify   2: the header, the point and the speculative words; then the gather of the matched normal, which needs the slot
  k_sel_partial   2: the header ahead of the exit, then the rest (the exit stands in front of its first barrier)
"""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_round_trips as isa  # noqa: E402

pytestmark = pytest.mark.skipif(isa.hipcc() is None, reason="hipcc is not installed")

CERT_MATCH2 = "k_match2<false,2,2,4,true,true>"   # STATS off, two lanes per query, row-disc far search, certificates: the converged C2 chain
MAX_TRIPS = {"k_sel_ne": 1, "k_solve": 2, "k_sel_finish": 1, CERT_MATCH2: 1, "k_classify": 2, "k_sel_partial": 2}
NOT_ENTERED = isa.DEFAULT_IGNORE   # regions the converged C2 chain never enters: the tool's own list, so table and bounds agree
REPLICA_LOAD = "hist_rep + (size_t)"
GATHER_LOAD = "refn[matched ? slot0 : 0]"


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    return isa.compile_both(str(tmp_path_factory.mktemp("isa")))


@pytest.mark.parametrize("spec", list(MAX_TRIPS))
def test_first_round_trip_is_one_batch(kernels, spec):
    k = isa.find(kernels, spec)
    events, serial, loads = isa.first_trip(k, NOT_ENTERED.get(spec, ()))
    print("\n".join(events))
    assert loads > 0
    assert serial + 1 <= MAX_TRIPS[spec], f"{spec}: {serial + 1} round trips ahead of the first barrier\n" + "\n".join(events)


def test_named_regions_exist(kernels):
    """A region that is named but matches no load would silently stop being left out (or never was): every name matches."""
    for spec, texts in NOT_ENTERED.items():
        k = isa.find(kernels, spec)
        for t in texts + [GATHER_LOAD]:
            assert any(kind == "load" and t in loc for kind, _, loc in k.ops), (spec, t)


def test_replica_loads_travel_as_one_batch_on_every_call_site(kernels):
    groups = isa.region_waits(isa.find(kernels, "k_classify"), REPLICA_LOAD, 16)
    print(groups)
    assert len(groups) >= 2                      # load_replicas() is inlined at least at the two call sites the issue names
    assert all(g == (16, 0) for g in groups), groups   # 16 loads, no wait that retires one of them before the last is out


def test_gather_is_in_flight_across_the_first_barrier(kernels):
    """The matched-normal gather is requested right behind the first trip and consumed behind the bin scans: on the converged
    chain's path (the named regions left out, with the waits inside them) no wait stands between the gather and the first s_barrier."""
    k = isa.find(kernels, "k_classify")
    events, _, _ = isa.first_trip(k, NOT_ENTERED["k_classify"])
    at = [j for j, e in enumerate(events) if GATHER_LOAD in e]
    assert len(at) == 1, at
    behind = [e for e in events[at[0] + 1:] if "s_waitcnt" in e]
    assert not behind, "\n".join(events[at[0]:])
    through, _, _ = isa.first_trip(k, NOT_ENTERED["k_classify"], barriers=1)   # and the tool sees it in flight at that barrier
    bar = [e for e in through if "s_barrier" in e]
    assert bar and "0 load(s) in flight" not in bar[0], bar


def test_chain_kernels_use_no_scratch(kernels):
    for spec in MAX_TRIPS:
        k = isa.find(kernels, spec)
        assert "ScratchSize: 0" in k.resources, (spec, k.resources)
