"""The pinger's two-pass plan path (zone_dev.h k_step) with 8-byte tile
records and two super-rounds, against the CPU oracle — bit-exact state,
counts and step count, at both zone geometries.

The shapes are the ones at which that code can go wrong: a super-round's
sends past the tile (the direct-to-chunk branch puts the constant argument
back), a last zone with fewer actors than threads' pairs, lanes that are
almost all empty, actors that reach their budget in mid-step (pass 1's counts
must equal pass 2's sends, or the tile has holes), two ranks (buckets past
the zones: the exchange record's argument), and a batch limit, under which
the zones leave the path for the general one and come back."""
import ctypes
import json

import pytest

from ponyc_amd import workloads as W
from test_gpu_parity import _both, _assert_same
from test_multirank import _launch

pytestmark = pytest.mark.gpu


@pytest.fixture(params=["11", "12"])
def zone_bits(request, monkeypatch):
    monkeypatch.setenv("PONYC_AMD_ZONE_BITS", request.param)
    return int(request.param)


def plan_zones(e) -> int:
    """zone steps that took the plan path (gpu_actor_debug_info's slot 20)"""
    out = (ctypes.c_uint64 * 21)()
    fn = e.lib.gpu_actor_debug_info
    fn.argtypes = [ctypes.c_void_p, ctypes.c_uint64]
    fn.restype = ctypes.c_int
    assert fn(out, 21) == 0
    return int(out[20])


def _run(engine_factory, oracle, n, initial, budget, **kw):
    made = []

    def factory(**ekw):
        e = engine_factory(**ekw)
        made.append(e)
        return e
    g, o = _both(factory, oracle, lambda e: W.ubench(e, n, initial, budget, **kw), W.ubench_result)
    _assert_same(g, o)
    return made[0], g


# (n, initial, budget): every pinger's mail stays within its batch of 100, so
# every zone with mail plans.
#  2048 x 10, budget 8: one zone whose first step sends 2048 * 8 = 16384, a
#    super-round 8192 — the 2048-actor geometry's tile, full to its last place;
#  2048 x 10, budget 12: 20480 sends, 10240 a super-round — past that tile, in
#    both super-rounds (the direct branch);
#  4096 x 8, budget 8: a 4096-actor zone's 32768 sends, 16384 a super-round —
#    past its tile of 14336 (two zones of 8192 a super-round at 2048);
#  4196 x 5, budget 6: a last zone of 100 actors (nact < kZone): most threads
#    have no second actor in a super-round, or none at all;
#  8 x 5, budget 1000 and 1000 x 5, budget 3: nearly every lane empty; with
#    budget 3 the later messages of a step send nothing.
SHAPES = [(2048, 10, 8), (2048, 10, 12), (4096, 8, 8), (4096 + 100, 5, 6), (8, 5, 1000),
          (1000, 5, 3)]


@pytest.mark.parametrize("n,initial,budget", SHAPES)
def test_plan_pairs(engine_factory, oracle, zone_bits, n, initial, budget):
    e, g = _run(engine_factory, oracle, n, initial, budget)
    assert g[1]["debug"]["zone_bits"] == zone_bits
    # (an engine of a few actors runs its steps on the small-step path, k_sparse)
    if n >= 2048:
        assert plan_zones(e) > 0           # the two-pass path was taken
    assert g[1]["sent"] > 0


def test_plan_pairs_batch_limit(engine_factory, oracle, zone_bits):
    """40 pings per pinger against a batch of 3: mail is carried and actors
    overload, so the zones leave the plan path (through zone_step_rest, which
    shares the zone's LDS and the dynamic bucket arrays) and stay exact."""
    e, g = _run(engine_factory, oracle, 512, 40, 60, batch=3)
    assert plan_zones(e) < g[0]           # the backlog's steps did not plan


@pytest.mark.parametrize("zones", ["11", "12"])
def test_plan_pairs_two_ranks(zones, monkeypatch):
    """2048 * 3 pingers on two ranks over the host transport: half of every
    zone's sends go to the bucket of the peer rank (b >= nz), whose exchange
    record gets the constant argument back."""
    monkeypatch.setenv("PONYC_AMD_ZONE_BITS", zones)
    out = _launch("mr_plan_pairs_worker.py", 2)
    line = [l for l in out.splitlines() if l.startswith("MR_RESULT ")]
    assert line, out[-2000:]
    r = json.loads(line[-1][len("MR_RESULT "):])
    assert r["dropped"] == 0
    assert r["state_equal"]
    assert r["steps"][0] == r["steps"][1]
    assert r["delivered"][0] == r["delivered"][1]
    assert r["sent"][0] == r["sent"][1]
    assert r["pending"][0] == r["pending"][1]
    assert r["by_type"]
    assert r["remote"] > 0
    assert r["plan_zones"] > 0
