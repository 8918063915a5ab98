"""Block-cyclic placement on the GPU (include/gpu_actor_place.h): the two- and
three-rank parity cases of tests/test_multirank.py under Engine(block_bits=b),
every rank on the one GPU through the host transport
(tests/mr_place_worker.py). The oracle has no ranks, so parity with it means
the placement moved actors and nothing else: state, steps, delivered, sent,
pending and the per-type counts are the oracle's, nothing is dropped, and the
session reports the block size asked for.

What `remote` counts: gpu_actor_counts' `remote` is per rank and not summed —
the cross-rank records that rank received in its exchanges (plus, for GUPS,
the updates of peers' chunks it applied). Host sends are injected by their
owner and never cross. So for the rings the expectation below is, per rank,
the hops of a Python walk that end on that rank and started on another; with
b = 0 that walk gives 200 per rank for `ring` (4 rings x 100 hops, every hop
crossing, half of them into each rank), the figure the default placement
reports."""
import json
import os

import numpy as np
import pytest

from test_multirank import _launch

pytestmark = pytest.mark.gpu


def run_case(case, ranks, bits):
    out = _launch("mr_place_worker.py", ranks, case, "--bits", str(bits))
    line = [l for l in out.splitlines() if l.startswith("MR_RESULT ")]
    assert line, out[-2000:]
    r = json.loads(line[-1][len("MR_RESULT "):])
    print(case, ranks, bits, {k: r[k] for k in ("steps", "delivered", "remote", "block_bits",
                                                "zone_bits", "local_count")})
    assert r["block_bits"] == bits
    assert r["peer_write"] == int(os.environ.get("PONYC_AMD_PEER_WRITE", "0") not in ("", "0"))
    assert r["dropped"] == 0
    assert r["state_equal"]
    assert r["steps"][0] == r["steps"][1]
    assert r["delivered"][0] == r["delivered"][1]
    assert r["sent"][0] == r["sent"][1]
    assert r["pending"][0] == r["pending"][1]
    assert r["by_type"]
    assert all(sum(lc.values()) > 0 for lc in r["local_count"])     # every rank owns actors
    # every rank's share of a type: the ids of its range that the map gives it
    for t, (first, count) in r["ranges"].items():
        owner = (np.arange(first, first + count, dtype=np.uint64) >> np.uint64(bits)) % np.uint64(ranks)
        assert [lc[t] for lc in r["local_count"]] == [int((owner == k).sum()) for k in range(ranks)]
    return r


def ring_walk(ranks, bits, size=64, rings=4, passes=100, first=0):
    """Per rank, the hops of mr_worker's `ring` that arrive from another rank:
    hop k of a ring goes from position k mod size to position (k + 1) mod size."""
    def owner(i):
        return (i >> bits) % ranks
    into = [0] * ranks
    for ring in range(rings):
        base = first + ring * size
        for k in range(passes):
            src, dst = base + k % size, base + (k + 1) % size
            if owner(src) != owner(dst):
                into[owner(dst)] += 1
    return into


@pytest.mark.parametrize("case", ["ring", "ring_prog"])
@pytest.mark.parametrize("bits", [0, 4])
def test_ring_crossings(case, bits):
    """Block boundaries inside a zone; `remote` is exactly the walk's count
    (b = 0: the default placement's figure, the walk confirmed against the engine)."""
    r = run_case(case, 2, bits)
    assert r["remote"] == ring_walk(2, bits)


def test_ring_inside_one_block():
    """64-actor rings in 64-id blocks: no hop crosses."""
    r = run_case("ring", 2, 6)
    assert r["remote"] == [0, 0]
    assert [lc["0"] for lc in r["local_count"]] == [128, 128]


CASES = [
    # random targets through send_serial, the cross-rank record and k_xinject
    ("ubench", 2, 5), ("ubench_det", 2, 5), ("det_prog", 2, 5), ("storm", 2, 5),
    # a rank count that is no power of two through the fast division
    ("ubench_det", 3, 3), ("storm", 3, 3),
    # two types whose first ids are off the block grid; the split sequence
    # number put together again with the new sender id (the 3 ids of
    # fifo_seq_max in 2-id blocks: the sink and one source on rank 0, the other
    # source on rank 1 — 4-id blocks would leave rank 1 without an actor, which
    # the engine refuses: include/gpu_actor_place.h)
    ("fifo", 2, 2), ("fifo_seq_max", 2, 1), ("fifo_seq_max_carry", 2, 1),
    # trigger bytes indexed by the new global id, merged across ranks
    ("mute", 2, 3), ("priority", 2, 3),
    # spawned ids landing at their owner's next local slot
    ("spreader", 2, 5), ("spreader", 3, 5),
    # reducible applies on both ranks; every updater on rank 0
    ("fanin", 2, 1), ("gups", 2, 1), ("gups", 2, 3),
    # zone and exchange spill lists, zones that grow
    ("spill", 2, 4), ("xspill", 2, 4), ("backlog", 2, 4),
]


@pytest.mark.parametrize("case,ranks,bits", CASES)
def test_parity_under_placement(case, ranks, bits):
    r = run_case(case, ranks, bits)
    if case == "gups" and bits == 3:
        assert [lc["0"] for lc in r["local_count"]] == [8, 0]      # the 8 updaters (type 0)


@pytest.mark.parametrize("case", ["storm_9k", "mute_9k", "spreader_13"])
def test_blocks_of_4096_zones(case, monkeypatch):
    """Whole 4096-actor zones of consecutive ids on one rank. mr_worker's
    storm, mute and spreader have fewer than 4096 ids: in 4096-id blocks they
    would leave rank 1 without an actor, which the engine refuses, so these
    are the same worlds grown to two or three blocks (mr_place_worker.CASES)."""
    monkeypatch.setenv("PONYC_AMD_ZONE_BITS", "12")
    r = run_case(case, 2, 12)
    assert r["zone_bits"] == 12


@pytest.mark.parametrize("case", ["ubench", "ring", "spreader", "mute"])
def test_placement_with_peer_write(case, monkeypatch):
    """The same with k_step storing cross-rank records straight into the
    owner's inbox (PONYC_AMD_PEER_WRITE=1)."""
    monkeypatch.setenv("PONYC_AMD_PEER_WRITE", "1")
    r = run_case(case, 2, 4)
    if case == "ring":
        assert r["remote"] == ring_walk(2, 4)


def test_world_with_an_empty_rank_is_refused():
    """256 ids in one 256-id block: rank 1 would own no actor and take no part
    in a step's exchange. run and run_fixed return EINVAL on both ranks, before
    any collective, and the engine shuts down holding nothing."""
    out = _launch("mr_place_worker.py", 2, "ring", "--bits", "8", "--refused")
    line = [l for l in out.splitlines() if l.startswith("MR_REFUSED ")]
    assert line, out[-2000:]
    r = json.loads(line[-1][len("MR_REFUSED "):])
    assert [k["local"] for k in r] == [256, 0]
    for k in r:
        assert k["codes"] == [-1, -1]             # GPU_ACTOR_EINVAL
        assert k["live"] == [0, 0]


def test_ranks_must_agree():
    """Rank 0 asks for 16-id blocks, rank 1 for 32-id blocks: init fails on
    both with EINVAL and holds nothing; equal values then work."""
    out = _launch("mr_place_worker.py", 2, "ring", "--mismatch", "4,5")
    line = [l for l in out.splitlines() if l.startswith("MR_MISMATCH ")]
    assert line, out[-2000:]
    r = json.loads(line[-1][len("MR_MISMATCH "):])
    assert len(r) == 2
    for k in r:
        assert k["code"] == -1                    # GPU_ACTOR_EINVAL
        assert k["live"] == [0, 0]
        assert k["again"] == 4


def test_single_rank_accepts_and_ignores():
    """block_bits = 11 with one rank: accepted, reported, and nothing changes —
    ubench 9000 against the oracle."""
    import pyoracle
    from ponyc_amd import workloads as W
    from ponyc_amd.engine import Engine
    with Engine(device=0, block_bits=11) as e:
        w = W.ubench(e, 9000, initial=4, budget=32)
        steps = e.run()
        got = W.ubench_result(e, w)
        cnt = e.counts()
        assert e.debug_info()["block_bits"] == 11
        ids = np.arange(9000, dtype=np.uint64)
        assert not e.owner_of(ids).any() and np.array_equal(e.slot_of(ids), ids)
    # (the library keeps the choice for later sessions of this process)
    assert e.lib.gpu_actor_place_blocks(0) == 0
    with pyoracle.Oracle() as o:
        wo = W.ubench(o, 9000, initial=4, budget=32)
        osteps = o.run()
        want = W.ubench_result(o, wo)
        ocnt = o.counts()
    assert np.array_equal(got, want)
    assert steps == osteps
    for k in ("delivered", "sent", "pending", "delivered_by_type"):
        assert cnt[k] == ocnt[k], k
    assert cnt["dropped"] == 0 and cnt["remote"] == 0
