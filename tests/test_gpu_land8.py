"""The compact landing lane: 8-byte {w0, from} records between
plan-path zones of the pinger table, against the CPU oracle — bit-exact state
and counters. Every case asserts from debug_info which path ran: plan zone
steps, and records taken from the compact lane (> 0 with the lane, 0 with
PONYC_AMD_LAND8=0)."""
import json

import numpy as np
import pytest

from ponyc_amd import workloads as W
from ponyc_amd.engine import live_buffers
from test_gpu_parity import _both, _assert_same
from test_gpu_split import FORMS
from test_multirank import _launch

pytestmark = pytest.mark.gpu


@pytest.fixture(params=["11", "12"])
def zone_bits(request, monkeypatch):
    monkeypatch.setenv("PONYC_AMD_ZONE_BITS", request.param)
    return int(request.param)


def _totals(e, o):
    ce, co = e.counts(), o.counts()
    assert ce["dropped"] == 0
    for k in ("delivered", "sent", "pending", "delivered_by_type"):
        assert ce[k] == co[k], (k, ce[k], co[k])


@pytest.mark.parametrize("land8", ["1", "0"])
@pytest.mark.parametrize("form", list(FORMS))
def test_steady_plan_path(engine_factory, oracle, monkeypatch, zone_bits, form, land8):
    """4096 pingers x 5 pings, 8 steps, in the three launch forms."""
    split, fuse = FORMS[form]
    monkeypatch.setenv("PONYC_AMD_SPLIT_PLAN", split)
    monkeypatch.setenv("PONYC_AMD_FUSE", fuse)
    monkeypatch.setenv("PONYC_AMD_LAND8", land8)
    g, o = _both(engine_factory, oracle, lambda e: W.ubench(e, 4096, 5, 100), W.ubench_result,
                 run_steps=8)
    _assert_same(g, o)
    d = g[1]["debug"]
    assert d["zone_bits"] == zone_bits and d["plan_zones"] > 0
    assert (d["land8_records"] > 0) == (land8 == "1"), d


def test_both_lanes_and_grow(engine_factory, oracle, zone_bits):
    """A mailbox capacity of 1: a zone holds as many records as it has pingers,
    so the first step's chunks reach past a zone's capacity (holes in the
    lane, the 16-byte route, a halted step, the host's expand and grow). Host
    pings with another argument then land 16-byte records in zones that also
    receive compact ones."""
    def setup(e):
        return W.ubench(e, 6144, 1, 1000, mailbox_cap=1)

    e = engine_factory()
    we, wo = setup(e), setup(oracle)
    for k in range(4):
        assert e.run(2) == oracle.run(2)
        to = np.arange(0, 6144, 3, dtype=np.uint64)
        for x in (e, oracle):
            W._sendv(x, W._msgs(wo["first"] + to, W.PINGER_PING, 7 + k))
    assert e.run(3) == oracle.run(3)
    np.testing.assert_array_equal(W.ubench_result(e, we), W.ubench_result(oracle, wo))
    _totals(e, oracle)
    d = e.debug_info()
    assert d["fixups"] > 0 and d["plan_zones"] > 0 and d["land8_records"] > 0, d


def test_sparse_tail(engine_factory, oracle, zone_bits):
    """run_fixed(k), then run() on the small-step path: 500 pings among 4096
    pingers are few enough for k_sparse, but run_fixed's steps are zone steps
    that plan and leave them in the compact lane, which the host expands in
    front of k_sparse."""
    def setup(x):
        w = W.ubench(x, 4096, 0, 1000)
        to = np.arange(0, 4000, 8, dtype=np.uint64)
        W._sendv(x, W._msgs(w["first"] + to, W.PINGER_PING, 42))
        return w

    e = engine_factory()
    we, wo = setup(e), setup(oracle)
    e.run_fixed(3)
    before = e.debug_info()
    assert before["plan_zones"] > 0 and before["land8_records"] > 0, before
    assert before["sparse_steps"] == 0, before
    assert e.run(5) == 5 and oracle.run(8) == 8
    np.testing.assert_array_equal(W.ubench_result(e, we), W.ubench_result(oracle, wo))
    _totals(e, oracle)
    d = e.debug_info()
    assert d["sparse_launches"] > 0 and d["sparse_steps"] == 5, d
    assert d["plan_zones"] == before["plan_zones"], d


def _burst_after_plan_steps(e, oracle, n, initial, mailbox_cap):
    """Plan steps first, so that compact records are pending; then 120 host
    pings to one pinger, more than its batch of 100: its zone is not `fast`,
    leaves the plan path with compact mail, expands it, and carries the
    actor's remainder over."""
    we = W.ubench(e, n, initial, 1000, mailbox_cap=mailbox_cap)
    wo = W.ubench(oracle, n, initial, 1000, mailbox_cap=mailbox_cap)
    assert e.run(3) == oracle.run(3)
    d0 = e.debug_info()
    assert d0["plan_zones"] == 3 * d0["zones"] and d0["land8_records"] > 0, d0
    for x in (e, oracle):
        W._sendv(x, W._msgs(np.full(120, wo["first"], dtype=np.uint64), W.PINGER_PING, 9))
    assert e.run(4) == oracle.run(4)
    np.testing.assert_array_equal(W.ubench_result(e, we), W.ubench_result(oracle, wo))
    _totals(e, oracle)
    d = e.debug_info()
    # the burst's zone step, and the step that ran its carried mail, did not plan
    assert d["plan_zones"] <= 7 * d["zones"] - 2, (d0, d)
    assert d["land8_records"] > d0["land8_records"]
    assert d["fixups"] == 0, d
    return d


def test_carried_mail(engine_factory, oracle, zone_bits):
    """6144 pingers x 3: the general path reads expanded records beside the
    burst's 16-byte ones and leaves carried mail."""
    _burst_after_plan_steps(engine_factory(), oracle, 6144, 3, 0)


def test_mail_past_index_cap(engine_factory, oracle, zone_bits):
    """9 pings a pinger: a zone's mail (18,432 records at 2048-actor zones,
    36,864 at 4096) is past kIdxCap, so the plan path counts both lanes in the
    unindexed loop, and the burst's zone expands the lane for the scratch
    path."""
    d = _burst_after_plan_steps(engine_factory(), oracle, 4096, 9, 16)
    assert d["land8_records"] > 3 * 16384


def test_second_table_after_plan_steps(engine_factory, oracle, zone_bits, monkeypatch):
    """FIFO sinks and sources created after three plan steps: the step entry
    changes, the pending compact records are expanded and delivered, and the
    lane stays unused from then on. (The mix runs on the compiled-in any-mix
    kernel: building its run-time compiled step takes 15 s and is not what
    this test is about.)"""
    monkeypatch.setenv("PONYC_AMD_JIT", "0")
    e = engine_factory()
    we, wo = W.ubench(e, 4096, 3, 12), W.ubench(oracle, 4096, 3, 12)
    assert e.run(3) == oracle.run(3)
    taken = e.debug_info()["land8_records"]
    assert taken > 0
    fe = W.fifo(e, sources=16, sinks=4, bursts=3, m=2, sink_type=1, src_type=2)
    fo = W.fifo(oracle, sources=16, sinks=4, bursts=3, m=2, sink_type=1, src_type=2)
    assert e.run() == oracle.run()
    np.testing.assert_array_equal(W.ubench_result(e, we), W.ubench_result(oracle, wo))
    np.testing.assert_array_equal(W.fifo_result(e, fe), W.fifo_result(oracle, fo))
    _totals(e, oracle)
    assert e.debug_info()["land8_records"] == taken


def _two_ranks(case, monkeypatch, bits="11", land8="1"):
    monkeypatch.setenv("PONYC_AMD_ZONE_BITS", bits)
    monkeypatch.setenv("PONYC_AMD_LAND8", land8)
    out = _launch("mr_land8_worker.py", 2, case)
    line = [l for l in out.splitlines() if l.startswith("MR_RESULT ")]
    assert line, out[-2000:]
    r = json.loads(line[-1][len("MR_RESULT "):])
    assert r["dropped"] == 0, r
    assert r["state_equal"], r
    for k in ("steps", "delivered", "sent", "pending"):
        assert r[k][0] == r[k][1], (k, r)
    assert r["by_type"] and r["remote"] > 0, r
    assert all(p > 0 for p in r["plan_zones"]), r
    return r


@pytest.mark.parametrize("land8", ["1", "0"])
@pytest.mark.parametrize("bits", ["11", "12"])
def test_two_ranks(monkeypatch, bits, land8):
    """Two ranks on one GPU over the host transport: a zone's records from its
    own rank come through the compact lane, the peer's as exchange records
    (`remote`) landed 16-byte in the same zones."""
    r = _two_ranks("steady", monkeypatch, bits, land8)
    assert all((n > 0) == (land8 == "1") for n in r["land8_records"]), r
    assert r["fixups"] == [0, 0], r


@pytest.mark.parametrize("bits", ["11", "12"])
def test_two_ranks_grow(monkeypatch, bits):
    """A mailbox capacity of 1 on two ranks: the two lanes together pass a
    zone's capacity, the next step halts on every rank, and all ranks expand
    and grow together."""
    r = _two_ranks("grow", monkeypatch, bits)
    assert all(n > 0 for n in r["land8_records"]), r
    assert all(n > 0 for n in r["fixups"]), r


def test_two_ranks_fixed(monkeypatch):
    """run_fixed, run, run_fixed on two ranks."""
    r = _two_ranks("fixed", monkeypatch)
    assert all(n > 0 for n in r["land8_records"]), r


def test_fixed_run_fixed_and_buffers(oracle):
    """run_fixed, run, run_fixed; after shutdown no device buffer is left."""
    from conftest import make_engine
    e = make_engine()
    try:
        we, wo = W.ubench(e, 4096, 3, 30), W.ubench(oracle, 4096, 3, 30)
        e.run_fixed(3)
        assert e.run(2) == oracle.run(5) - 3
        e.run_fixed(2)
        e.sync()
        oracle.run(2)
        np.testing.assert_array_equal(W.ubench_result(e, we), W.ubench_result(oracle, wo))
        _totals(e, oracle)
        assert e.debug_info()["land8_records"] > 0
    finally:
        e.shutdown()
    assert live_buffers()[0] == 0
