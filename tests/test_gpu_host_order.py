"""GPU parity where the inputs come from the host: the host as one of the
senders of an order-sensitive arrival group, and small id spaces
(gpu_actor_config_t.max_actors).

A. k_inject (csrc/zone_dev.h) stamps a host message with from = 0xFF000000 |
hseq >> 16 and seq = hseq & 0xFFFF. A group that holds a host record and an
actor record has a 32-bit sender range, so its compressed key (coop_sort_group,
k_hot P2: (from - fmin) << sbits | seq) is up to 48 bits wide where actor-only
groups stay below 43: exactly 64 bits of item on the LDS-index path, and past
64 on the scratch path, where the workgroup refuses the sort and one lane
orders the group (drain_zone's key window, AccS::sort). The scenarios
(tests/host_order.py, each with its arithmetic) put such groups on every one
of those paths, with FIFO sinks whose fold is order-sensitive, and compare
step count, whole sink state and the counters with the CPU oracle, which
appends host sends in call order. tests/test_host_order_oracle.py shows that
the fold does tell the orders apart. The largest refused group here is 276
records (at most 276^2 / 2 = 38,088 record moves by its lane, against the
5 * 10^5 allowed); none is built that is both past 1,024 and carried.

C. max_actors fixes the host-port key shift (16 + bits(max_actors - 1)),
host_step_room(), the trigger arrays and the ERANGE bound of
gpu_actor_create / gpu_actor_type_reserve; nothing here goes above 1 << 22."""
import numpy as np
import pytest

import host_order as HO
import host_port_checks as H
from ponyc_amd import program as P
from ponyc_amd import workloads as W
from ponyc_amd.engine import (Engine, GpuActorError, HT_HOST_PORT, HT_PROGRAM, HT_RING,
                              live_buffers)
from test_gpu_edges import PORT_WORLD
from test_gpu_limits import _env, _assert_sparse
from test_gpu_parity import _both, _assert_same

pytestmark = pytest.mark.gpu

ERANGE = -7
BITS = ["11", "12"]


def _parity(engine_factory, oracle, scenario, result=W.fifo_result, **eng_kw):
    """The scenario on the engine and on the oracle, then both to quiescence."""
    g, o = _both(engine_factory, oracle, scenario, result, **eng_kw)
    _assert_same(g, o)
    assert g[1]["pending"] == 0
    return g


# ---- A. host and actor senders in one ordered group ------------------------------------------
@pytest.mark.parametrize("batch", [100, 1 << 20])
@pytest.mark.parametrize("bits", BITS)
def test_index_path_64_bit_item(engine_factory, oracle, monkeypatch, bits, batch):
    """Case 1 (host_order.idx64): LDS-index path, kbits = 48 + pay 16 = 64:
    coop_msd_sort(ia, ib, g, 16, 48). 8 groups of 204 (<= kMaxBig = 32 big
    groups: all sorted by the workgroup); the zone lands 1,632 <= kIdxCap.
    Batch 100 carries 104 of each group, 2^20 runs it whole."""
    _env(monkeypatch, bits=bits)
    g = _parity(engine_factory, oracle, lambda e: HO.idx64(e, batch=batch))
    assert g[2][2].sum() == 0                          # the sinks' FIFO violations
    assert g[2][1][:8].tolist() == [204] * 8
    assert g[1]["delivered"] == 8 + 32768 + 8 * 204    # the BURSTs, the fillers, the groups
    assert g[1]["debug"]["zone_bits"] == int(bits)
    assert g[0] == (3 if batch == 100 else 1)           # steps after the first


@pytest.mark.parametrize("batch", [512, 100])
@pytest.mark.parametrize("bits", BITS)
def test_scratch_path_sort_refused(engine_factory, oracle, monkeypatch, bits, batch):
    """Case 2 (host_order.scratch, 96 x 264): scratch path (25,728 landed
    records: above kIdxCap of either geometry, below kHotMin), kbits = 47 +
    pay 20 = 67: refused. Batch 512 >= 268: the key window; batch 100:
    AccS::sort, then carried mail over 3 steps. PONYC_AMD_HOT=0 keeps k_hot
    out whatever the engine's default."""
    _env(monkeypatch, bits=bits, hot="0")
    g = _parity(engine_factory, oracle, lambda e: HO.scratch(e, batch=batch))
    assert g[2][2].sum() == 0
    assert g[2][1][:96].tolist() == [268] * 96
    d = g[1]["debug"]
    assert d["zone_bits"] == int(bits) and d["hot_on"] == 0, d
    assert g[0] == (1 if batch == 512 else 3)


@pytest.mark.parametrize("batch", [512, 100])
@pytest.mark.parametrize("hot", ["1", "0"])
@pytest.mark.parametrize("bits", BITS)
def test_hot_zone(engine_factory, oracle, monkeypatch, bits, hot, batch):
    """Case 3 (host_order.scratch, 128 x 260, mailboxes of 16 as
    test_gpu_backpressure.py's _hot_zones_60_to_70): the zone lands 33,792 >=
    kHotMin and its capacity is 32,768 or 65,536, so min(land_n, zcapz) >=
    kHotMin. PONYC_AMD_HOT=1: k_hot bins on the 48-bit compressed key (the
    host's 260 records of a group share the top 12 bits: one bin, sorted by
    one thread, 260^2 / 2 = 33,800 moves); 0: the workgroup's own scratch
    path, the sort refused (67 bits), groups of 264 <= 1,024 ordered by the
    lane."""
    _env(monkeypatch, bits=bits, hot=hot)
    g = _parity(engine_factory, oracle,
                lambda e: HO.scratch(e, batch=batch, hot=128, per=260, cap=16), mailbox_cap=16)
    assert g[2][2].sum() == 0
    assert g[2][1][:128].tolist() == [264] * 128
    d = g[1]["debug"]
    assert d["zone_bits"] == int(bits)
    assert d["hot_on"] == int(hot) and d["hot_missed"] == 0, d


@pytest.mark.parametrize("form,batch", [("alone", 512), ("sources", 100), ("staged", 512)])
@pytest.mark.parametrize("hot", ["1", "0"])
@pytest.mark.parametrize("bits", BITS)
def test_hseq_wrap(engine_factory, oracle, monkeypatch, bits, hot, form, batch):
    """Case 4 (host_order.wrap): 69,632 host PUSHes in one window; every
    sink's 272 host records straddle hseq 65,536, where seq restarts at 0
    under from 0xFF000001. "alone": kbits = 17, sorted by the workgroup (or
    k_hot's bins); "sources" and "staged": an actor sender in each group,
    kbits = 48 — k_hot's bins, or refused on the scratch path: 276 records in
    the key window (batch 512) or AccS::sort (batch 100). "staged" builds the
    window from sendv, 3,000 single sends across the wrap, sendv: the header
    promises call order."""
    _env(monkeypatch, bits=bits, hot=hot)
    g = _parity(engine_factory, oracle, lambda e: HO.wrap(e, form=form, batch=batch, cap=16),
                mailbox_cap=16)
    assert g[2][2].sum() == 0
    per = HO.WRAP_PER + (0 if form == "alone" else 4)
    assert g[2][1][:HO.WRAP_SINKS].tolist() == [per] * HO.WRAP_SINKS
    d = g[1]["debug"]
    assert d["zone_bits"] == int(bits)
    assert d["hot_on"] == int(hot) and d["hot_missed"] == 0, d


@pytest.mark.parametrize("sparse", [True, False])
def test_small_step_path(engine_factory, oracle, monkeypatch, sparse):
    """Case 5 (host_order.small_step): 416 pending records, 50 a sink: k_sparse
    ranks by slot << 32 | sender and then seq, the host's from in the low
    word; with GPA_NO_SPARSE=1 the zone step takes the same mail."""
    _env(monkeypatch, sparse=sparse)
    g = _parity(engine_factory, oracle, HO.small_step)
    assert g[2][2].sum() == 0
    assert g[2][1].tolist() == [60] * 8
    _assert_sparse(g[1]["debug"], sparse)


def test_muted_receiver(engine_factory, oracle):
    """Case 6 (host_order.muted): a muted actor's arrivals, mixed from itself
    and the host, are sorted for the carry without draining (zone_actor's
    `stays`). The oracle confirms the shape: beside the 7 overloaded sinks,
    sources are muted when the host sends."""
    def scenario(e):
        w = HO.muted(e)
        if hasattr(e, "trig_count"):
            assert e.trig_count() > 7
        return w
    _parity(engine_factory, oracle, scenario, mailbox_cap=16)


def test_new_window_over_carried_mail(engine_factory, oracle):
    """Case 7 (host_order.two_windows): hseq restarts at 0 after each run, so
    the second window's keys are below those of the first window's carried
    records, which it must follow."""
    g = _parity(engine_factory, oracle, HO.two_windows)
    assert g[2][2].sum() == 0
    assert g[2][1][:8].tolist() == [454] * 8


@pytest.mark.parametrize("jit", ["1", "0"])
def test_program_receiver(engine_factory, oracle, monkeypatch, jit):
    """Case 9 (host_order.scratch_programs): the case-2 drain (scratch path,
    sort refused, batch 100: AccS::sort and carried mail) with every actor a
    program: the step compiled at run time from the programs
    (PONYC_AMD_JIT=1) and the interpreter (0)."""
    _env(monkeypatch, hot="0", jit=jit)
    g = _parity(engine_factory, oracle, HO.scratch_programs,
                result=lambda e, w: np.concatenate([e.state_read(0), e.state_read(1)], axis=1))
    assert g[2][1][:96].tolist() == [268] * 96
    d = g[1]["debug"]
    assert (d["jit"] == 1) == (jit == "1"), d
    # sink 0's fold, worked out here: its source's 4 PUSHes, then the host's 264
    h = 0
    for a in [(0 << 32) | c for c in range(1, 5)] + [(96 << 32) | k for k in range(1, 265)]:
        h = ((h ^ a) * H.FNV_PRIME) & H.M64
    assert int(g[2][0][0]) == h


# ---- C. max_actors -----------------------------------------------------------------------------
# PORT_WORLD's shape with 3 bursts: three steps, so that run_fixed(3) leaves
# three steps' keys for one collection
TOP_WORLD = dict(PORT_WORLD, bursts=3)


def _top_world(e, kw):
    """TOP_WORLD with the emitters at the top of the id space: the port first
    (id 0), then the emitters (ids 1..n)."""
    n, m = kw["n"], kw["m"]
    e.type_register(1, 11, HT_HOST_PORT)
    pfirst = e.create(1, 1)
    e.type_register(0, 8, HT_PROGRAM)
    e.type_program(0, P.emitter_program())
    first = e.create(0, n)
    e.type_param(0, 0, pfirst)
    e.type_param(0, 1, 1)
    e.type_param(0, 2, 1)                      # (the modulus' magic: unused with one port)
    e.type_param(0, 3, first)
    e.type_param(0, 4, kw["bursts"])
    e.sendv(W._msgs(first + np.arange(n, dtype=np.uint64), 0, m))
    return {"first": first, "n": n, "port_first": pfirst, "n_ports": 1, "ids": first + n}


def _as_reference_ids(msgs, w, ref_w):
    """The received list with the ids of W.emitter's layout (emitters first),
    which host_port_checks' stand-ins use; the emitters' order is kept."""
    out = msgs.copy()
    out["from"] = msgs["from"] - w["first"] + ref_w["first"]
    out["to"] = msgs["to"] - w["port_first"] + ref_w["port_first"]
    return out


def _ports_run(max_actors, fixed):
    with Engine(max_actors=max_actors) as e:
        w = _top_world(e, TOP_WORLD)
        assert w["ids"] == TOP_WORLD["n"] + 1
        if fixed:
            e.run_fixed(fixed)
            assert e.recv_pending() > 0        # the observing call collects the steps' keys
            steps = fixed
        else:
            steps = e.run()
        msgs, counts, emit = e.recv(), e.counts(), e.state_read(0)
    H.check_structure(msgs, w)
    assert int(msgs["from"].max()) == w["ids"] - 1
    ref = _as_reference_ids(msgs, w, H.stand_in(TOP_WORLD, "A")["w"])
    H.check_a(ref, steps, counts, emit, TOP_WORLD)
    H.check_b(ref, TOP_WORLD)
    return steps, msgs.tobytes()


def test_host_ports_under_three_id_spaces():
    """The host-port key is step << kshift | from << 16 | seq with kshift = 16
    + bits(max_actors - 1): the last emitter's id is max_actors - 1 when
    max_actors is the world's id count (101, not a power of two: kshift 23),
    then 128 (kshift 23 from the other side) and 1 << 22 (kshift 38). run():
    one collection per step; run_fixed(k) and an observing call: k steps' keys
    sorted in one collection, above kshift. The same bytes all six times."""
    ids = TOP_WORLD["n"] + 1
    assert ids & (ids - 1)
    seen = set()
    k = None
    for max_actors in (ids, 1 << (ids - 1).bit_length(), 1 << 22):
        steps, raw = _ports_run(max_actors, 0)
        k = k or steps
        assert steps == k == TOP_WORLD["bursts"]      # a burst a step: several steps' keys
        seen.add(raw)
        assert _ports_run(max_actors, k) == (k, raw)
    assert len(seen) == 1


def test_create_erange(engine_factory, oracle):
    """One actor more than max_actors allows, and a count + reserve that
    crosses it: ERANGE, nothing created; the engine then runs a small world
    equal to the oracle and shuts down holding nothing."""
    e = engine_factory(max_actors=1000)
    e.type_register(0, 4, HT_RING)
    with pytest.raises(GpuActorError) as ei:
        e.create(0, 1001)
    assert ei.value.code == ERANGE
    e.type_register(1, 5, W.HT_SPREADER)
    e.type_reserve(1, 999)
    with pytest.raises(GpuActorError) as ei:
        e.create(1, 2)
    assert ei.value.code == ERANGE
    with pytest.raises(GpuActorError) as ei:
        e.type_reserve(1, 1001)
    assert ei.value.code == ERANGE
    e.type_reserve(1, 0)
    e.type_param(0, 0, 700)
    we = W.ring(e, 100, 3, 50, type_id=2)
    first = e.create(0, 700)                   # ids 300..999: the last id max_actors - 1
    assert first == 300
    with pytest.raises(GpuActorError) as ei:
        e.create(1, 1)
    assert ei.value.code == ERANGE
    se, ce, re = e.run(), e.counts(), W.ring_result(e, we)
    wo = W.ring(oracle, 100, 3, 50, type_id=2)
    so, co = oracle.run(), oracle.counts()
    np.testing.assert_array_equal(re, W.ring_result(oracle, wo))
    assert se == so and ce["delivered"] == co["delivered"] and ce["sent"] == co["sent"]
    assert ce["dropped"] == 0 and ce["pending"] == 0
    e.shutdown()
    assert live_buffers() == (0, 0)


def test_run_fixed_past_host_step_room():
    """With ports, run_fixed(host_step_room() + 1) returns ERANGE before any
    launch: room = min(2^(64 - kshift), 2^31) = 2^22 at the default
    max_actors (2^26: kshift 42)."""
    with Engine() as e:
        H.world(e, PORT_WORLD)
        before = e.counts()
        with pytest.raises(GpuActorError) as ei:
            e.run_fixed((1 << 22) + 1)
        assert ei.value.code == ERANGE
        after = e.counts()
        assert after["steps"] == before["steps"] == 0
        assert after["delivered"] == 0 and after["pending"] == before["pending"]


def test_benched_id_space(engine_factory, oracle):
    """bench.py's max_actors = n + 1024 (not a power of two) at a test's size:
    4,096 pingers, bit-exact."""
    g, o = _both(engine_factory, oracle, lambda e: W.ubench(e, 4096, 4, 32), W.ubench_result,
                 max_actors=4096 + 1024)
    _assert_same(g, o)
