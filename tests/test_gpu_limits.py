"""GPU parity at the widths of the fields every message is packed into, and
GPU_ACTOR_ERANGE one past them.

A sender's sequence number is 16 bits of ZRec.w0 / ORec.w (seq << 16 | beh <<
12 | local), of the sort key (from << 16 | seq), of the host-port key (step |
self << 16 | seq) and of the spawn key (type << 52 | self << 20 | seq << 4 |
beh); the two-pass pinger path packs a zone's per-bucket counts in 16-bit
halves and plans a zone only when its mail is below seq_max. Every case here
drives one of those fields to its last value (kSeqMax - 1 = 0xFFFD on one
rank) and compares the engine bit for bit with the CPU oracle, which has no
such limit; the cases one past it expect ERANGE, a clean shutdown and a
following engine that equals the oracle again. Each case asserts from
debug_info() the path its parameters were meant to take, so a silent
fallback does not pass as coverage. (tests/mr_worker.py fifo_seq_max* and
tests/mr_erange_worker.py are the two-rank side: 16,382 and the XRec split.)

Highest sequence number reached per format: ZRec/ORec/sort key 0xFFFD
(test_fifo_seq_limit*), host key 0xFFFD (test_host_port_high_seq), spawn key
0xFFFD (test_spawn_high_seq)."""
import json

import numpy as np
import pytest

import host_port_checks as H
from ponyc_amd import program as P
from ponyc_amd import workloads as W
from ponyc_amd.engine import GpuActorError, HT_FIFO_SINK, HT_PROGRAM, live_buffers
from test_gpu_host_port import _run as _host_run, _check as _host_check
from test_gpu_parity import _both, _assert_same
from test_gpu_plan_pairs import plan_zones
from test_gpu_split import FORMS
from test_multirank import _launch

pytestmark = pytest.mark.gpu

SEQ_MAX = 0xFFFE            # engine_dev.h kSeqMax: sends per actor per superstep, one rank
ERANGE = -7


def _env(monkeypatch, bits=None, hot=None, sparse=None, jit=None):
    if bits is not None:
        monkeypatch.setenv("PONYC_AMD_ZONE_BITS", bits)
    if hot is not None:
        monkeypatch.setenv("PONYC_AMD_HOT", hot)
    if sparse is not None:
        if sparse:
            monkeypatch.delenv("GPA_NO_SPARSE", raising=False)
        else:
            monkeypatch.setenv("GPA_NO_SPARSE", "1")
    if jit is not None:
        monkeypatch.setenv("PONYC_AMD_JIT", jit)


def _assert_sparse(d, sparse):
    if sparse:
        assert d["sparse_steps"] > 0, d
    else:
        assert d["sparse_steps"] == 0, d


# ---- 1. a sender's sequence numbers up to the limit, one rank ----------------------------
@pytest.mark.parametrize("batch", [1000, 262144])
@pytest.mark.parametrize("sparse", [True, False])
@pytest.mark.parametrize("hot", ["0", "1"])
@pytest.mark.parametrize("bits", ["11", "12"])
def test_fifo_seq_limit(engine_factory, oracle, monkeypatch, bits, hot, sparse, batch):
    """Two sources send exactly kSeqMax PUSHes each in one behaviour (seq
    0..0xFFFD, no self-send) to one sink whose fold is order-sensitive and
    which counts FIFO violations: equal to the oracle only if delivery is in
    canonical (sender, seq) order over all 16 bits of seq. The first step (2
    messages) runs in k_sparse unless GPA_NO_SPARSE=1, so the sends are stamped
    by both kernels; the group of 131,068 is above kHotMin (k_hot's bins with
    PONYC_AMD_HOT=1, the workgroup's sorts with 0); batch 1000 carries a
    backlog for ~132 steps (the carry sort and kCarryRun's samples see the
    high keys), 262144 runs the whole group in one step."""
    _env(monkeypatch, bits=bits, hot=hot, sparse=sparse)
    g, o = _both(engine_factory, oracle,
                 lambda e: W.fifo(e, sources=2, sinks=1, bursts=1, m=SEQ_MAX, batch=batch,
                                  mailbox_cap=16),
                 W.fifo_result)
    _assert_same(g, o)
    assert g[2][2].sum() == 0                          # the sink's FIFO violations
    assert g[1]["sent"] == 2 * SEQ_MAX == 131068
    assert g[1]["delivered"] == 2 * SEQ_MAX + 2 == 131070
    d = g[1]["debug"]
    assert d["zone_bits"] == int(bits)
    assert d["hot_on"] == int(hot) and d["hot_missed"] == 0, d
    _assert_sparse(d, sparse)
    assert d["fixups"] > 0, d                          # the sink's zone of 16 grew
    if batch > 2 * SEQ_MAX:
        assert g[0] == 2


@pytest.mark.parametrize("sparse", [True, False])
@pytest.mark.parametrize("bits", ["11", "12"])
def test_fifo_seq_limit_self_send_last(engine_factory, oracle, monkeypatch, bits, sparse):
    """65,533 PUSHes and then the BURST self-send: the self-send takes the
    sender's last sequence number, 0xFFFD, in the first burst; the sinks have
    priority and drain everything at once."""
    _env(monkeypatch, bits=bits, sparse=sparse)
    g, o = _both(engine_factory, oracle,
                 lambda e: W.fifo(e, 3, 2, 2, SEQ_MAX - 1, sink_priority=1), W.fifo_result)
    _assert_same(g, o)
    assert g[2][2].sum() == 0
    assert g[0] == 3
    assert g[1]["sent"] == 3 * (2 * (SEQ_MAX - 1) + 1) == 393201
    d = g[1]["debug"]
    assert d["zone_bits"] == int(bits) and d["hot_missed"] == 0, d
    _assert_sparse(d, sparse)
    assert d["fixups"] > 0, d


# ---- 2. one past the limit: ERANGE -----------------------------------------------------------
OVER = {
    # 65,535 PUSHes: the last one has no sequence number
    "pushes": lambda e: W.fifo(e, sources=2, sinks=1, bursts=1, m=SEQ_MAX + 1, mailbox_cap=16),
    # 65,534 PUSHes take them all: the self-send has none
    "self_send": lambda e: W.fifo(e, 3, 2, 2, SEQ_MAX, sink_priority=1),
}


@pytest.mark.parametrize("sparse", [True, False])
@pytest.mark.parametrize("bits", ["11", "12"])
@pytest.mark.parametrize("shape", list(OVER))
def test_fifo_seq_over_limit(engine_factory, oracle, monkeypatch, shape, bits, sparse):
    """One send past kSeqMax in one behaviour: gpu_actor_run returns
    GPU_ACTOR_ERANGE (include/gpu_actor.h) — not EMAILBOX, not a wrong result,
    not a hang — from k_sparse's check (the first step, unless GPA_NO_SPARSE=1)
    or k_step's. The error is sticky (gpu_actor_sync returns it), the engine
    shuts down cleanly, and a fresh engine in the same process equals the
    oracle at the limit. (The oracle has no limit: no state is compared for
    the failed engine.)"""
    _env(monkeypatch, bits=bits, sparse=sparse)
    e = engine_factory()
    OVER[shape](e)
    with pytest.raises(GpuActorError) as ei:
        e.run()
    assert ei.value.code == ERANGE
    # which kernel's check fired. (gpu_actor_debug_info is a diagnostic export
    # outside include/gpu_actor.h: this relies on it not returning the sticky
    # error, as engine.hip has it; the header's promises are the lines around)
    _assert_sparse(e.debug_info(), sparse)
    with pytest.raises(GpuActorError) as ei:
        e.sync()
    assert ei.value.code == ERANGE
    e.shutdown()
    assert live_buffers() == (0, 0)
    g, o = _both(engine_factory, oracle,
                 lambda e: W.fifo(e, sources=2, sinks=1, bursts=1, m=SEQ_MAX, batch=262144,
                                  mailbox_cap=16),
                 W.fifo_result)
    _assert_same(g, o)
    assert g[2][2].sum() == 0 and g[1]["sent"] == 2 * SEQ_MAX


def test_seq_over_limit_two_ranks():
    """16,383 sends in one behaviour with n_ranks = 2 (kXSeqMax = 16,382): the
    rank of every sender that ran out reports ERANGE from gpu_actor_run. The
    error is each rank's own (engine.hip check_sticky reads the rank's own
    counters; the run's collectives do not depend on it), so no rank waits for
    another in a collective: with a sender on each rank both report it, with
    the only sender on rank 1 that rank does, and both ranks finish. What
    rank 0 returns in that case is left unasserted on purpose: the header
    does not say what a rank without an overflowing actor reports."""
    out = _launch("mr_erange_worker.py", 2)
    line = [l for l in out.splitlines() if l.startswith("MR_RESULT ")]
    assert line, out[-2000:]
    r = json.loads(line[-1][len("MR_RESULT "):])
    assert r["both"] == [ERANGE, ERANGE]
    assert r["one"][1] == ERANGE
    assert r["live"] == [[0, 0], [0, 0]]


# ---- 4. host-port and spawn keys at high seq -------------------------------------------------
# emitter_program's BURST loop runs 14 instructions per send with one port, so
# GPU_ACTOR_PROG_MAX_STEPS = 4096 allows m <= 291; 217 * 302 = 65,534 = kSeqMax:
# each of the 2 emitters handles 302 BURST(217) in one step (batch 512 >= 302)
# and sends seq 0..0xFFFD to the port.
HOST_HIGH = dict(n=2, ports=(1,), bursts=1, m=217, batch=512, initial=302)


@pytest.mark.parametrize("jit", ["1", "0"])
def test_host_port_high_seq(monkeypatch, jit):
    _env(monkeypatch, jit=jit)
    r = _host_run(HOST_HIGH)
    _host_check(r, HOST_HIGH)
    msgs, w = r["msgs"], r["w"]
    assert r["steps"] == 1 and msgs.shape[0] == 2 * SEQ_MAX
    assert len(set(msgs["step"].tolist())) == 1
    for k in range(2):
        mine = msgs[msgs["from"] == w["first"] + k]
        # each sender's messages in sequence order, over all 16 bits of seq
        np.testing.assert_array_equal(mine["seq"], np.arange(SEQ_MAX, dtype=np.uint32))
        np.testing.assert_array_equal(mine["arg"],
                                      (np.uint64(k) << np.uint64(32)) |
                                      np.arange(1, SEQ_MAX + 1, dtype=np.uint64))
    # the list is sender-major: the first sender's whole run, then the second's
    assert (msgs["from"][:SEQ_MAX] == w["first"]).all()
    assert (r["dbg"]["jit"] == 1) == (jit == "1"), r["dbg"]


SPAWN_K, SPAWN_COPIES = 60, 1057       # (60 + 2) * 1057 = 65,534 = kSeqMax
SPAWN_PARENTS = 2


def spawner_program(type_id: int) -> np.ndarray:
    """Behaviour 0 WORK: param 1 times, bump c (word 1) and SEND behaviour 0
    with index << 32 | c to the sink param 0; then SPAWN two children of the
    own type whose constructor (behaviour 1) gets index << 32 | ordinal
    (word 2, bumped per spawn). Behaviour 1: word 0 = the argument, word 3 = 1.
    index = self - param 3."""
    p = P.Program()
    p.behaviour(0)
    p.ldp(11, 3)
    p.sub(11, P.R_SELF, 11)
    p.ldi(12, 32)
    p.shl(11, 11, 12)                   # index << 32
    p.ldp(12, 1)                        # sends left
    p.ldp(13, 0)                        # the sink
    p.label("loop")
    p.jz(12, "spawn")
    p.addi(1, 1, 1)
    p.or_(14, 11, 1)
    p.send(13, 0, 14)
    p.addi(12, 12, -1)
    p.jmp("loop")
    p.label("spawn")
    for _ in range(2):
        p.addi(2, 2, 1)
        p.or_(14, 11, 2)
        p.spawn(type_id, 1, 14)
    p.halt()
    p.behaviour(1)
    p.mov(0, P.R_ARG)
    p.ldi(3, 1)
    p.halt()
    return p.assemble()


def fold_sink_program() -> np.ndarray:
    """The FIFO sink's PUSH as a program, for senders of index 0 and 1:
    word 0 h = (h ^ arg) * 0x100000001b3 (order-sensitive, from 0), word 1 the
    messages, word 2 FIFO violations (the low 32 bits of arg must follow the
    sender's last: words 3 and 4)."""
    p = P.Program()
    p.behaviour(0)
    p.ldi(11, 32)
    p.shr(12, P.R_ARG, 11)              # the sender's index
    p.ldi(14, -1)
    p.shr(14, 14, 11)
    p.and_(13, P.R_ARG, 14)             # its counter
    p.jnz(12, "s1")
    p.addi(15, 3, 1)
    p.eq(15, 15, 13)
    p.jnz(15, "ok0")
    p.addi(2, 2, 1)
    p.label("ok0")
    p.mov(3, 13)
    p.jmp("fold")
    p.label("s1")
    p.addi(15, 4, 1)
    p.eq(15, 15, 13)
    p.jnz(15, "ok1")
    p.addi(2, 2, 1)
    p.label("ok1")
    p.mov(4, 13)
    p.label("fold")
    p.addi(1, 1, 1)
    p.xor(0, 0, P.R_ARG)
    p.ldi(14, 1)
    p.ldi(15, 40)
    p.shl(14, 14, 15)
    p.addi(14, 14, 0x1b3)               # the FNV prime
    p.mul(0, 0, 14)
    p.halt()
    return p.assemble()


def spawn_programs():
    """[(type id, words)] of the all-program spawn world (scripts/jit_precompile.py)"""
    return [(0, fold_sink_program()), (1, spawner_program(1))]


def _spawn_world(e, sink_prog=False):
    n_children = SPAWN_PARENTS * SPAWN_COPIES * 2
    if sink_prog:
        e.type_register(0, 8, HT_PROGRAM)
        e.type_program(0, fold_sink_program())
    else:
        e.type_register(0, 11, HT_FIFO_SINK)
        e.type_param(0, 0, 1)
    e.type_config(0, 262144, 0)         # the sink folds a step's arrivals whole
    sink = e.create(0, 1)
    e.type_register(1, 8, HT_PROGRAM)
    e.type_program(1, spawner_program(1))
    e.type_config(1, 2048, 0)           # a parent runs all its copies in one step
    e.type_reserve(1, n_children)
    e.type_param(1, 0, sink)
    e.type_param(1, 1, SPAWN_K)
    first = e.create(1, SPAWN_PARENTS)
    e.type_param(1, 3, first)
    to = np.repeat(first + np.arange(SPAWN_PARENTS, dtype=np.uint64), SPAWN_COPIES)
    W._sendv(e, W._msgs(to, 0, 0))
    return {"first": first, "children": n_children}


def _spawn_result(e, w):
    return np.concatenate([e.state_read(0).ravel(), e.state_read(1).ravel(),
                           np.array([e.type_live(0), e.type_live(1)], dtype=np.uint64)])


@pytest.mark.parametrize("jit", ["1", "0"])
@pytest.mark.parametrize("sink", ["fifo", "program"])
def test_spawn_high_seq(engine_factory, oracle, monkeypatch, sink, jit):
    """Each of 2 parents handles 1,057 WORKs in one step: 60 sends to one sink
    and 2 spawns each, so a parent's spawns take seq 60, 61, 122, 123, ...
    65,532, 65,533 — every bit of the spawn key's seq field — between sends
    that fill the same 16 bits of the sort key. Ids are given in (creator,
    seq) order: child j's constructor argument names its parent and ordinal.
    sink "fifo": the compiled HT_FIFO_SINK table; the engine is then a mix of
    tables, and PONYC_AMD_JIT=1 means the any-mix kernel built for this mix
    (engine.hip plan_step, kind 2), in which the spawner still runs in the
    interpreter. sink "program": the same fold as a program, so every serial
    actor runs a program and PONYC_AMD_JIT=1 runs the step generated from the
    programs (kind 1): SPAWN and SEND at high seq in compiled program code."""
    _env(monkeypatch, jit=jit)
    made = []

    def factory(**kw):
        e = engine_factory(**kw)
        made.append(e)
        return e
    g, o = _both(factory, oracle, lambda e: _spawn_world(e, sink == "program"), _spawn_result)
    _assert_same(g, o)
    per = SPAWN_COPIES * 2
    st = made[0].state_read(1)
    assert made[0].type_live(1) == SPAWN_PARENTS + SPAWN_PARENTS * per
    want = np.concatenate([(np.uint64(k) << np.uint64(32)) | np.arange(1, per + 1, dtype=np.uint64)
                           for k in range(SPAWN_PARENTS)])
    np.testing.assert_array_equal(st[0][SPAWN_PARENTS:], want)
    assert (st[3][SPAWN_PARENTS:] == 1).all()
    sk = made[0].state_read(0)
    assert int(sk[1][0]) == SPAWN_PARENTS * SPAWN_COPIES * SPAWN_K and int(sk[2][0]) == 0
    assert g[1]["sent"] == SPAWN_PARENTS * SEQ_MAX
    d = made[0].debug_info()
    assert (d["jit_builds"] >= 1) == (jit == "1"), d
    if sink == "program":
        # the fold, worked out here: parent 0's 63,420 sends in order, then parent 1's
        h = 0
        for k in range(SPAWN_PARENTS):
            for c in range(1, SPAWN_COPIES * SPAWN_K + 1):
                h = ((h ^ (k << 32 | c)) * H.FNV_PRIME) & H.M64
        assert int(sk[0][0]) == h
        assert (d["jit"] == 1) == (jit == "1"), d      # the last step ran the programs' module


# ---- 5. zone mail at seq_max: the plan guard ---------------------------------------------------
def _zone_at(e, n, initial, extra):
    w = W.ubench(e, n, initial, budget=40)
    W._sendv(e, W._msgs(w["first"] + np.arange(extra, dtype=np.uint64), W.PINGER_PING, 42))
    return w


def _stepped(e, w, planned=None):
    """two single steps, then to quiescence"""
    steps = 0
    for _ in range(2):
        steps += e.run(1)
        if planned is not None:
            planned.append(plan_zones(e))
    steps += e.run()
    return steps, e.counts(), W.ubench_result(e, w)


@pytest.mark.parametrize("over", [0, 1])
@pytest.mark.parametrize("bits,n,initial,extra", [("11", 2048, 31, 2045), ("12", 4096, 15, 4093)])
@pytest.mark.parametrize("form", list(FORMS))
def test_plan_guard_at_seq_max(engine_factory, oracle, monkeypatch, form, bits, n, initial, extra,
                               over):
    """One zone of pingers whose mail is exactly seq_max - 1 (the two-pass
    path plans it: zone_dev.h `s_tot < c_eng.seq_max`; its packed 16-bit count
    halves and kPlain sends rest on that) and exactly seq_max (it must not).
    Every pinger holds initial or initial + 1 messages, under the batch and the
    budget, so step 1 forwards every message and step 2's zone mail is the same
    total. Unsplit, two launches and fused: the zone at the limit goes through
    PM 2 / zone_step_rest in each."""
    split, fuse = FORMS[form]
    monkeypatch.setenv("PONYC_AMD_SPLIT_PLAN", split)
    monkeypatch.setenv("PONYC_AMD_FUSE", fuse)
    _env(monkeypatch, bits=bits)
    mail = n * initial + extra + over
    assert mail == SEQ_MAX - 1 + over
    e = engine_factory()
    planned = []
    se, ce, re = _stepped(e, _zone_at(e, n, initial, extra + over), planned)
    ce["debug"] = e.debug_info()
    so, co, ro = _stepped(oracle, _zone_at(oracle, n, initial, extra + over))
    _assert_same((se, ce, re), (so, co, ro))
    assert ce["debug"]["zone_bits"] == int(bits) and ce["debug"]["zones"] == 1
    assert planned == ([0, 0] if over else [1, 2]), planned


@pytest.mark.parametrize("extra,plans", [(4090, True), (4092, False)])
def test_plan_guard_two_ranks(extra, plans):
    """4,096 pingers on two ranks, 7 pings each and one more to the first
    `extra` ids: each rank's zone holds 14,336 + extra / 2 = 16,381 (below
    kXSeqMax: planned) or 16,382 (not planned) in the first step."""
    out = _launch("mr_plan_pairs_worker.py", 2, str(extra))
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
    # zone steps that planned in the first step, summed over the ranks
    assert (r["plan_zones_first"] > 0) if plans else (r["plan_zones_first"] == 0), r
