"""Edge cases of the boundary on the GPU (the reference's own tests pin the
same corners of the runtime: nothing to run, zero-length sends, bad ids —
pony_sendv to a non-actor is impossible in Pony, so the C-ABI rejects it).
Every case goes through libgpuactor.so; state is compared with the oracle."""
import numpy as np
import pytest

import host_port_checks as H
from ponyc_amd import workloads as W
from ponyc_amd.engine import MSG_DTYPE, RING_PASS, RING_SET, GpuActorError, live_buffers

pytestmark = pytest.mark.gpu

EINVAL, ESTATE, EBUSY = -1, -6, -9


def test_no_actors(engine_factory):
    e = engine_factory()
    assert e.run() == 0
    e.run_fixed(3)
    c = e.counts()
    assert c["delivered"] == 0 and c["sent"] == 0 and c["pending"] == 0


def test_actors_without_mail_are_quiescent(engine_factory, oracle):
    """Constructors only: no step runs and the constructed state equals the
    oracle's (ring: next / id words, examples/ring/main.pony:3-24)."""
    e = engine_factory()
    e.type_register(0, 4, W.HT_RING)
    e.type_param(0, 0, 10)
    e.create(0, 30)
    assert e.run() == 0
    oracle.type_register(0, 4, W.HT_RING)
    oracle.type_param(0, 0, 10)
    oracle.create(0, 30)
    assert oracle.run() == 0
    np.testing.assert_array_equal(e.state_read(0), oracle.state_read(0))
    e.run_fixed(2)                        # empty supersteps change nothing
    np.testing.assert_array_equal(e.state_read(0), oracle.state_read(0))
    assert e.counts()["delivered"] == 0


def test_empty_sendv_is_a_noop(engine_factory, oracle):
    g = engine_factory()
    w = W.ubench(g, 256, 2, det=True, hops=5)
    g.sendv(np.zeros(0, dtype=MSG_DTYPE))
    steps = g.run()
    wo = W.ubench(oracle, 256, 2, det=True, hops=5)
    assert steps == oracle.run()
    np.testing.assert_array_equal(W.ubench_result(g, w), W.ubench_result(oracle, wo))


def test_bad_arguments_are_rejected(engine_factory):
    e = engine_factory()
    with pytest.raises(GpuActorError) as ex:
        e.type_register(16, 1, W.HT_RING)             # >= GPU_ACTOR_MAX_TYPES
    assert ex.value.code == EINVAL
    e.type_register(0, 4, W.HT_RING)
    e.type_param(0, 0, 3)
    first = e.create(0, 3)
    with pytest.raises(GpuActorError) as ex:
        e.send(first + 3, 0, 1)                       # past the last id
    assert ex.value.code == EINVAL
    with pytest.raises(GpuActorError) as ex:
        e.send(first, 16, 1)                          # behaviour outside the table
    assert ex.value.code == EINVAL
    with pytest.raises(GpuActorError):
        e.create(0, 3)                                # a type is created once
    with pytest.raises(GpuActorError) as ex:
        e.state_read(0, 0, 4)                         # past the type's actors
    assert ex.value.code == EINVAL
    # the engine is still usable after rejected calls
    e.send(first, RING_SET, first + 1)
    e.send(first, RING_PASS, 4)
    assert e.run() > 0
    assert e.counts()["dropped"] == 0


def test_reinit_after_shutdown_repeats_bit_for_bit(engine_factory):
    """The runtime is per process: shutdown + init again gives the same run."""
    out = []
    for _ in range(2):
        e = engine_factory()
        w = W.fanin(e, 300, 3, 7, 1)
        steps = e.run()
        out.append((steps, W.fanin_result(e, w).copy(), e.counts()["delivered"]))
        e.shutdown()
        assert live_buffers() == (0, 0)
    assert out[0][0] == out[1][0] and out[0][2] == out[1][2]
    np.testing.assert_array_equal(out[0][1], out[1][1])


def test_failed_init_leaves_nothing_behind(engine_factory, oracle):
    """gpu_actor_init is all or nothing: two ranks with neither a comm_id nor a
    transport fail after the stream and some thirty buffers exist; nothing of
    them stays, and the next engine runs as if the attempts had not happened."""
    for _ in range(4):
        with pytest.raises(GpuActorError) as ex:
            engine_factory(n_ranks=2, rank=0)
        assert ex.value.code == EINVAL
        assert live_buffers() == (0, 0)
    e = engine_factory()
    w = W.fanin(e, 300, 3, 7, 1)
    steps = e.run()
    wo = W.fanin(oracle, 300, 3, 7, 1)
    assert steps == oracle.run()
    np.testing.assert_array_equal(W.fanin_result(e, w), W.fanin_result(oracle, wo))
    assert e.counts()["delivered"] == oracle.counts()["delivered"]
    e.shutdown()
    assert live_buffers() == (0, 0)


# Four worlds that use disjoint parts of an engine's session: each returns what
# a run leaves behind, as bytes and numbers that compare with ==.
PORT_WORLD = dict(n=100, ports=(1,), bursts=1, m=3)   # test_gpu_host_port.py's smallest


def _counts(c):
    return tuple(c[k] for k in ("delivered", "sent", "pending", "dropped")) + \
        tuple(c["delivered_by_type"])


def _world_ports(make):
    """host ports, the host lists, the sort scratch"""
    e = make()
    w = H.world(e, PORT_WORLD)
    steps = e.run()
    msgs, counts, emit = e.recv(), e.counts(), e.state_read(w["emit_type"])
    H.check_structure(msgs, w)
    H.check_a(msgs, steps, counts, emit, PORT_WORLD)
    H.check_b(msgs, PORT_WORLD)
    return e, (steps, emit.tobytes(), _counts(counts), msgs.tobytes())


def _world_plain(setup, result, check=lambda d: None, **kw):
    def run(make):
        import pyoracle
        e = make(**kw)
        w = setup(e)
        steps = e.run()
        state, counts = result(e, w), e.counts()
        check(e.debug_info())
        if run not in _ORACLE:
            with pyoracle.Oracle() as o:
                wo = setup(o)
                _ORACLE[run] = (o.run(), result(o, wo).tobytes(), _counts(o.counts()))
        got = (steps, state.tobytes(), _counts(counts))
        assert got == _ORACLE[run]
        return e, got
    return run


def _expect(key, op):
    def check(d):
        assert op(d[key]), (key, d[key])
    return check


_ORACLE = {}
WORLDS = [
    _world_ports,
    # split launches, two zones
    _world_plain(lambda e: W.ubench(e, 4096, 4, det=True, hops=8), W.ubench_result,
                 _expect("zones", lambda v: v == 2)),
    # the small-step path
    _world_plain(lambda e: W.ring(e, 10, 3, 20), W.ring_result,
                 _expect("sparse_steps", lambda v: v > 0)),
    # spill lists, relayout_zones (test_gpu_parity.py's overflow shape: a fan-in
    # of 300 sources into 3 sinks through zones sized for one message per actor)
    _world_plain(lambda e: W.fifo(e, 300, 3, 4, 9, batch=4, mailbox_cap=1), W.fifo_result,
                 _expect("fixups", lambda v: v > 0), mailbox_cap=1),
]


def test_unlike_engines_in_one_process_do_not_see_each_other(engine_factory):
    """Four unlike worlds one after the other, then again in reverse order:
    each equals the oracle, holds nothing after its shutdown, and the second
    pass repeats the first bit for bit — nothing of an engine reaches the next."""
    passes = []
    for order in (WORLDS, WORLDS[::-1]):
        got = {}
        for world in order:
            e, got[world] = world(engine_factory)
            e.shutdown()
            assert live_buffers() == (0, 0)
        passes.append(got)
    assert passes[0] == passes[1]


def test_run_async_busy_and_serialised(engine_factory, oracle):
    """While an async run is in flight gpu_actor_run returns EBUSY; other calls
    wait behind it; wait() joins it."""
    e = engine_factory()
    w = W.ubench(e, 4096, 4, det=True, hops=64)
    e.run_async(0)
    try:
        e.run()                           # EBUSY unless the async run already ended
    except GpuActorError as ex:
        assert ex.code == EBUSY
    c = e.counts()                        # serialised behind the async run
    steps = e.wait()
    wo = W.ubench(oracle, 4096, 4, det=True, hops=64)
    assert steps == oracle.run()
    assert c["delivered"] == oracle.counts()["delivered"]
    np.testing.assert_array_equal(W.ubench_result(e, w), W.ubench_result(oracle, wo))
