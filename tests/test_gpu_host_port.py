"""Host ports on the GPU (include/gpu_actor_host.h): programs' SENDs to port
ids, collected in canonical (step, from, seq) order. The unchanged oracle
checks them through two stand-ins for the port type (tests/host_port_checks.py):
A, fan-in Analyzers — steps, counts, delivered_by_type, emitter state and each
port's count / XOR equal; B, FIFO sinks that never overload — each port's
order-sensitive fold of the received arguments, in received order, equals the
sink's. Compiled (PONYC_AMD_JIT=1) and interpreted programs, both zone
geometries, carried mail, determinism, run_fixed, the notify callback, the
reserve's overflow contract, the rejections, and two ranks on one GPU."""
import functools
import json

import numpy as np
import pytest

import host_port_checks as H
from ponyc_amd.engine import Engine, GpuActorError, HOST_MSG_DTYPE
from test_multirank import _launch

pytestmark = pytest.mark.gpu


def _run(kw):
    """One fresh engine on the world `kw`, run to quiescence."""
    with Engine() as e:
        w = H.world(e, kw)
        steps = e.run()
        assert e.recv_pending() == e.recv_pending()
        msgs = e.recv()
        assert e.recv_pending() == 0
        return {"w": w, "steps": steps, "msgs": msgs, "counts": e.counts(),
                "emit": e.state_read(w["emit_type"]), "dbg": e.debug_info()}


@functools.lru_cache(maxsize=None)
def _reference():
    """The parity world's received list from an engine with the defaults
    (what tests 3-5 compare against), made once."""
    r = _run(H.SMALL)
    r["msgs"].setflags(write=False)
    return r


def _check(r, kw):
    assert r["msgs"].dtype == HOST_MSG_DTYPE and r["msgs"].shape[0] > 0
    H.check_structure(r["msgs"], r["w"])
    H.check_a(r["msgs"], r["steps"], r["counts"], r["emit"], kw)
    H.check_b(r["msgs"], kw)


@pytest.mark.parametrize("bits", ["11", "12"])
@pytest.mark.parametrize("jit", ["1", "0"])
def test_parity_small(monkeypatch, jit, bits):
    monkeypatch.setenv("PONYC_AMD_JIT", jit)
    monkeypatch.setenv("PONYC_AMD_ZONE_BITS", bits)
    r = _run(H.SMALL)
    _check(r, H.SMALL)
    assert r["msgs"]["seq"].max() > 0                   # several sends in one behaviour
    assert r["dbg"]["sparse_steps"] == 0                # engines with ports stay on the zone path
    assert (r["dbg"]["jit"] == 1) == (jit == "1"), r["dbg"]
    assert r["dbg"]["zone_bits"] == int(bits)


@pytest.mark.parametrize("jit", ["1", "0"])
def test_carried_mail(monkeypatch, jit):
    monkeypatch.setenv("PONYC_AMD_JIT", jit)
    r = _run(H.CARRY)
    _check(r, H.CARRY)
    # mail was carried: more steps than the same world draining whole
    assert r["steps"] > H.stand_in(H.SMALL, "A")["steps"]


def test_determinism():
    a, b = _reference()["msgs"], _run(H.SMALL)["msgs"]
    assert a.tobytes() == b.tobytes()


def test_run_fixed_and_recv_cap():
    ref = _reference()
    with Engine() as e:
        H.world(e, H.SMALL)
        e.run_fixed(ref["steps"])
        n = e.recv_pending()
        assert n == ref["msgs"].shape[0]
        head = e.recv(1000)
        assert head.shape[0] == 1000 and e.recv_pending() == n - 1000
        mid = e.recv(7)
        rest = e.recv()
        assert e.recv_pending() == 0 and e.recv().shape[0] == 0
    got = np.concatenate([head, mid, rest])
    assert got.tobytes() == ref["msgs"].tobytes()


def test_host_notify():
    ref = _reference()
    batches = []
    with Engine() as e:
        H.world(e, H.SMALL)
        e.host_notify(batches.append)
        e.run()
        assert e.recv_pending() == 0 and e.recv().shape[0] == 0
        e.host_notify(None)
    assert len(batches) > 1 and all(b.shape[0] > 0 for b in batches)
    assert np.concatenate(batches).tobytes() == ref["msgs"].tobytes()


def test_reserve_exceeded():
    kw = dict(n=100, ports=(1,), bursts=1, m=3)       # one step sends 300
    with Engine() as e:
        e.host_reserve(100)
        w = H.world(e, kw)
        with pytest.raises(GpuActorError) as ei:
            e.run()
        assert ei.value.code == -4                      # GPU_ACTOR_EMAILBOX
        assert e.counts()["dropped"] == 200
        msgs = e.recv()
    assert msgs.shape[0] == 100
    H.check_structure(msgs, w)
    assert len(set(msgs["step"].tolist())) == 1
    want = {(w["first"] + i, k, w["port_first"], 0, (i << 32) | (k + 1))
            for i in range(100) for k in range(3)}
    got = list(zip(msgs["from"].tolist(), msgs["seq"].tolist(), msgs["to"].tolist(),
                   msgs["behaviour"].tolist(), msgs["arg"].tolist()))
    assert len(set(got)) == 100 and set(got) <= want


def test_rejections():
    with Engine() as e:
        w = H.world(e, H.SMALL)
        for port in (w["port_first"], w["port_first"] + w["n_ports"] - 1):
            with pytest.raises(GpuActorError) as ei:
                e.send(port, 0, 1)
            assert ei.value.code == -1                  # GPU_ACTOR_EINVAL
            with pytest.raises(GpuActorError) as ei:
                e.sendv([(w["first"], 0, 0), (port, 0, 1)])
            assert ei.value.code == -1
    from ponyc_amd import workloads as W
    with Engine() as e:                                 # no ports
        W.ring(e, 8, 1, 20)
        e.run()
        assert e.recv_pending() == 0 and e.recv(16).shape[0] == 0


def _mixed(eng, port_ht=None):
    """8 analyzers, 1,000 fan-in senders and 1,000 emitters in ONE 2048-actor
    zone (slots 8-1007 and 1008-2007; a thread drains slots t, t + 512,
    t + 1024, t + 1536: senders and emitters both), then the ports: the
    any-mix kernel, and threads whose one drain context makes Analyzer
    applies and host-bound sends."""
    from ponyc_amd import workloads as W
    wf = W.fanin(eng, 1000, 8, 5, 1, an_type=0, snd_type=1)
    we = W.emitter(eng, n=1000, ports=(3, 1), bursts=3, emit_type=2, port_type0=3, port_ht=port_ht)
    return wf, we


def test_mixed_zone_by_type(monkeypatch, oracle):
    # (the precompiled any-mix kernel: no run-time build of this one mix)
    monkeypatch.setenv("PONYC_AMD_JIT", "0")
    from ponyc_amd.engine import HT_FANIN_ANALYZER
    with Engine() as e:
        wf, we = _mixed(e)
        steps = e.run()
        msgs, c = e.recv(), e.counts()
        an, emit = e.state_read(wf["an_type"]), e.state_read(we["emit_type"])
        assert e.debug_info()["zones"] == 1
    wfo, weo = _mixed(oracle, port_ht=HT_FANIN_ANALYZER)
    so, co = oracle.run(), oracle.counts()
    assert steps == so
    for k in ("delivered", "sent", "pending", "dropped"):
        assert c[k] == co[k], (k, c[k], co[k])
    assert c["delivered_by_type"] == co["delivered_by_type"]
    assert sum(c["delivered_by_type"]) == c["delivered"]
    np.testing.assert_array_equal(an, oracle.state_read(wfo["an_type"]))
    np.testing.assert_array_equal(emit, oracle.state_read(weo["emit_type"]))
    H.check_structure(msgs, we)
    for t, f, n in zip(we["port_types"], we["pfirst"], we["ports"]):
        st = oracle.state_read(t)
        for k in range(n):
            mine = msgs["arg"][msgs["to"] == f + k]
            assert mine.shape[0] == int(st[0, k])
            assert int(np.bitwise_xor.reduce(mine)) == int(st[1, k])


def test_two_ranks_one_gpu():
    out = _launch("mr_hostport_worker.py", 2)
    line = [l for l in out.splitlines() if l.startswith("MR_RESULT ")]
    assert line, out[-2000:]
    r = json.loads(line[-1][len("MR_RESULT "):])
    assert r["own_senders_only"] == [True, True]
    assert all(n > 0 for n in r["received"])
    assert r["checks"] == "ok", r["checks"]
    assert r["remote"] == 0
