"""Shared by the host-port tests (test_gpu_host_port.py, mr_hostport_worker.py,
test_host_port_abi.py): the emitter world, the oracle's two stand-ins for the
port type, and the checks of a received list against them.

The oracle is unchanged: its world registers the same types, ids and programs
with the port types under another table.
  A: HT_FANIN_ANALYZER — applied at send, delivered at once, never pending:
     steps, every count, delivered_by_type and the emitters' state are EQUAL,
     and each port's message count / XOR of arguments are its two state words.
  B: HT_FIFO_SINK with a batch above the run's messages (never overloaded,
     nothing muted): each sink folds its arrivals step by step in (sender,
     seq) order — the received list filtered by port — so folding the received
     arguments in received order from the sink's constructed h must give its
     word 0, and their number word 1.
Each stand-in runs once per world (cached) and is left unchanged."""
from __future__ import annotations

import functools

import numpy as np

from ponyc_amd import workloads as W
from ponyc_amd.engine import HT_FANIN_ANALYZER, HT_FIFO_SINK

FNV_PRIME = 0x100000001b3
FNV_BASIS = 0xcbf29ce484222325
M64 = (1 << 64) - 1

# the parity world: 3,000 emitters (two 2048-actor zones, the second partly
# filled), 3 ports of one type and 1 of a second, m = index % 4, 3 bursts
SMALL = dict(n=3000, ports=(3, 1), bursts=3)
# ... with the emitters' batch 2 and 5 BURSTs each to start with: mail is
# carried over steps and the emitters are overloaded
CARRY = dict(n=3000, ports=(3, 1), bursts=3, batch=2, initial=5)


def world(eng, kw: dict, **more):
    return W.emitter(eng, **dict(kw, **more))


@functools.lru_cache(maxsize=None)
def _stand_in(key: tuple, which: str):
    import pyoracle
    kw = dict(key)
    with pyoracle.Oracle() as o:
        if which == "A":
            w = world(o, kw, port_ht=HT_FANIN_ANALYZER)
        else:
            w = world(o, kw, port_ht=HT_FIFO_SINK, port_batch=1 << 30)
        steps = o.run()
        res = {"steps": steps, "counts": o.counts(), "emit": o.state_read(w["emit_type"]),
               "ports": [o.state_read(t) for t in w["port_types"]], "w": w}
    for v in [res["emit"], *res["ports"]]:
        v.setflags(write=False)
    return res


def stand_in(kw: dict, which: str):
    return _stand_in(tuple(sorted(kw.items())), which)


def port_ids(w: dict) -> list:
    """[(type, [ids])] of the world's ports"""
    return [(t, list(range(f, f + c))) for t, f, c in zip(w["port_types"], w["pfirst"], w["ports"])]


def check_structure(msgs: np.ndarray, w: dict) -> None:
    """keys strictly increasing in (step, from, seq); every `to` a port; for
    each (from, to) the low 32 bits of arg strictly increase"""
    key = list(zip(msgs["step"].tolist(), msgs["from"].tolist(), msgs["seq"].tolist()))
    assert all(a < b for a, b in zip(key, key[1:])), "keys not strictly increasing"
    lo, hi = w["port_first"], w["port_first"] + w["n_ports"]
    assert ((msgs["to"] >= lo) & (msgs["to"] < hi)).all()
    assert (msgs["behaviour"] == 0).all()
    assert ((msgs["from"] >= w["first"]) & (msgs["from"] < w["first"] + w["n"])).all()
    assert ((msgs["arg"] >> np.uint64(32)) == (msgs["from"] - w["first"])).all()
    last = {}
    for f, t, a in zip(msgs["from"].tolist(), msgs["to"].tolist(), msgs["arg"].tolist()):
        c = a & 0xFFFFFFFF
        assert last.get((f, t), 0) < c, (f, t, c)
        last[(f, t)] = c


def check_a(msgs: np.ndarray, steps: int, counts: dict, emit: np.ndarray, kw: dict,
            check_steps: bool = True) -> None:
    ref = stand_in(kw, "A")
    if check_steps:
        assert steps == ref["steps"], (steps, ref["steps"])
    for k in ("delivered", "sent", "pending", "dropped"):
        assert counts[k] == ref["counts"][k], (k, counts[k], ref["counts"][k])
    if check_steps:
        assert counts["steps"] == ref["counts"]["steps"]
    assert counts["delivered_by_type"] == ref["counts"]["delivered_by_type"]
    np.testing.assert_array_equal(emit, ref["emit"])
    for (t, ids), st in zip(port_ids(ref["w"]), ref["ports"]):
        for k, pid in enumerate(ids):
            mine = msgs["arg"][msgs["to"] == pid]
            assert mine.shape[0] == int(st[0, k]), (pid, mine.shape[0], int(st[0, k]))
            x = int(np.bitwise_xor.reduce(mine)) if mine.shape[0] else 0
            assert x == int(st[1, k]), (pid, x, int(st[1, k]))


def check_b(msgs: np.ndarray, kw: dict) -> None:
    ref = stand_in(kw, "B")
    assert ref["counts"]["dropped"] == 0 and ref["counts"]["pending"] == 0
    for (t, ids), st in zip(port_ids(ref["w"]), ref["ports"]):
        for k, pid in enumerate(ids):
            h = FNV_BASIS
            mine = msgs["arg"][msgs["to"] == pid].tolist()
            for a in mine:
                h = ((h ^ a) * FNV_PRIME) & M64
            assert len(mine) == int(st[1, k]), (pid, len(mine), int(st[1, k]))
            assert h == int(st[0, k]), (pid, hex(h), hex(int(st[0, k])))
