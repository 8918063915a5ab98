"""Worlds of several workloads in one engine: the setups of ponyc_amd.workloads
composed with consecutive type ids, so that the serial actors run more than
one handler table and the engine takes the any-mix step (k_step<-1>: the
compiled-in one of csrc/step_any*.hip, or the one csrc/jit_host.h compiles
for exactly that mix). Every type but the first starts at a nonzero id, most
of them off the zone grid. Shared by tests/test_mixed_worlds.py (CPU),
tests/test_gpu_mixed.py, tests/mr_mixed_worker.py and
scripts/jit_precompile.py.

A world's `setup(e)` works on an engine or the oracle and returns one
workload dict per part; `result(e, w)` is every part's result, flattened and
concatenated in part order; `part_results(e, w)` keeps them apart by name."""
from collections import namedtuple

import numpy as np

from ponyc_amd import workloads as W
from ponyc_amd.engine import (HT_RING, HT_PINGER, HT_PINGER_DET, HT_FANIN_SENDER,
                              HT_FANIN_ANALYZER, HT_GUPS_STREAMER, HT_GUPS_UPDATER, HT_STORM,
                              HT_FIFO_SRC, HT_FIFO_SINK, HT_SPREADER, HT_HOST_PORT)

# tables whose actors are no serial actors (engine.hip reducible_ht): they do
# not count towards the step kernel's choice or the mix mask
REDUCIBLE = (HT_FANIN_ANALYZER, HT_GUPS_UPDATER, HT_HOST_PORT)

# name; handler tables, one per type id the part takes, in type order;
# setup(e, t): the workload at type ids t, t + 1, ...; result(e, w)
Part = namedtuple("Part", "name tables setup result")


def _state(e, w):
    return e.state_read(w["type"])


def ring(size, count, passes, name="ring"):
    return Part(name, (HT_RING,),
                lambda e, t: W.ring(e, size, count, passes, type_id=t), W.ring_result)


def pad():
    """37 ring actors that take one SET message: whatever follows starts at
    id 37, off every zone, block and wave boundary."""
    return ring(37, 1, 0, name="pad")


def pinger(n, initial, budget):
    return Part("pinger", (HT_PINGER,),
                lambda e, t: W.ubench(e, n, initial, budget, type_id=t), W.ubench_result)


def det(n, initial, hops):
    return Part("det", (HT_PINGER_DET,),
                lambda e, t: W.ubench(e, n, initial, det=True, hops=hops, type_id=t),
                W.ubench_result)


def storm(n, r, hops):
    return Part("storm", (HT_STORM,), lambda e, t: W.storm(e, n, r, hops, type_id=t), _state)


def gups(logtable, updaters, streamers, chunk, iterate, name="gups"):
    return Part(name, (HT_GUPS_UPDATER, HT_GUPS_STREAMER),
                lambda e, t: W.gups(e, logtable, updaters, streamers, chunk, iterate,
                                    up_type=t, str_type=t + 1), W.gups_result)


def fanin(senders, analyzers, msgs, seedmode):
    return Part("fanin", (HT_FANIN_ANALYZER, HT_FANIN_SENDER),
                lambda e, t: W.fanin(e, senders, analyzers, msgs, seedmode,
                                     an_type=t, snd_type=t + 1), W.fanin_result)


def fifo(sources, sinks, bursts, m, batch, mailbox_cap):
    return Part("fifo", (HT_FIFO_SINK, HT_FIFO_SRC),
                lambda e, t: W.fifo(e, sources, sinks, bursts, m, sink_type=t, src_type=t + 1,
                                    batch=batch, mailbox_cap=mailbox_cap), W.fifo_result)


def spreader(count):
    return Part("spreader", (HT_SPREADER,),
                lambda e, t: W.spreader(e, count, type_id=t), W.spreader_result)


class World:
    def __init__(self, name, parts, **eng_kw):
        self.name, self.parts, self.eng_kw = name, list(parts), eng_kw
        assert len({p.name for p in self.parts}) == len(self.parts)

    def type0(self, part_name):
        """First type id of a part."""
        t = 0
        for p in self.parts:
            if p.name == part_name:
                return t
            t += len(p.tables)
        raise KeyError(part_name)

    def setup(self, e):
        out, t = [], 0
        for p in self.parts:
            out.append(p.setup(e, t))
            t += len(p.tables)
        return out

    def part_results(self, e, w):
        return {p.name: p.result(e, wp) for p, wp in zip(self.parts, w)}

    def result(self, e, w):
        return np.concatenate([p.result(e, wp).ravel() for p, wp in zip(self.parts, w)])

    def mask(self):
        """The mix a run-time compiled any-mix step of this world holds
        (engine.hip plan_step): a bit per table of its serial actors."""
        m = 0
        for p in self.parts:
            for ht in p.tables:
                if ht not in REDUCIBLE:
                    m |= 1 << ht
        return m


def alone(part):
    """The part by itself at type 0: what a one-table engine runs."""
    return World(part.name + "_alone", [part])


# the parts of the pairs: each runs behind the pad, at type 1 (and 2)
PAIR_PARTS = {
    "pinger": pinger(2500, 4, 12),
    "det": det(3000, 3, 9),
    "storm": storm(3000, 2, 12),
    "gups": gups(10, 4, 64, 100, 3),
    "fanin": fanin(700, 3, 6, 1),
    "fifo": fifo(300, 5, 3, 2, batch=4, mailbox_cap=16),
}
PAIRS = {name: World("pair_" + name, [pad(), part]) for name, part in PAIR_PARTS.items()}

WORLDS = {
    # 6,168 actors; det (ids 100..3099) and storm (3100..6099) each straddle
    # boundaries of 2048- and of 4096-actor zones, zone 1 holds both, the last
    # zone storm, updaters and streamers. Chunk 100: k_gups_apply's wave has
    # dead lanes (L = 16, 7 parts)
    "A": World("A", [ring(100, 1, 20), det(3000, 3, 9), storm(3000, 2, 12),
                     gups(10, 4, 64, 100, 3)]),
    # faithful pingers at first = 37; a batch-limited FIFO whose sources get
    # muted; the spreader's reserve in the middle of the id space; fan-in last
    "B": World("B", [pad(), pinger(2500, 4, 12), fifo(300, 5, 3, 2, batch=4, mailbox_cap=16),
                     spreader(8), fanin(700, 3, 6, 1)], mailbox_cap=16),
    # every step's pending records stay under k_sparse's 1024
    "THIN": World("THIN", [ring(1000, 3, 200), det(300, 1, 60), storm(200, 1, 40),
                           gups(12, 4, 2, 16, 40)]),
    # two streamer types: k_gups_apply lists the first, the second applies
    # its own chunks of 33 updates in the same steps
    "GUPS2": World("GUPS2", [pad(), gups(10, 4, 64, 100, 3),
                             gups(8, 2, 5, 33, 6, name="gups_b")]),
}
# the worlds that also run on the run-time compiled any-mix step
JIT_WORLDS = ("A", "B")


def mix_units():
    """What the JIT-on cases compile at run time, for
    scripts/jit_precompile.py: (mix mask, z12) of the JIT worlds at both zone
    geometries."""
    return [(WORLDS[name].mask(), z12) for name in JIT_WORLDS for z12 in (False, True)]
