"""Shared by test_gpu_host_order.py, test_host_order_oracle.py and
mr_worker.py: worlds in which the host is one of the senders
of an order-sensitive arrival group.

Every scenario builds a FIFO world (ponyc_amd.workloads.fifo: sinks first, so
their ids are small, then sources), runs one step so that the sources' PUSHes
are pending, puts host PUSHes into the same step's landing buffers, and
returns with the engine ready for the run to quiescence. It drives any object
with the Engine interface, so the GPU engine and the CPU oracle get the same
calls. With swap=True two messages of one sink change places (the CPU file
checks that the sinks' state then differs: the fold sees the order).

k_inject (csrc/zone_dev.h) stamps a host message with from = 0xFF000000 |
hseq >> 16 and seq = hseq & 0xFFFF, hseq counting the host's sends since the
last run; the arithmetic of each scenario's docstring is in those terms."""
from __future__ import annotations

import numpy as np

from ponyc_amd import program as P
from ponyc_amd import workloads as W
from ponyc_amd.engine import FIFO_BURST, FIFO_PUSH, HT_PROGRAM

SINKS = 8192            # four zones of 2048, two of 4096
FILLER_FIRST = 4096     # fillers go to sinks 4096..8191: never the zone of sink 0
HOST_WRAP = 1 << 16     # hseq at which seq wraps to 0 and from becomes 0xFF000001
U32 = np.uint64(32)


class Pushes:
    """The host's PUSH arguments: tag << 32 | k, k rising from 1 per sink over
    every call. tag = slot * n_sinks, so the sink files the host under
    (tag / n_sinks) % 8 == slot of its per-sender counters (oracle/bsp.c
    HT_FIFO_SINK); source i has slot (i / n_sinks) % 8."""

    def __init__(self, n_sinks: int, slot: int = 1, first: int = 0):
        self.tag = np.uint64(slot * n_sinks)
        self.first = first
        self.sent = np.zeros(n_sinks, dtype=np.uint64)

    def to(self, sinks) -> np.ndarray:
        """PUSHes to `sinks` (ids, in send order)"""
        s = np.asarray(sinks, dtype=np.int64) - self.first
        order = np.argsort(s, kind="stable")
        ss = s[order]
        start = np.flatnonzero(np.concatenate([[True], ss[1:] != ss[:-1]]))
        size = np.diff(np.concatenate([start, [ss.shape[0]]]))
        rank = np.empty(s.shape[0], dtype=np.int64)
        rank[order] = np.arange(ss.shape[0]) - np.repeat(start, size)
        k = self.sent[s] + rank.astype(np.uint64) + np.uint64(1)
        self.sent += np.bincount(s, minlength=self.sent.shape[0]).astype(np.uint64)
        return W._msgs((s + self.first).astype(np.uint64), FIFO_PUSH, (self.tag << U32) | k)


def round_robin(n: int, per: int, first: int = 0) -> np.ndarray:
    """first, first + 1, ..., first + n - 1, `per` times over"""
    return np.tile(np.arange(first, first + n, dtype=np.int64), per)


def filler(p: Pushes, n: int) -> np.ndarray:
    """n PUSHes spread over the sinks from FILLER_FIRST on"""
    span = SINKS - FILLER_FIRST
    return p.to(FILLER_FIRST + np.arange(n, dtype=np.int64) % span)


def _early(e, main: np.ndarray, swap: bool) -> np.ndarray:
    """swap: the host's first PUSH (sink 0's k = 1) is sent before the step in
    which the sources push, so sink 0 takes it ahead of its source's PUSHes
    instead of right behind them. Returns what is left to send."""
    if not swap:
        return main
    assert int(main["to"][0]) == 0
    W._sendv(e, main[:1])
    return main[1:]


def idx64(e, swap: bool = False, batch: int = 0, n_filler: int = 32768, hot: int = 8,
          per: int = 200, m: int = 4):
    """Case 1. 8 sources push m = 4 each to sinks 0..7; the host sends 32,768
    fillers (hseq 0..32,767, 8 to each of sinks 4096..8191) and then 200
    PUSHes to each of sinks 0..7, round-robin: hseq 32,768..34,367, so every
    one of them has seq >= 32,768 (sbits = 16) beside an actor sender (from
    range 32 bits): kbits = 48. The zone of sink 0 lands 8 * 204 = 1,632
    records (<= kIdxCap = 16,384: the LDS-index path, pay = 16, a 64-bit
    item), in groups of 204 > kBigGroup = 128."""
    w = W.fifo(e, hot, SINKS, 1, m, batch=batch)
    p = Pushes(SINKS)
    main = p.to(round_robin(hot, per))
    main = _early(e, main, swap)
    e.run(1)
    W._sendv(e, filler(p, n_filler))
    W._sendv(e, main)
    return w


def scratch(e, swap: bool = False, batch: int = 0, hot: int = 96, per: int = 264, m: int = 4,
            cap: int = 0):
    """Cases 2 and 3. `hot` sources push m = 4 each to sinks 0..hot-1 and the
    host sends `per` PUSHes to each of them, round-robin: hseq 0..hot*per-1,
    the group of sink s holding hseq s, s + hot, ..., s + (per - 1) * hot.
    Case 2 (96 x 264): the zone lands 96 * 268 = 25,728 records, above the
    LDS index of either geometry (16,384; 24,576 with 4096-actor zones) and
    below kHotMin = 32,768: the scratch path, pay = 20. Every group (268 >
    kBigGroup, <= 1,024) reaches hseq >= 263 * 96 = 25,248 >= 4,096, so sbits
    = 15 and kbits = 47: 67 bits, coop_sort_group refuses, and the lane orders
    it: through the key window when the batch takes the group whole, with
    acc.sort (at most 268^2 / 2 = 35,912 moves a lane) when it does not.
    Case 3 (128 x 260, cap 16): 128 * 264 = 33,792 >= kHotMin."""
    w = W.fifo(e, hot, SINKS, 1, m, batch=batch, mailbox_cap=cap)
    main = _early(e, Pushes(SINKS).to(round_robin(hot, per)), swap)
    e.run(1)
    W._sendv(e, main)
    return w


WRAP_SINKS, WRAP_PER = 256, 272          # 256 * 272 = 69,632 = 65,536 + 4,096


def wrap(e, swap: bool = False, form: str = "alone", batch: int = 0, cap: int = 0):
    """Case 4. 69,632 host PUSHes in one window, round-robin over sinks
    0..255: sink s holds hseq s, s + 256, ..., s + 271 * 256, that is 256
    records below hseq 65,536 (from 0xFF000000, seq up to 0xFF00 | s) and 16
    from it on (from 0xFF000001, seq from s): in order only if from is
    compared before seq. Groups of 272 > kBigGroup; the zone lands >= 69,632
    >= kHotMin.
    form "alone":   no actor sender (the sources burst 0): kbits = 1 + 16;
         "sources": 256 sources push 4 each in the same step: kbits = 48,
                    groups of 276 <= 1,024;
         "staged":  as "sources", the window built from sendv (hseq 0..63,999),
                    3,000 single sends (staged by the library; 64,000..66,999,
                    across the wrap) and a sendv of the rest.
    swap: the two PUSHes of sink 255 on either side of the wrap (hseq 65,535
    and 65,791) change places."""
    m = 0 if form == "alone" else 4
    w = W.fifo(e, WRAP_SINKS, SINKS, 1, m, batch=batch, mailbox_cap=cap)
    main = Pushes(SINKS).to(round_robin(WRAP_SINKS, WRAP_PER))
    if swap:
        a, b = HOST_WRAP - 1, HOST_WRAP - 1 + WRAP_SINKS
        assert main["to"][a] == main["to"][b]
        main["arg"][[a, b]] = main["arg"][[b, a]]
    e.run(1)
    if form == "staged":
        W._sendv(e, main[:64000])
        for to, beh, arg in main[64000:67000].tolist():
            W._send(e, to, beh, arg)
        W._sendv(e, main[67000:])
    else:
        W._sendv(e, main)
    return w


def small_step(e, swap: bool = False):
    """Case 5. 16 sources push 5 each to 8 sinks (10 a sink) and the host 40
    to each sink: 80 + 16 self-sent BURSTs + 320 = 416 pending records (<=
    1,024: k_sparse's step unless GPA_NO_SPARSE=1), 50 a sink (below the
    batch of 100). The sources use slots 0 and 1 of a sink's counters, the
    host slot 5."""
    w = W.fifo(e, 16, 8, 2, 5)
    main = _early(e, Pushes(8, slot=5).to(round_robin(8, 40)), swap)
    e.run(1)
    W._sendv(e, main)
    return w


def muted(e, swap: bool = False):
    """Case 6. test_gpu_backpressure.py's (64, 7, 10, 4, batch 7): the sinks
    are overloaded from step 2 on, the sources send to them in step 3 and are
    muted. Then every source gets BURST(3) and BURST(5) from the host beside
    the BURST(4) it sent itself: in step 4 it stays muted (its sink is still
    overloaded: 9 senders' pushes against a batch of 7) and its three
    arrivals are put in canonical order for the carry, without draining
    (zone_actor's `stays`). The order decides how many PUSHes each later
    burst makes. The sinks get 20 host PUSHes each as well (every slot of a
    sink is in use by sources here: the violation word means nothing)."""
    w = W.fifo(e, 64, 7, 10, 4, batch=7, mailbox_cap=16)
    e.run(3)
    src = np.arange(7, 7 + 64, dtype=np.uint64)
    W._sendv(e, W._msgs(np.repeat(src, 2), FIFO_BURST, np.tile(np.array([3, 5], np.uint64), 64)))
    W._sendv(e, Pushes(7, slot=1).to(round_robin(7, 20)))
    return w


def two_windows(e, swap: bool = False):
    """Case 7. 8 sources push 4 each to sinks 0..7; window 1 is 300 host
    PUSHes to each of them (hseq 0..2,399): groups of 304 on the LDS-index
    path, kbits = 32 + 12, 60 bits, sorted by the workgroup. One step with the
    batch of 100 leaves 204 host records carried at each sink. Window 2 (150
    to each, hseq 0..1,199 again: keys below the carried ones) must follow
    them."""
    w = W.fifo(e, 8, SINKS, 1, 4, batch=100)
    p = Pushes(SINKS)
    e.run(1)
    W._sendv(e, p.to(round_robin(8, 300)))
    e.run(1)
    W._sendv(e, p.to(round_robin(8, 150)))
    return w


# ---- the ordered receiver as a program (case 9) -----------------------------------------
def scratch_programs(e, swap: bool = False, batch: int = 100, hot: int = 96, per: int = 264,
                     m: int = 4):
    """Case 9: `scratch`'s case-2 shape with programs (ponyc_amd.program
    fold_program and burst_program; scripts/jit_precompile.py lists the set):
    96 fold sinks (ids 0..95) and 96 burst sources, all in one zone, which
    lands 96 * 268 = 25,728 records (scratch path; groups of 268 with hseq up
    to 25,343: 67 bits, refused, ordered by the lane)."""
    e.type_register(0, 8, HT_PROGRAM)
    e.type_program(0, P.fold_program())
    e.type_config(0, batch, 0)
    e.create(0, hot)
    e.type_register(1, 8, HT_PROGRAM)
    e.type_program(1, P.burst_program())
    first = e.create(1, hot)
    e.type_param(1, 0, first)
    st = np.zeros((8, hot), dtype=np.uint64)
    st[0] = np.arange(hot, dtype=np.uint64)
    e.state_write(1, st)
    W._sendv(e, W._msgs(first + np.arange(hot, dtype=np.uint64), 0, m))
    main = _early(e, Pushes(hot).to(round_robin(hot, per)), swap)
    e.run(1)
    W._sendv(e, main)
    return {"sink_type": 0, "src_type": 1}


# ---- two ranks (case 10, tests/mr_worker.py) ----------------------------------------------
def two_ranks(e, swap: bool = False):
    """62 sources push 4 each to 31 sinks, 8 a sink, twice. With ids dealt to
    two ranks by parity, source i (id 31 + i) and its sink i % 31 are on
    different ranks for i < 31 and on the same rank from there on: every sink
    has one remote and one local source. The host of each rank sends 300
    PUSHes to each sink it owns (16 sinks, 4,800 sends, on rank 0; 15 and
    4,500 on rank 1: both above 4,096; W._sendv keeps a rank's own share, in
    call order): groups of 308 > kBigGroup whose senders are a local actor, an
    actor of the other rank and the host. Sources use slots 0 and 1 of a
    sink's counters, the host slot 5."""
    w = W.fifo(e, 62, 31, 2, 4)
    main = _early(e, Pushes(31, slot=5).to(round_robin(31, 300)), swap)
    e.run(1)
    W._sendv(e, main)
    return w
