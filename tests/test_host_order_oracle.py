"""The host-order scenarios (tests/host_order.py) on the CPU oracle alone: each
is run as test_gpu_host_order.py runs it and once more with two messages of
one sink in swapped places, and the sinks' state must differ. This pins that
the order-sensitive fold sees the order the GPU tests rely on: a GPU engine
that delivered the pair the other way round could not equal the oracle.

The swapped pair: for the shapes with an actor sender, the host's first PUSH
to sink 0 and that sink's source PUSHes (neighbours in canonical order: every
actor ranks below the host), by sending the host PUSH before the step in
which the sources push; for the wrap, the two PUSHes of one sink on either
side of hseq 65,535 / 65,536. Nothing is scaled down: the oracle takes the
GPU cases' full shapes, fillers included, in well under a second each."""
import numpy as np
import pytest

import host_order as HO
from ponyc_amd import workloads as W

CASES = {
    "idx64": lambda e, swap: HO.idx64(e, swap),
    "idx64_whole": lambda e, swap: HO.idx64(e, swap, batch=1 << 20),
    "scratch_window": lambda e, swap: HO.scratch(e, swap, batch=512),
    "scratch_carry": lambda e, swap: HO.scratch(e, swap, batch=100),
    "hot": lambda e, swap: HO.scratch(e, swap, batch=100, hot=128, per=260, cap=16),
    "wrap_alone": lambda e, swap: HO.wrap(e, swap, "alone", batch=512),
    "wrap_sources": lambda e, swap: HO.wrap(e, swap, "sources", batch=100),
    "wrap_staged": lambda e, swap: HO.wrap(e, swap, "staged", batch=512),
    "small_step": lambda e, swap: HO.small_step(e, swap),
    "programs": lambda e, swap: HO.scratch_programs(e, swap),
    "two_ranks": lambda e, swap: HO.two_ranks(e, swap),
}


def _run(case, swap):
    import pyoracle
    with pyoracle.Oracle() as o:
        w = CASES[case](o, swap)
        steps = o.run()
        return steps, o.counts(), W.fifo_result(o, w)


@pytest.mark.parametrize("case", list(CASES))
def test_swapped_pair_changes_the_fold(case):
    steps, c, st = _run(case, False)
    steps_s, c_s, st_s = _run(case, True)
    assert c["dropped"] == 0 and c["pending"] == 0
    # the same messages either way: only their order at one sink differs
    assert c["delivered"] == c_s["delivered"] and c["sent"] == c_s["sent"]
    np.testing.assert_array_equal(st[1], st_s[1])           # messages per sink
    sink = 255 if case.startswith("wrap") else 0
    assert st[0][sink] != st_s[0][sink]                      # its fold
    others = np.arange(st.shape[1]) != sink
    np.testing.assert_array_equal(st[0][others], st_s[0][others])
    if case.startswith("wrap"):
        # the swapped pair is the host's own: the sink counts it as a violation
        assert int(st[2].sum()) == 0 and int(st_s[2][sink]) > 0


def test_violation_word_is_zero_as_specified():
    """Where no two senders share a slot of the sink's counters (every
    scenario here but `muted`), in-order delivery leaves the violation word 0:
    the tags keep the host clear of the sources' slots."""
    for case in CASES:
        if case == "programs":
            continue                                        # the fold program has no such word
        _, _, st = _run(case, False)
        assert int(st[2].sum()) == 0, case


def test_pushes_count_per_sink():
    p = HO.Pushes(4, slot=3)
    a = p.to([2, 0, 2, 2, 1])
    b = p.to([2, 3])
    assert (a["arg"] >> np.uint64(32)).tolist() == [12] * 5
    assert (a["arg"] & np.uint64(0xFFFFFFFF)).tolist() == [1, 1, 2, 3, 1]
    assert (b["arg"] & np.uint64(0xFFFFFFFF)).tolist() == [4, 1]
    assert a["to"].tolist() == [2, 0, 2, 2, 1] and (a["behaviour"] == 0).all()
