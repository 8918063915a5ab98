"""The mixed worlds of tests/mixed_worlds.py on the CPU oracle: a workload
that runs behind other types, at a nonzero first id, must compute what it
computes alone at type 0. This is a second reference for the offset
arithmetic of the handlers (`params[1] + k`, `a.self - T.first`,
`ubase + ...`): the GPU parity tests compare engine and oracle, and would
pass if both were wrong in the same way.

Which parts are compared: every part whose result holds no actor ids —
pingers, det pingers, storm, the GUPS table, the fan-in analyzers, the FIFO
sinks, and the rings ([recv, done] only: ring_result leaves the successor id
out). The spreader's state holds its parent's id; world B, the only one with
a spreader, is not compared part by part here."""
import numpy as np
import pytest

import mixed_worlds as MW
import pyoracle


def _run(world):
    with pyoracle.Oracle() as o:
        w = world.setup(o)
        steps = o.run()
        c = o.counts()
        parts = {k: v.copy() for k, v in world.part_results(o, w).items()}
    assert c["dropped"] == 0 and c["pending"] == 0
    return steps, c, parts


@pytest.fixture(scope="module")
def alone():
    """Every pair part by itself at type 0, run once."""
    return {name: _run(MW.alone(part)) for name, part in MW.PAIR_PARTS.items()}


@pytest.mark.parametrize("name", sorted(MW.PAIRS))
def test_pair_equals_alone(alone, name):
    """Behind the 37-actor pad: the same result bit for bit, the same step
    count, and exactly one message more delivered (the pad's SET)."""
    world = MW.PAIRS[name]
    steps, c, parts = _run(world)
    a_steps, a_c, a_parts = alone[name]
    np.testing.assert_array_equal(parts[name], a_parts[name])
    assert steps == a_steps
    assert c["delivered"] == a_c["delivered"] + 1
    assert c["sent"] == a_c["sent"]
    assert c["delivered_by_type"][0] == 1
    n = len(MW.PAIR_PARTS[name].tables)
    assert c["delivered_by_type"][1:1 + n] == a_c["delivered_by_type"][:n]


@pytest.mark.parametrize("part", ["det", "storm", "gups"])
def test_world_a_parts_equal_alone(alone, part):
    """World A's det pingers (first 100), storm (first 3100) and GUPS types
    (first 6100) are the pairs' shapes: each computes what it computes alone,
    and its types take the same number of messages."""
    world = MW.WORLDS["A"]
    _steps, c, parts = _run(world)
    _a_steps, a_c, a_parts = alone[part]
    np.testing.assert_array_equal(parts[part], a_parts[part])
    t, n = world.type0(part), len(MW.PAIR_PARTS[part].tables)
    assert t > 0
    assert c["delivered_by_type"][t:t + n] == a_c["delivered_by_type"][:n]


def test_world_a_ring_and_totals():
    steps, c, parts = _run(MW.WORLDS["A"])
    assert (steps, c["delivered"]) == (21, 232878)
    assert parts["ring"][0].sum() == 21          # pass(20) visits 21 actors


@pytest.mark.parametrize("name,steps,delivered", [("B", 91, 51090), ("THIN", 201, 36700),
                                                  ("GUPS2", 7, None)])
def test_world_shapes(name, steps, delivered):
    """The worlds quiesce without drops in the step counts the GPU tests
    rely on (THIN's steps stay sparse, B's runs cross call boundaries)."""
    s, c, _parts = _run(MW.WORLDS[name])
    assert s == steps
    if delivered is not None:
        assert c["delivered"] == delivered


def test_gups2_tables_equal_alone():
    """Both GUPS worlds of GUPS2 against their stand-alone runs."""
    _s, _c, parts = _run(MW.WORLDS["GUPS2"])
    for p in MW.WORLDS["GUPS2"].parts[1:]:
        np.testing.assert_array_equal(parts[p.name], _run(MW.alone(p))[2][p.name])


def test_mix_units():
    from ponyc_amd import engine as E
    units = MW.mix_units()
    assert len(units) == 4 and len(set(units)) == 4
    assert {z for _m, z in units} == {False, True}
    for mask, _z12 in units:
        for ht in MW.REDUCIBLE:
            assert not (mask >> ht) & 1
    a, b = MW.WORLDS["A"].mask(), MW.WORLDS["B"].mask()
    assert a == sum(1 << h for h in (E.HT_RING, E.HT_PINGER_DET, E.HT_STORM, E.HT_GUPS_STREAMER))
    assert b == sum(1 << h for h in (E.HT_RING, E.HT_PINGER, E.HT_FIFO_SINK, E.HT_FIFO_SRC,
                                     E.HT_SPREADER, E.HT_FANIN_SENDER))
    # the tables this suite never ran through the any-mix switch before
    for ht in (E.HT_PINGER_DET, E.HT_STORM, E.HT_GUPS_STREAMER):
        assert (a >> ht) & 1
    assert (b >> E.HT_PINGER) & 1


def test_precompile_lists_the_mix_units():
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                    "scripts"))
    try:
        import jit_precompile
    finally:
        sys.path.pop(0)
    listed = [(p, z) for p, z in jit_precompile.sets() if isinstance(p, int)]
    for unit in MW.mix_units():
        assert unit in listed
