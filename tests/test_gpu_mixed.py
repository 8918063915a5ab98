"""Every handler table through the any-mix step: the worlds of
tests/mixed_worlds.py on the engine, bit-exact against the CPU oracle (state,
delivered, sent, pending, delivered_by_type, steps, nothing dropped).

An engine whose serial actors run more than one table takes k_step<-1> — the
compiled-in kernel of csrc/step_any*.hip (PONYC_AMD_JIT=0) or the one compiled
at run time for the world's mix (csrc/jit_host.h; precompiled by build()
through mixed_worlds.mix_units) — whose drains are chosen by zone_dev.h's
ZCASE switch; k_sparse has a switch of its own (sparse_dev.h) and
k_gups_apply runs behind either. In these worlds every type but the first
starts at a nonzero id, off the zone grid, and zones hold two serial types."""
import json
import os

import numpy as np
import pytest

import mixed_worlds as MW
from test_gpu_parity import _both, _assert_same
from test_multirank import _launch

pytestmark = pytest.mark.gpu

GUPS_A = 64 * 100 * 4           # gups(10, 4, 64, 100, 3): streamers * chunk * (iterate + 1)


def _run_world(engine_factory, oracle, monkeypatch, world, zbits, jit):
    monkeypatch.setenv("PONYC_AMD_ZONE_BITS", zbits)
    monkeypatch.setenv("PONYC_AMD_JIT", jit)
    g, o = _both(engine_factory, oracle, world.setup, world.result, **world.eng_kw)
    _assert_same(g, o)
    d = g[1]["debug"]
    print(world.name, zbits, jit, {k: d[k] for k in ("jit_builds", "plan_zones", "zone_bits",
                                                     "sparse_steps", "gups_updates",
                                                     "gups_atomics", "fixups")})
    assert d["zone_bits"] == int(zbits)
    assert d["plan_zones"] == 0             # the two-pass pinger kernel did not run
    assert (d["jit_builds"] >= 1) == (jit == "1")
    return g, d


@pytest.mark.parametrize("jit", ["1", "0"])
@pytest.mark.parametrize("zbits", ["11", "12"])
@pytest.mark.parametrize("name", MW.JIT_WORLDS)
def test_world(engine_factory, oracle, monkeypatch, name, zbits, jit):
    """A: ring + det pingers + storm + GUPS; B: pad + faithful pingers + FIFO
    + spreader + fan-in. Both any-mix kernels, both zone geometries."""
    _g, d = _run_world(engine_factory, oracle, monkeypatch, MW.WORLDS[name], zbits, jit)
    if name == "A":
        assert d["gups_updates"] == GUPS_A
        assert 0 < d["gups_atomics"] <= d["gups_updates"]


@pytest.mark.parametrize("zbits", ["11", "12"])
@pytest.mark.parametrize("name", sorted(MW.PAIRS))
def test_pair(engine_factory, oracle, monkeypatch, name, zbits):
    """One workload behind the 37-actor pad: its first id is 37."""
    _g, d = _run_world(engine_factory, oracle, monkeypatch, MW.PAIRS[name], zbits, "0")
    if name == "gups":
        assert d["gups_updates"] == GUPS_A


def test_world_a_gups_not_deferred(engine_factory, oracle, monkeypatch):
    """PONYC_AMD_GUPS_DEFER=0: the streamers send one record per update
    through the any-mix step; k_gups_apply takes none."""
    monkeypatch.setenv("PONYC_AMD_GUPS_DEFER", "0")
    _g, d = _run_world(engine_factory, oracle, monkeypatch, MW.WORLDS["A"], "11", "0")
    assert d["gups_updates"] == 0


@pytest.mark.parametrize("no_sparse", ["0", "1"])
def test_two_streamer_types(engine_factory, oracle, monkeypatch, no_sparse):
    """k_gups_apply lists the first streamer type's chunks and no others: the
    second type's 5 * 33 * 7 updates are applied by its streamers in the same
    steps and are not in gups_updates. `result` holds both tables. The world
    is small enough for every step to take k_sparse; GPA_NO_SPARSE=1 sends
    the same steps through the any-mix k_step."""
    monkeypatch.setenv("GPA_NO_SPARSE", no_sparse)
    _g, d = _run_world(engine_factory, oracle, monkeypatch, MW.WORLDS["GUPS2"], "11", "0")
    assert d["gups_updates"] == GUPS_A
    assert (d["sparse_steps"] > 0) == (no_sparse == "0")


def _run_sparse(engine_factory, world, sparse):
    """tests/test_gpu_sparse.py _run, with the engine's debug counters."""
    old = os.environ.get("GPA_NO_SPARSE")
    os.environ["GPA_NO_SPARSE"] = "0" if sparse else "1"
    try:
        e = engine_factory(**world.eng_kw)
        w = world.setup(e)
        s = e.run()
        c = e.counts()
        d = e.debug_info()
        r = world.result(e, w).copy()
        e.shutdown()
    finally:
        if old is None:
            os.environ.pop("GPA_NO_SPARSE", None)
        else:
            os.environ["GPA_NO_SPARSE"] = old
    return s, c, r, d


def test_thin_sparse_and_zone_path(engine_factory, oracle, monkeypatch):
    """THIN stays under k_sparse's 1024 pending records: its steps go through
    sparse_dev.h's own switch over the tables (GPA_NO_SPARSE=0) or through the
    any-mix k_step (1). Both equal each other and the oracle."""
    monkeypatch.setenv("PONYC_AMD_JIT", "0")
    world = MW.WORLDS["THIN"]
    sp = _run_sparse(engine_factory, world, True)
    dn = _run_sparse(engine_factory, world, False)
    wo = world.setup(oracle)
    so = oracle.run()
    co = oracle.counts()
    ro = world.result(oracle, wo)
    for s, c, r, _d in (sp, dn):
        np.testing.assert_array_equal(r, ro)
        assert s == so
        assert c["delivered"] == co["delivered"] and c["sent"] == co["sent"]
        assert c["pending"] == co["pending"] == 0
        assert c["delivered_by_type"] == co["delivered_by_type"]
        assert c["dropped"] == 0
    np.testing.assert_array_equal(sp[2], dn[2])
    assert sp[1]["active"] == dn[1]["active"]
    print("THIN sparse_steps", sp[3]["sparse_steps"], dn[3]["sparse_steps"])
    assert sp[3]["sparse_steps"] > 0
    assert dn[3]["sparse_steps"] == 0


def test_world_b_across_calls(engine_factory, oracle, monkeypatch):
    """run(5), run_fixed(4), run(): spawned actors, carried FIFO mail and
    muted sources cross the call boundaries; the oracle is stepped the same
    way and every intermediate state compared."""
    monkeypatch.setenv("PONYC_AMD_JIT", "0")
    world = MW.WORLDS["B"]
    e = engine_factory(**world.eng_kw)
    we, wo = world.setup(e), world.setup(oracle)

    def same():
        ce, co = e.counts(), oracle.counts()
        np.testing.assert_array_equal(world.result(e, we), world.result(oracle, wo))
        for k in ("delivered", "sent", "pending", "delivered_by_type"):
            assert ce[k] == co[k], k
        assert ce["dropped"] == 0
        return co["pending"]

    assert e.run(5) == oracle.run(5) == 5
    assert same() > 0
    e.run_fixed(4)
    oracle.run_fixed(4)
    assert same() > 0
    se, so = e.run(), oracle.run()
    assert se == so and 9 + so == 91
    assert same() == 0
    assert e.debug_info()["plan_zones"] == 0


@pytest.mark.parametrize("bits", [None, 4])
@pytest.mark.parametrize("name", MW.JIT_WORLDS)
def test_two_ranks(monkeypatch, name, bits):
    """Two ranks on one GPU through the host transport
    (tests/mr_mixed_worker.py), at the default placement and in blocks of 16
    ids: more than one workload in a multi-rank engine."""
    monkeypatch.setenv("PONYC_AMD_JIT", "0")
    args = [name] + ([] if bits is None else ["--bits", str(bits)])
    out = _launch("mr_mixed_worker.py", 2, *args)
    line = [l for l in out.splitlines() if l.startswith("MR_RESULT ")]
    assert line, out[-2000:]
    r = json.loads(line[-1][len("MR_RESULT "):])
    print(r)
    assert r["block_bits"] == (bits or int(os.environ.get("PONYC_AMD_BLOCK_BITS") or 0))
    assert r["dropped"] == 0
    assert r["state_equal"]
    assert r["steps"][0] == r["steps"][1]
    assert r["delivered"][0] == r["delivered"][1]
    assert r["sent"][0] == r["sent"][1]
    assert r["pending"][0] == r["pending"][1]
    assert r["by_type"]
    assert r["remote"] > 0
    assert r["plan_zones"] == 0
