"""The step plan (csrc/engine.hip StepPlan: entry, launch form, run-time
compiled module) is decided once per configuration and must be decided again
when the configuration changes under a live engine: a second handler table
created after steps ran moves the choice from the pinger's own step to the
any-mix step, a batch change keeps it there, and a replaced program takes
another module. Every stage is compared with the CPU oracle bit for bit, and
debug_info()'s `jit` / `jit_builds` show that a module is built when the mix
changes and not per step.

The smallest worlds that cross a zone boundary: a zone and one actor
(2,049 pingers at 2048-actor zones, 4,097 at 4096-actor zones; two zones).
build() compiles the any-mix modules of pingers + a ring
(scripts/jit_precompile.py).

Pinned elsewhere, not repeated here: a second table created after plan steps
with the compact landing lane in use, on the compiled-in any-mix kernel
(test_gpu_land8.py test_second_table_after_plan_steps)."""
import numpy as np
import pytest

from ponyc_amd import program as P
from ponyc_amd import workloads as W
from ponyc_amd.engine import MSG_DTYPE, PINGER_PING

pytestmark = pytest.mark.gpu



def _same(e, oracle, parts):
    """parts: (result function, engine's workload, oracle's workload)"""
    for result, we, wo in parts:
        np.testing.assert_array_equal(result(e, we), result(oracle, wo))
    ce, co = e.counts(), oracle.counts()
    for k in ("delivered", "sent", "pending", "delivered_by_type"):
        assert ce[k] == co[k], (k, ce[k], co[k])
    assert ce["dropped"] == 0
    return ce


@pytest.mark.parametrize("jit", ["1", "0"])
@pytest.mark.parametrize("bits,n", [("11", 2049), ("12", 4097)])
def test_second_table_then_batch(engine_factory, oracle, monkeypatch, bits, n, jit):
    monkeypatch.setenv("PONYC_AMD_ZONE_BITS", bits)
    monkeypatch.setenv("PONYC_AMD_JIT", jit)
    e = engine_factory()
    on = 1 if jit == "1" else 0
    # 1. pingers alone: their own step, nothing compiled at run time
    parts = [(W.ubench_result, W.ubench(e, n, 3, 100), W.ubench(oracle, n, 3, 100))]
    assert e.run(3) == oracle.run(3) == 3
    assert _same(e, oracle, parts)["pending"] > 0
    d = e.debug_info()
    assert (d["zone_bits"], d["zones"]) == (int(bits), 2)
    assert d["plan_zones"] > 0 and (d["jit"], d["jit_builds"]) == (0, 0), d
    # 2. a ring of 8 behind them: the any-mix step, compiled for this mix once
    parts.append((W.ring_result, W.ring(e, 8, 1, 100, type_id=1), W.ring(oracle, 8, 1, 100, type_id=1)))
    plan_zones = d["plan_zones"]
    assert e.run(3) == oracle.run(3) == 3
    _same(e, oracle, parts)
    d = e.debug_info()
    assert d["plan_zones"] == plan_zones          # the pinger's two-pass step ran no more
    assert (d["jit"], d["jit_builds"]) == (on, on), d
    # 3. another batch for the pingers: a new plan, the same module
    e.type_config(0, batch=2)
    oracle.type_config(0, batch=2)
    assert e.run(3) == oracle.run(3) == 3
    assert _same(e, oracle, parts)["pending"] > 0
    d = e.debug_info()
    assert d["plan_zones"] == plan_zones and d["zones"] == 2
    assert (d["jit"], d["jit_builds"]) == (on, on), d


def test_program_replaced(engine_factory, oracle, monkeypatch):
    """256 actors run the ring's program, then the deterministic ping's in its
    place (gpu_actor_type_program on the created type): the steps after it run
    the second program's module."""
    monkeypatch.setenv("PONYC_AMD_JIT", "1")
    e = engine_factory()
    we, wo = W.ring_prog(e, 64, 4, 100), W.ring_prog(oracle, 64, 4, 100)
    state = [(lambda x, w: x.state_read(w["type"]), we, wo)]
    e.run_fixed(3)
    oracle.run_fixed(3)
    _same(e, oracle, state)
    d = e.debug_info()
    assert (d["jit"], d["jit_builds"]) == (1, 1), d
    assert e.run() == oracle.run()
    _same(e, oracle, state)
    assert e.debug_info()["jit_builds"] == 1
    n = we["n"]
    i = np.arange(n, dtype=np.uint64)
    m = np.empty(n, dtype=MSG_DTYPE)
    m["to"], m["behaviour"], m["arg"] = we["first"] + i, PINGER_PING, i << np.uint64(32)
    for x, w in ((e, we), (oracle, wo)):
        x.type_program(0, P.det_program(PINGER_PING))
        for idx, v in enumerate((n, w["first"], 9, 5489)):
            x.type_param(0, idx, v)
        x.sendv(m)
    e.run_fixed(3)
    oracle.run_fixed(3)
    assert _same(e, oracle, state)["pending"] > 0
    d = e.debug_info()
    assert (d["jit"], d["jit_builds"]) == (1, 2), d
    assert e.run() == oracle.run()
    assert _same(e, oracle, state)["pending"] == 0
    assert e.debug_info()["jit_builds"] == 2
