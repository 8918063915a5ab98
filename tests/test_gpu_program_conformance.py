"""Per-op conformance of GPU_ACTOR_HT_PROGRAM on the GPU: the engine against
the oracle and the reference model (tests/prog_model.py) on every conformance
set (tests/prog_conformance.py) — state words, delivered / sent / dropped /
pending and the step count after every run, bit for bit.

4,200 actors per type: three zones at PONYC_AMD_ZONE_BITS=11, two at 12; the
edge cross product sits in the first zone, random operands cross the zone
boundaries. With GPA_NO_SPARSE=1 every step is a zone step: the run-time
compiled step (PONYC_AMD_JIT=1, the default users get) or the device
interpreter (PONYC_AMD_JIT=0) — asserted from debug_info(), so a compile that
is rejected or fails and falls back to the interpreter fails the test. One
more case per set, small enough that every step takes the small-step path,
compares k_sparse's interpreter."""
import pytest

import prog_conformance as C
from test_program_conformance import model_of

pytestmark = pytest.mark.gpu

_oracle_cache: dict = {}


def oracle_of(oracle, name, n):
    """The oracle's snapshots of a set, computed once and left unchanged."""
    if (name, n) not in _oracle_cache:
        _oracle_cache[name, n] = C.play(oracle, C.SETS[name](n))
    return _oracle_cache[name, n]


@pytest.mark.parametrize("jit", ["1", "0"])
@pytest.mark.parametrize("bits", ["11", "12"])
@pytest.mark.parametrize("name", list(C.SETS))
def test_zone_steps(engine_factory, oracle, monkeypatch, name, bits, jit):
    monkeypatch.setenv("PONYC_AMD_ZONE_BITS", bits)
    monkeypatch.setenv("PONYC_AMD_JIT", jit)
    monkeypatch.setenv("GPA_NO_SPARSE", "1")
    s, want, _ = model_of(name, C.GPU_N)
    C.assert_same(oracle_of(oracle, name, C.GPU_N), want, f"oracle, {name}")
    e = engine_factory()
    got = C.play(e, s)
    d = e.debug_info()
    C.assert_same(got, want, f"engine, {name}, zone bits {bits}, jit {jit}")
    assert d["zone_bits"] == int(bits) and d["sparse_steps"] == 0, d
    if jit == "1":
        assert d["jit_builds"] >= 1 and d["jit"] == 1, d    # built, and the last step ran it
    else:
        assert d["jit_builds"] == 0 and d["jit"] == 0, d


@pytest.mark.parametrize("name", list(C.SETS))
def test_small_steps(engine_factory, oracle, monkeypatch, name):
    """Every step on the small-step path (k_sparse's interpreter)."""
    monkeypatch.delenv("GPA_NO_SPARSE", raising=False)
    n = C.SPARSE_N[name]
    s, want, _ = model_of(name, n)
    C.assert_same(oracle_of(oracle, name, n), want, f"oracle, {name}")
    e = engine_factory()
    got = C.play(e, s)
    d = e.debug_info()
    C.assert_same(got, want, f"engine, {name}, small steps")
    assert d["sparse_steps"] == want[-1][3]["steps"] > 0, (d, want[-1][3])
