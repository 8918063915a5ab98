"""Per-op conformance of GPU_ACTOR_HT_PROGRAM on the CPU. The reference model
(tests/prog_model.py, written from the instruction set's statement in
include/gpu_actor.h) against

- the oracle's interpreter (oracle/bsp.c run_program), which until now only
  its own compiled tables pinned: state words, delivered / sent / dropped /
  pending and the step count, bit for bit, on every conformance set
  (tests/prog_conformance.py);
- the C++ that csrc/jit_host.h generates for the run-time compiled step,
  compiled for the host against a shim (tests/prog_jit_host.py): state, the
  sends in order and the drops of every actor and message of every set.

The device interpreters and the compiled step itself are compared with the
same model in tests/test_gpu_program_conformance.py."""
import os

import numpy as np
import pytest

import prog_conformance as C
import prog_jit_host as H
import prog_model as M
import pyoracle
from ponyc_amd import program as P
from ponyc_amd.engine import LIB_PATH

_model_cache: dict = {}


def model_of(name, n=C.CPU_N):
    """The model's snapshots and world of a set, computed once."""
    if (name, n) not in _model_cache:
        s = C.SETS[name](n)
        w = C.model_world(s)
        _model_cache[name, n] = (s, C.model_play(s, world=w), w)
    return _model_cache[name, n]


def test_model_unit():
    """The model on hand-computed cases (it is the reference: a slip in it
    must not pass as everyone else's bug)."""
    p = P.Program()
    p.behaviour(3)
    p.ldi(11, -1)                       # 2^64 - 1
    p.addi(0, 11, 2)                    # wraps to 1
    p.mulhi(1, 11, 11)                  # 2^64 - 2
    p.ldi(12, 65)
    p.shl(2, 0, 12)                     # 1 << (65 & 63) = 2
    p.sub(3, 0, 2)                      # 1 - 2 = 2^64 - 1
    p.ltu(4, 0, 3)
    p.ldp(5, -1)                        # param 7
    p.send(11, 0x1F, 9)                 # past the ids: dropped
    p.send(0, -1, 10)                   # to id 1, behaviour 15, arg the behaviour
    p.yield_()
    p.spawn(2, 5, 0)
    p.mix(6, 13)                        # mix(0)
    p.halt()
    r = M.run(p.assemble(), [10, 11, 12, 13, 14, 15, 16, 17], [7] * 8, 42, 3, 99, 50)
    assert r.state == [1, C.M64 - 1, 2, C.M64, 1, 17, 0xE220A8397B1DCDAF, 7]
    assert r.sends == [(1, 15, 3)] and r.dropped == 1 and r.yields == 1
    assert r.spawns == [(2, 5, 1)] and r.executed == 14
    # an entry of 0, an entry past the program, an empty program: nothing runs
    assert M.run(p.assemble(), [0] * 8, [7] * 8, 0, 4, 0, 50).executed == 0
    code = [int(w) for w in p.assemble()]
    code[4] = len(code) + (1 << 32)
    assert M.run(code, [0] * 8, [7] * 8, 0, 4, 0, 50).executed == 0
    code[4] = 16 + (3 << 32)            # modulo 2^32: the first code word
    assert M.run(code, [0] * 8, [7] * 8, 0, 4, 0, 50).executed == 14


def test_control_set_reaches_its_cases():
    """The control program does what its comments say (model alone): the
    loops are cut by the step limit inside their body, at each of its three
    instructions; the bounded loop is not; the crafted entry words land where
    they should."""
    s = C.alu_control(C.CPU_N)
    ctl, params = [int(w) for w in s.types[1].code], [0] * 8
    z = [0] * 8
    cut = {b: M.run(ctl, params, z, 0, b, 0, 10) for b in C.HEAVY}
    assert all(r.executed == P.MAX_STEPS for r in cut.values())
    # r4 counts the instructions before the loop, r2 the body's first instruction
    assert [(cut[b].state[4], cut[b].state[2]) for b in (C.C_CUT1, C.C_CUT2, C.C_CUT3)] == \
        [(1, 1365), (2, 1365), (3, 1365)]
    assert [(P.MAX_STEPS - pre) % 3 for pre in (1, 2, 3)] == [0, 2, 1]
    assert cut[C.C_LINE].state[6] == (P.MAX_STEPS + 2) // 3
    r = M.run(ctl, params, [63] + [0] * 7, 0, C.C_LOOP, 0, 10)
    assert r.state[2] == 3 * 63 and r.executed < P.MAX_STEPS
    r = M.run(ctl, params, z, 0, C.C_BRANCH, 0, 10)
    assert r.state[2] == 0b010110        # jz 0, jnz 1, jnz 2^63 are taken
    for b, want in ((C.C_J_NP, {3: C.C_J_NP}), (C.C_J_LAST, {3: C.C_J_LAST, 4: 7}),
                    (C.C_J_FIRST, {3: C.C_J_FIRST, 5: 1}), (C.C_J_TABLE, {3: C.C_J_TABLE, 2: 5}),
                    (C.C_J_NEG, {3: C.C_J_NEG}), (C.C_UNKNOWN, {2: 1}), (C.C_ENTRY_CRAFT, {6: 9}),
                    (C.C_ENTRY_ZERO, {})):
        assert M.run(ctl, params, z, 0, b, 0, 10).state == [want.get(k, 0) for k in range(8)], b
    alu = [int(w) for w in s.types[0].code]
    st = [5, 9, 0, 0, 0, 0, 0, 0]
    want = M.run(alu, params, st, 0, 0, 0, 10).state
    assert M.run(alu, params, st, 0, C.B_ENTRY_HIGH, 0, 10).state == want != st
    for b in (C.B_ENTRY_ZERO, C.B_ENTRY_NP, C.B_ENTRY_PAST):
        assert M.run(alu, params, st, 0, b, 0, 10).executed == 0
    assert M.run(alu, params, st, 0, C.B_ENTRY_TABLE, 0, 10).executed >= 1


def test_no_set_holds_a_yield_or_spawn_word():
    """No word of any set's programs — entry words included — reads as YIELD
    or SPAWN: the sets are eligible for the small-step path."""
    for name, make in C.SETS.items():
        for _, code in make(C.SPARSE_N[name]).programs():
            assert not np.isin(code & np.uint64(0xFF), [P.OPS["yield"], P.OPS["spawn"]]).any(), name


def test_programs_do_not_depend_on_the_size():
    """One run-time compiled unit per set and geometry, whatever the number
    of actors (scripts/jit_precompile.py caches the units of jit_units())."""
    for name, make in C.SETS.items():
        small, big = make(C.SPARSE_N[name]), make(C.GPU_N)
        assert small.mix_mask() == big.mix_mask()
        for (ta, a), (tb, b) in zip(small.programs(), big.programs()):
            assert ta == tb and np.array_equal(a, b), name
    assert C.ring_mix(C.GPU_N).mix_mask() == (1 << 1) | (1 << 12)


def test_random_set_conditions():
    """What the random set must exercise, checked with the model alone: every
    op of the instruction set that the generator may emit (all but YIELD and
    SPAWN) occurs in executed code; at least half of all sends go to valid
    ids and at least one is dropped; every behaviour executes at least 8
    instructions on at least one actor."""
    s = C.random_set(C.CPU_N)
    w = C.model_world(s)
    ops = set()
    C.model_play(s, executor=M.ModelExec(ops), world=w)
    assert ops == set(range(23)) - {M.YIELD, M.SPAWN}, sorted(set(range(21)) - ops)
    assert w.dropped >= 1 and w.sent >= w.dropped
    for t in w.types:
        assert all(t.most_executed.get(b, 0) >= 8 for b in range(C.RANDOM_BEHS)), t.most_executed


@pytest.mark.parametrize("name", list(C.SETS))
def test_model_equals_oracle(name):
    s, want, _ = model_of(name)
    o = pyoracle.Oracle()
    try:
        got = C.play(o, s)
    finally:
        o.shutdown()
    C.assert_same(got, want, f"oracle, {name}")
    assert want[-1][3]["delivered"] > 0
    if s.lossy:
        assert want[-1][3]["dropped"] > 0


@pytest.mark.parametrize("name", [n for n in C.SETS])
def test_generated_code_equals_model(name, tmp_path):
    """Every actor and message of the set through the host-compiled
    jit_prog_<type> functions: state, sends in order, drops, counters."""
    if not os.path.exists(LIB_PATH):
        pytest.skip(f"{LIB_PATH} is not built: no run-time step generator to ask for its source")
    assert H.compiler() is not None, "no host C++ compiler"
    s, want, wm = model_of(name)
    exe = H.build(s.programs(), str(tmp_path), name)
    wj = C.model_world(s)
    got = C.model_play(s, executor=H.HostJitExec(exe, str(tmp_path)), world=wj)
    C.assert_same(got, want, f"generated code, {name}")
    assert len(wj.sends_log) == len(wm.sends_log)
    for k, (a, b) in enumerate(zip(wj.sends_log, wm.sends_log)):
        assert a == b, (name, k, next((i, a.get(i), b.get(i)) for i in sorted(set(a) | set(b))
                                      if a.get(i) != b.get(i)))
