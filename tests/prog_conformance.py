"""Deterministic conformance program sets for GPU_ACTOR_HT_PROGRAM types
(include/gpu_actor.h): every op on edge operands, control flow at the limits
the four implementations each restate (entry words, jump targets, the step
limit), sends at the edges of the id range across two program types, a
compiled table mixed with a program type, and seeded random programs.

A set is a list of types with their programs, params and initial state, and a
list of runs: the messages the host injects before each run to quiescence.
`play` drives anything with the Engine interface (the engine, the oracle);
`model_play` drives the reference model (tests/prog_model.py). Both return one
snapshot per run — supersteps, the state of every type, the counters — and a
conforming implementation's snapshots equal the model's bit for bit.

Fixed seeds throughout; nothing depends on time or environment. Imported by
the tests and by scripts/jit_precompile.py (`jit_units`)."""
from __future__ import annotations

import random

import numpy as np

import prog_model as M
from ponyc_amd import program as P
from ponyc_amd.engine import HT_PROGRAM, HT_RING, MSG_DTYPE, NONE_ID

M64 = (1 << 64) - 1
GPU_N = 4200            # actors per type: three zones of 2048, two of 4096 (per type)
CPU_N = 600             # the CPU tests' size
SINK = 15               # the commutative behaviour: r6 += arg; r7 ^= mix(arg)

EDGES = [0, 1, 2, 63, 64, 65, (1 << 31) - 1, 1 << 31, (1 << 32) - 1, 1 << 32,
         (1 << 63) - 1, 1 << 63, M64 - 1, M64]
IMMS = [-(1 << 31), -1, 0, 1, (1 << 31) - 1]
LDP_IDX = [0, 1, 2, 3, 4, 5, 6, 7, -3, 13]        # all masked with & 7


class Prog(P.Program):
    """The assembler, with behaviours placed so that no entry word reads as a
    YIELD or SPAWN instruction (an engine that sees one in any word of a
    program keeps it off the small-step path)."""

    def behaviour(self, beh: int) -> None:
        while (P.ENTRIES + len(self.code)) & 0xFF in (P.OPS["yield"], P.OPS["spawn"]):
            self.halt()
        super().behaviour(beh)

    def pc(self) -> int:
        return P.ENTRIES + len(self.code)

    def sink(self) -> None:
        self.behaviour(SINK)
        self.add(6, 6, P.R_ARG)
        self.mix(11, P.R_ARG)
        self.xor(7, 7, 11)
        self.halt()


class TypeSpec:
    def __init__(self, ht, words, count, code=None, params=None, state=None):
        self.ht, self.words, self.count = ht, words, count
        self.code = None if code is None else np.asarray(code, dtype=np.uint64)
        self.params = dict(params or {})            # index -> value
        self.state = state                          # (words, count) uint64, or None


class Set:
    def __init__(self, name, types, runs, commutative, lossy):
        self.name, self.types, self.runs = name, types, runs
        self.commutative, self.lossy = commutative, lossy
        self.firsts = list(np.cumsum([0] + [t.count for t in types])[:-1])
        self.n_ids = int(sum(t.count for t in types))

    def programs(self):
        """[(type id, words)] of the program types: one run-time compiled unit."""
        return [(k, t.code) for k, t in enumerate(self.types) if t.ht == HT_PROGRAM]

    def mix_mask(self):
        """Bit per handler table, when a compiled table is mixed in (the
        any-mix step, compiled for this mask); else 0."""
        hts = {t.ht for t in self.types}
        return sum(1 << h for h in hts) if hts != {HT_PROGRAM} else 0


def _rng_words(rng, n):
    return np.array([rng.getrandbits(64) for _ in range(n)], dtype=np.uint64)


def _msgs(to, beh, arg):
    to = np.asarray(to, dtype=np.uint64)
    m = np.empty(to.shape[0], dtype=MSG_DTYPE)
    m["to"] = to.astype(np.uint32)
    m["behaviour"] = np.broadcast_to(np.asarray(beh, dtype=np.uint32), to.shape)
    m["arg"] = np.broadcast_to(np.asarray(arg, dtype=np.uint64), to.shape)
    return m


def _spread(n, k=64):
    """k actor indices of n that sit on both sides of every zone boundary of
    either geometry, at both ends, and in between."""
    pick = {0, 1, n - 2, n - 1}
    for b in (2048, 4096):
        for z in range(b, n, b):
            pick |= {z - 1, z}
    step = max(1, n // k)
    pick |= set(range(0, n, step))
    return np.array(sorted(i for i in pick if 0 <= i < n), dtype=np.uint64)


# ---- ALU: every result-producing op, its result in a state word of its own ----------
def alu_results():
    """(name, emit(p, d)) for each result; six per behaviour, in this order.
    Operands are r0 and r1, which no behaviour writes."""
    out = []
    for v in IMMS:
        out.append((f"ldi {v}", lambda p, d, v=v: p.ldi(d, v)))
    for v in IMMS:
        out.append((f"addi {v}", lambda p, d, v=v: p.addi(d, 0, v)))
    for k in LDP_IDX:
        out.append((f"ldp {k}", lambda p, d, k=k: p.ldp(d, k)))
    out.append(("mov", lambda p, d: p.mov(d, 0)))
    for op in ("add", "sub", "mul", "mulhi", "and_", "or_", "xor", "shl", "shr", "ltu", "eq"):
        out.append((op, lambda p, d, op=op: getattr(p, op)(d, 0, 1)))
    out.append(("mix", lambda p, d: p.mix(d, 0)))
    for op in ("sub", "ltu", "shl", "shr"):           # operands swapped
        out.append((op + " swapped", lambda p, d, op=op: getattr(p, op)(d, 1, 0)))
    out.append(("mix r1", lambda p, d: p.mix(d, 1)))
    out.append(("mul r0 r0", lambda p, d: p.mul(d, 0, 0)))
    out.append(("mulhi r1 r1", lambda p, d: p.mulhi(d, 1, 1)))
    out.append(("eq r0 r0", lambda p, d: p.eq(d, 0, 0)))
    for r in (9, 10, 11, 12, 13, 14, 15):             # self, behaviour, zero at entry
        out.append((f"r{r}", lambda p, d, r=r: p.mov(d, r)))
    assert len(out) == 48
    return out


ALU_BEHS = 8
B_ENTRY_ZERO, B_ENTRY_TABLE, B_ENTRY_NP, B_ENTRY_PAST, B_ENTRY_HIGH = 8, 9, 10, 11, 12


def alu_program():
    """Behaviours 0-7: six results each into r2-r7. Behaviours 8-12 have
    crafted entry words: 0 (does nothing), 4 (inside the entry table: the
    entry words from there on run as instructions), n (ends at once), past n,
    and 2^32 + 16 (taken modulo 2^32: behaviour 0's code). No backward jump
    and fewer words than the step limit: the compiled step counts no steps."""
    p = Prog()
    res = alu_results()
    for b in range(ALU_BEHS):
        p.behaviour(b)
        assert b or p.entries[0] == 16
        for k in range(6):
            res[6 * b + k][1](p, 2 + k)
        p.halt()
    n = p.pc()
    p.entries[B_ENTRY_ZERO] = 0
    p.entries[B_ENTRY_TABLE] = 4
    p.entries[B_ENTRY_NP] = n
    p.entries[B_ENTRY_PAST] = n + 1000
    p.entries[B_ENTRY_HIGH] = (1 << 32) + 16
    return p.assemble()


def alu_state(n, seed=0xA1):
    """Pair i of the full cross product of the edge set (with two seeded
    random words) in actor i; seeded random pairs in the rest; r2-r7 random."""
    rng = random.Random(seed)
    edge = EDGES + [rng.getrandbits(64), rng.getrandbits(64)]
    pairs = [(x, y) for x in edge for y in edge]
    assert n >= len(pairs)
    st = np.stack([_rng_words(rng, n) for _ in range(8)])
    for i, (x, y) in enumerate(pairs):
        st[0, i], st[1, i] = x, y
    return st


ALU_PARAMS = {k: (0x0123456789ABCDEF * (2 * k + 3) + (k << 60)) & M64 for k in range(8)}


# ---- control --------------------------------------------------------------------
(C_LOOP, C_CUT1, C_CUT2, C_CUT3, C_LINE, C_BRANCH, C_J_NP, C_J_LAST, C_J_FIRST, C_J_TABLE,
 C_J_NEG, C_UNKNOWN, C_ENTRY_CRAFT, C_ENTRY_ZERO) = range(14)
CRAFT_PC = 0x020D       # as an instruction: ADDI r2 = r0 + imm; as an entry: pc 525
HEAVY = (C_CUT1, C_CUT2, C_CUT3, C_LINE)    # 4096 instructions each: a few actors only
LINE_WORDS = 4200


def control_program():
    p = Prog()
    # the first code word (pc 16): the target of C_J_FIRST
    p.label("first")
    p.addi(5, 5, 1)
    p.halt()
    # a bounded backward loop: r0 & 63 trips, far below the step limit
    p.behaviour(C_LOOP)
    p.ldi(11, 63)
    p.and_(3, 0, 11)
    p.ldi(2, 0)
    p.label("loop")
    p.jz(3, "loop_end")
    p.addi(2, 2, 3)
    p.addi(3, 3, -1)
    p.jmp("loop")
    p.label("loop_end")
    p.halt()
    # endless loops of three instructions behind 1, 2 and 3 others: the step
    # limit cuts them after the body's 3rd, 1st and 2nd instruction
    for b, pre in ((C_CUT1, 1), (C_CUT2, 2), (C_CUT3, 3)):
        p.behaviour(b)
        for _ in range(pre):
            p.addi(4, 4, 1)
        p.label(f"cut{b}")
        p.addi(2, 2, 1)
        p.xor(3, 3, 2)
        p.jmp(f"cut{b}")
    # jz / jnz, taken and not, on 0, 1 and 2^63: r2 gets one bit per fall-through
    p.behaviour(C_BRANCH)
    p.ldi(11, 0)
    p.ldi(12, 1)
    p.ldi(13, 63)
    p.shl(13, 12, 13)
    p.ldi(2, 0)
    bit = 0
    for reg in (11, 12, 13):
        for j in (p.jz, p.jnz):
            j(reg, f"br{bit}")
            p.ldi(14, 1 << bit)
            p.or_(2, 2, 14)
            p.label(f"br{bit}")
            bit += 1
    p.halt()
    # jumps: to n exactly, to n - 1 (the last word runs), to the first code
    # word, into the entry table (word 13 runs as ADDI, word 14 is 0: HALT),
    # and below 0; the word behind each jump must not run
    for b, target in ((C_J_NP, "np"), (C_J_LAST, "last"), (C_J_FIRST, "first"),
                      (C_J_TABLE, "table"), (C_J_NEG, "neg")):
        p.behaviour(b)
        p.addi(3, 3, b)
        p.jmp(target)
        p.addi(3, 3, 1000)
        p.halt()
    # an unknown op (the first past SPAWN) in the middle of a block
    p.behaviour(C_UNKNOWN)
    p.addi(2, 2, 1)
    p.raw(P.word(23, 2, 2, 2, 77))
    p.addi(2, 2, 100)
    p.halt()
    # an entry word that is also an instruction, with bits above 2^32 set
    while p.pc() < CRAFT_PC:
        p.halt()
    assert p.pc() == CRAFT_PC
    p.addi(6, 6, 9)
    p.halt()
    # straight-line code longer than the step limit, cut inside it
    p.behaviour(C_LINE)
    for k in range(LINE_WORDS // 3):
        p.addi(6, 6, 1)
        p.xor(7, 7, 6)
        p.add(7, 7, 0)
    p.halt()
    p.label("last")
    p.addi(4, 4, 7)
    p.labels["np"] = len(p.code)
    p.labels["table"] = C_ENTRY_CRAFT - P.ENTRIES
    p.labels["neg"] = -P.ENTRIES - 5
    p.entries[C_ENTRY_CRAFT] = (5 << 32) | CRAFT_PC
    p.entries[C_ENTRY_ZERO] = 0
    code = p.assemble()
    assert P.MAX_STEPS < len(code) < (1 << 16)
    return code


def alu_control(n=GPU_N, heavy=64):
    """Type 0 the ALU program, type 1 the control program; run b injects
    behaviour b into every actor of each type that has one (the four
    4096-instruction behaviours into `heavy` actors spread over the zones)."""
    rng = random.Random(0xC7)
    t0 = TypeSpec(HT_PROGRAM, 8, n, alu_program(), ALU_PARAMS, alu_state(n))
    t1 = TypeSpec(HT_PROGRAM, 8, n, control_program(), {0: 1, 1: M64},
                  np.stack([_rng_words(rng, n) for _ in range(8)]))
    ids = np.arange(n, dtype=np.uint64)
    runs = []
    for b in range(14):
        m = []
        if b <= B_ENTRY_HIGH:
            m.append(_msgs(ids, b, rng.getrandbits(64)))
        sel = _spread(n, heavy) if b in HEAVY else ids
        m.append(_msgs(sel + np.uint64(n), b, rng.getrandbits(64)))
        runs.append(np.concatenate(m))
    return Set("alu_control", [t0, t1], runs, {}, lossy=False)


# ---- sends and types -----------------------------------------------------------------
def _send_program(variant):
    """Behaviour 0: three sends — to r0, to the sender itself, to r2 — with
    the behaviour immediates 0x1F and -1 (both arrive as 15). Behaviour 1: a
    target computed from the type's params (the other type's first id and
    count). The two variants differ in order, arguments and params used."""
    p = Prog()
    p.behaviour(0)
    if variant == 0:
        p.send(0, 0x1F, 1)
        p.mix(11, 1)
        p.send(P.R_SELF, -1, 11)
        p.send(2, SINK, P.R_ARG)
    else:
        p.ldp(12, 3)
        p.xor(11, 1, 12)
        p.send(P.R_SELF, 0x1F, 11)
        p.send(2, -1, 1)
        p.add(13, 1, P.R_ARG)
        p.send(0, -1, 13)
    p.addi(3, 3, 1)
    p.halt()
    p.behaviour(1)
    p.ldp(11, 2)
    p.xor(11, 11, 1)
    if variant:
        p.xor(11, 11, P.R_ARG)
    p.mix(11, 11)
    p.ldp(12, 1)
    p.mulhi(11, 11, 12)
    p.ldp(12, 0)
    p.add(11, 11, 12)
    p.send(11, 0x1F if variant else -1, P.R_SELF)
    p.mov(4, 11)
    p.halt()
    p.sink()
    return p.assemble()


def _edge_targets(n_ids):
    return [n_ids - 1, n_ids, 1 << 32, (1 << 32) + 5, M64]


def sends(n=GPU_N):
    """Two program types that send to each other. r0 holds an actor of the
    other type, r2 a valid actor of either — or, in a few actors of every
    zone, an edge of the id range: n_ids - 1, n_ids, 2^32 (a truncating check
    would alias it to id 0), 2^32 + 5 and 2^64 - 1."""
    rng = random.Random(0x5E)
    n_ids = 2 * n
    types = []
    for k in range(2):
        other = (1 - k) * n
        st = np.stack([_rng_words(rng, n) for _ in range(8)])
        st[0] = np.array([other + rng.randrange(n) for _ in range(n)], dtype=np.uint64)
        st[2] = np.array([rng.randrange(n_ids) for _ in range(n)], dtype=np.uint64)
        edge = _edge_targets(n_ids)
        for j, i in enumerate(_spread(n, 8)):
            st[2, int(i)] = edge[(j + k) % len(edge)]
        params = {0: other, 1: n, 2: rng.getrandbits(64), 3: rng.getrandbits(64)}
        types.append(TypeSpec(HT_PROGRAM, 8, n, _send_program(k), params, st))
    ids = np.arange(n_ids, dtype=np.uint64)
    runs = [_msgs(ids, 0, 0xD00D), _msgs(ids, 1, ids * np.uint64(0x9E3779B97F4A7C15))]
    return Set("sends", types, runs, {0: {SINK}, 1: {SINK}}, lossy=True)


# ---- a compiled table mixed with a program type ------------------------------------
RING_SIZE = 7


def ring_pass_model(st, self_id, beh, arg):
    """GPU_ACTOR_HT_RING as include/gpu_actor.h states it: SET stores the
    neighbour; PASS counts, and forwards arg - 1 or counts the print."""
    if beh == 0:
        st[0] = arg
        return []
    st[2] = (st[2] + 1) & M64
    if arg > 0:
        return [(st[0], 1, arg - 1)] if st[0] != NONE_ID else []
    st[3] = (st[3] + 1) & M64
    return []


def ring_state(first, n, size):
    """The ring constructor: actor k of ring j gets id k % size + 1 and the
    next actor of its ring, wrapping; id 1's next comes by SET."""
    st = np.zeros((4, n), dtype=np.uint64)
    for i in range(n):
        pos = i % size
        st[0, i] = NONE_ID if pos == 0 else first + (i // size) * size + (pos + 1) % size
        st[1, i] = pos + 1
    return st


def ring_mix(n=GPU_N):
    """The ring table (type 0) and a program type (type 1) whose behaviour 0
    sends pass(0) to the ring actor in r0 and to the one in r2, and the sink
    to itself: the any-mix step with the interpreter compiled in."""
    rng = random.Random(0x41)
    n_ring = n // RING_SIZE * RING_SIZE
    p = Prog()
    p.behaviour(0)
    p.send(0, 1, 11)                    # pass(0): r11 is zero at entry
    p.send(P.R_SELF, -1, 1)
    p.send(2, 1, 11)
    p.addi(3, 3, 1)
    p.halt()
    p.sink()
    st = np.stack([_rng_words(rng, n) for _ in range(8)])
    st[0] = np.array([rng.randrange(n_ring) for _ in range(n)], dtype=np.uint64)
    st[2] = np.array([rng.randrange(n_ring) for _ in range(n)], dtype=np.uint64)
    t0 = TypeSpec(HT_RING, 4, n_ring, None, {0: RING_SIZE}, None)
    t1 = TypeSpec(HT_PROGRAM, 8, n, p.assemble(), {}, st)
    runs = [_msgs(np.arange(n, dtype=np.uint64) + np.uint64(n_ring), 0, 3)]
    return Set("ring_mix", [t0, t1], runs, {0: {1}, 1: {SINK}}, lossy=False)


# ---- random programs --------------------------------------------------------------
RANDOM_SEED = 20240611
# behaviours per type. The instruction set allows 15 beside the sink, but the
# run-time compiled step of two types of 15 such behaviours — branchy code over
# 16 live registers, inlined into both step kernels — takes hiprtc more than
# ten minutes per geometry (3 behaviours: 80 s); 4 keep the build's warm-up short
RANDOM_BEHS = 4
_ALU3 = ["add", "sub", "mul", "mulhi", "and", "or", "xor", "shl", "shr", "ltu", "eq"]


def _random_behaviour(p, rng, tag):
    """20 to 40 instructions, forward jumps only, at most three sends, each
    target a hash of a register and the sender's id, scaled into
    [0, n_ids + 3) by a MULHI against param 7."""
    n = rng.randrange(20, 41)
    body = []                               # (kind, ...) per instruction slot
    inside = set()                          # slots a jump must not land on: a send's scaling
    sends_left = 3
    while len(body) < n:
        c = rng.random()
        d, a, b = rng.randrange(16), rng.randrange(16), rng.randrange(16)
        if d in (9, 14, 15):
            d = rng.randrange(8)            # r9 (self), r14 and r15 make the send targets
        if c < 0.50:
            body.append(("op", rng.choice(_ALU3), d, a, b, 0))
        elif c < 0.58:
            body.append(("op", "ldi", d, 0, 0, rng.choice(IMMS + [rng.randrange(-999, 999)])))
        elif c < 0.64:
            body.append(("op", "ldp", d, 0, 0, rng.randrange(-8, 16)))
        elif c < 0.70:
            body.append(("op", "addi", d, a, 0, rng.choice(IMMS + [rng.randrange(-999, 999)])))
        elif c < 0.76:
            body.append(("op", "mov", d, a, 0, 0))
        elif c < 0.82:
            body.append(("op", "mix", d, a, 0, 0))
        elif c < 0.92:
            body.append(("jump", rng.choice(["jz", "jnz", "jmp"]), a, rng.randrange(1, 5)))
        elif sends_left and len(body) + 5 <= n:
            sends_left -= 1
            inside |= {len(body) + k for k in (1, 2, 3, 4)}
            body.append(("op", "add", 14, a, 9, 0))     # differs from actor to actor
            body.append(("op", "mix", 14, 14, 0, 0))
            body.append(("op", "ldp", 15, 0, 0, 7))
            body.append(("op", "mulhi", 14, 14, 15, 0))
            body.append(("op", "send", 0, 14, b, rng.choice([SINK, 0x1F, -1])))
    for k, ins in enumerate(body):
        p.label(f"{tag}_{k}")
        if ins[0] == "op":
            _, name, d, a, b, imm = ins
            p._op(name, d, a, b, imm)
        else:
            _, name, a, skip = ins
            to = min(k + 1 + skip, len(body))
            while to in inside:
                to -= 1
            p._jump(name, a, f"{tag}_{to}")
    p.label(f"{tag}_{len(body)}")
    p.halt()


def random_programs(seed=RANDOM_SEED):
    rng = random.Random(seed)
    out = []
    for t in range(2):
        p = Prog()
        for b in range(RANDOM_BEHS):
            p.behaviour(b)
            _random_behaviour(p, rng, f"t{t}b{b}")
        p.sink()
        out.append(p.assemble())
    return out


def random_set(n=GPU_N, seed=RANDOM_SEED):
    """Two types of RANDOM_BEHS random behaviours and the sink. Run 0 gives
    actor i behaviour i % RANDOM_BEHS, run 1 behaviour (7 i + 3) % RANDOM_BEHS."""
    rng = random.Random(seed ^ 0xFFFF)
    n_ids = 2 * n
    types = []
    for code in random_programs(seed):
        params = {k: rng.getrandbits(64) for k in range(7)}
        params[7] = n_ids + 3
        types.append(TypeSpec(HT_PROGRAM, 8, n, code, params,
                              np.stack([_rng_words(rng, n) for _ in range(8)])))
    ids = np.arange(n_ids, dtype=np.uint64)
    nb = np.uint64(RANDOM_BEHS)
    runs = [_msgs(ids, ids % nb, ids * np.uint64(0xD6E8FEB86659FD93)),
            _msgs(ids, (ids * np.uint64(7) + np.uint64(3)) % nb, _rng_words(rng, n_ids))]
    return Set("random", types, runs, {0: {SINK}, 1: {SINK}}, lossy=True)


SETS = {"alu_control": alu_control, "sends": sends, "ring_mix": ring_mix, "random": random_set}
# the small-step path holds 1024 records a step: sizes at which every step fits
SPARSE_N = {"alu_control": 256, "sends": 160, "ring_mix": 161, "random": 160}


def jit_units():
    """What an engine running these sets compiles at run time, for
    scripts/jit_precompile.py: (programs or mix mask, z12). No program
    depends on the number of actors (params carry every count and id)."""
    out = []
    for name, make in SETS.items():
        s = make(SPARSE_N[name])
        for z12 in (False, True):
            out.append((s.mix_mask() or s.programs(), z12))
    return out


# ---- driving -----------------------------------------------------------------------
def setup(e, s):
    for k, t in enumerate(s.types):
        e.type_register(k, t.words, t.ht)
        if t.code is not None:
            e.type_program(k, t.code)
        for idx, v in t.params.items():
            e.type_param(k, idx, v)
    for k, t in enumerate(s.types):
        first = e.create(k, t.count)
        assert first == s.firsts[k]
        if t.state is not None:
            e.state_write(k, t.state)


def play(e, s):
    """[(supersteps, return code, [state per type], counters)] per run."""
    setup(e, s)
    out = []
    for m in s.runs:
        e.sendv(m)
        try:
            steps, rc = e.run(), 0
        except Exception as exc:            # a dropped send: EMAILBOX after finishing
            if not s.lossy or getattr(exc, "code", None) != -4:
                raise
            steps, rc = None, -4
        c = e.counts()
        out.append((steps, rc, [e.state_read(k) for k in range(len(s.types))],
                    {k: c[k] for k in ("steps", "delivered", "sent", "dropped", "pending")}))
    return out


def model_world(s):
    types = []
    for k, t in enumerate(s.types):
        if t.ht == HT_RING:
            st = ring_state(s.firsts[k], t.count, t.params[0])
            types.append(M.ModelType(s.firsts[k], t.count, [list(map(int, c)) for c in st.T],
                                     table=ring_pass_model))
        else:
            params = [t.params.get(i, 0) for i in range(8)]
            types.append(M.ModelType(s.firsts[k], t.count, [list(map(int, c)) for c in t.state.T],
                                     code=t.code, params=params))
    return M.World(types, s.commutative)


def model_play(s, executor=None, world=None):
    w = world or model_world(s)
    out = []
    for m in s.runs:
        w.inject(zip(m["to"].tolist(), m["behaviour"].tolist(), m["arg"].tolist()))
        steps = w.drive(executor)
        states = [np.array(t.state, dtype=np.uint64).T.copy() for t in w.types]
        out.append((steps, -4 if w.dropped else 0, states, w.counts()))
    return out


def assert_same(got, want, what):
    """Snapshots of `play` against the model's, bit for bit."""
    assert len(got) == len(want)
    for r, ((gs, grc, gst, gc), (ws, wrc, wst, wc)) in enumerate(zip(got, want)):
        for k, (a, b) in enumerate(zip(gst, wst)):
            if not np.array_equal(a, b):
                w, i = np.argwhere(a != b)[0]
                raise AssertionError(f"{what}: run {r} type {k} actor {i} word {w}: "
                                     f"{int(a[w, i]):#x} != model {int(b[w, i]):#x} "
                                     f"({int((a != b).any(axis=0).sum())} actors differ)")
        assert gc == wc, (what, r, gc, wc)
        assert grc == wrc, (what, r, grc, wrc)
        if gs is not None:                  # (a lossy run raises: its steps are in the counters)
            assert gs == ws, (what, r, gs, ws)
