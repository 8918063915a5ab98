"""A reference model of the GPU_ACTOR_HT_PROGRAM instruction set, written from
the comment block in include/gpu_actor.h alone: plain Python integers masked to
64 bits, one `if` per op. It is the independent statement that the CPU oracle
(oracle/bsp.c run_program), the device interpreters and the run-time compiled
step (csrc/jit_host.h) are all compared with (tests/test_program_conformance.py,
tests/test_gpu_program_conformance.py).

`run` executes one behaviour for one message. `drive` is the smallest world
around it: supersteps in which every actor with mail handles it in order, and
what it sends is delivered in the next superstep. Messages that behaviours
send must go to behaviours declared commutative, so the model never has to
know in which order a step's arrivals are queued."""
from __future__ import annotations

from collections import namedtuple

M64 = (1 << 64) - 1
ENTRIES = 16
MAX_STEPS = 4096
(HALT, LDI, LDP, MOV, ADD, SUB, MUL, MULHI, AND, OR, XOR, SHL, SHR, ADDI, LTU, EQ,
 JZ, JNZ, JMP, SEND, MIX, YIELD, SPAWN) = range(23)
MAX_TYPES = 16                      # GPU_ACTOR_MAX_TYPES
DEFAULT_BATCH = 100                 # messages an actor handles per superstep

Result = namedtuple("Result", "state sends dropped yields spawns executed ops")


def mix(x: int) -> int:
    z = (x + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def run(code, params, state8, self_id, beh, arg, n_ids, ops=None) -> Result:
    """One behaviour. `code`: the program's words (ints); `params`: the type's
    8 params; returns the state afterwards, the sends in order as (to, beh,
    arg), the dropped count, the yield requests, the spawn requests as (type,
    beh, arg), and the number of instructions executed. `ops`, a set, collects
    the ops executed."""
    code = [int(w) for w in code] if not isinstance(code, list) else code
    n = len(code)
    state8 = [int(v) for v in state8]
    sends, spawns = [], []
    dropped = yields = executed = 0
    if n <= ENTRIES:
        return Result(state8, sends, 0, 0, spawns, 0, ops)
    pc = code[beh & 15] & 0xFFFFFFFF
    if pc == 0:
        return Result(state8, sends, 0, 0, spawns, 0, ops)
    r = state8 + [arg & M64, self_id, beh, 0, 0, 0, 0, 0]
    while executed < MAX_STEPS and 0 <= pc < n:
        ins = code[pc]
        pc += 1
        executed += 1
        op, d = ins & 0xFF, (ins >> 8) & 15
        x, y = r[(ins >> 12) & 15], r[(ins >> 16) & 15]
        imm = (ins >> 32) & 0xFFFFFFFF
        if imm >= 1 << 31:
            imm -= 1 << 32
        if ops is not None:
            ops.add(op)
        if op == HALT or op > SPAWN:
            break
        if op == LDI:
            r[d] = imm & M64
        elif op == LDP:
            r[d] = params[imm & 7]
        elif op == MOV:
            r[d] = x
        elif op == ADD:
            r[d] = (x + y) & M64
        elif op == SUB:
            r[d] = (x - y) & M64
        elif op == MUL:
            r[d] = (x * y) & M64
        elif op == MULHI:
            r[d] = (x * y) >> 64
        elif op == AND:
            r[d] = x & y
        elif op == OR:
            r[d] = x | y
        elif op == XOR:
            r[d] = x ^ y
        elif op == SHL:
            r[d] = (x << (y & 63)) & M64
        elif op == SHR:
            r[d] = x >> (y & 63)
        elif op == ADDI:
            r[d] = (x + imm) & M64
        elif op == LTU:
            r[d] = 1 if x < y else 0
        elif op == EQ:
            r[d] = 1 if x == y else 0
        elif op == JZ:
            if x == 0:
                pc += imm
        elif op == JNZ:
            if x != 0:
                pc += imm
        elif op == JMP:
            pc += imm
        elif op == SEND:
            if x < n_ids:
                sends.append((x, imm & 15, y))
            else:
                dropped += 1
        elif op == MIX:
            r[d] = mix(x)
        elif op == YIELD:
            yields += 1
        elif op == SPAWN:
            if (imm & 0xFF) < MAX_TYPES:
                spawns.append((imm & 0xFF, (imm >> 8) & 15, y))
            else:
                dropped += 1
    return Result(r[:8], sends, dropped, yields, spawns, executed, ops)


class ModelType:
    """One actor type of a model world: `first` id, `count` actors, `state`
    as a list of per-actor 8-word lists, and either a program (`code`,
    `params`) or `table`, a function (state, self, beh, arg) -> sends for a
    compiled handler table the model restates."""

    def __init__(self, first, count, state, code=None, params=None, table=None, batch=0):
        self.first, self.count, self.state = first, count, state
        self.code = [int(w) for w in code] if code is not None else None
        self.params = [int(p) for p in (params or [0] * 8)]
        self.table = table
        self.batch = batch or DEFAULT_BATCH
        self.most_executed: dict = {}        # behaviour -> most instructions one actor ran


class ModelExec:
    """Runs one actor's share of a superstep with `run`. (The host-compiled
    run-time step of tests/prog_jit_host.py has the same interface.)"""

    def __init__(self, ops=None):
        self.ops = ops

    def step(self, world, jobs):
        """jobs: [(type index, actor id, state8, [(beh, arg), ...])] ->
        [(state8, sends, dropped, handled, executed per message)]"""
        out = []
        for ti, a, st, msgs in jobs:
            t = world.types[ti]
            sends, dropped, handled, ex = [], 0, 0, []
            for beh, arg in msgs:
                handled += 1
                if t.table is not None:
                    st = list(st)
                    sends += t.table(st, a, beh, arg)
                    ex.append(0)
                    continue
                res = run(t.code, t.params, st, a, beh, arg, world.n_ids, self.ops)
                if res.spawns:
                    raise NotImplementedError("the driver places no spawned actors")
                st = res.state
                sends += res.sends
                dropped += res.dropped
                ex.append(res.executed)
                if res.yields:
                    break
            out.append((st, sends, dropped, handled, ex))
        return out


class World:
    def __init__(self, types, commutative):
        """`types`: ModelType list, ids contiguous from 0 in list order;
        `commutative`: {type index: behaviours whose handling commutes} — the
        only ones that behaviours may send to."""
        self.types = types
        self.commutative = commutative
        self.n_ids = sum(t.count for t in types)
        self.mail: dict = {}
        self.steps = self.delivered = self.sent = self.dropped = 0
        self.sends_log: list = []       # per superstep: {actor id: [(to, beh, arg), ...]}

    def type_of(self, a):
        for k, t in enumerate(self.types):
            if t.first <= a < t.first + t.count:
                return k
        raise ValueError(a)

    def inject(self, msgs):
        """Host sends, in call order."""
        for to, beh, arg in msgs:
            self.mail.setdefault(int(to), []).append((int(beh), int(arg)))

    @property
    def pending(self):
        return sum(len(q) for q in self.mail.values())

    def drive(self, executor=None) -> int:
        """Supersteps until no mail is pending; returns how many ran."""
        executor = executor or ModelExec()
        done = 0
        while self.pending:
            jobs, rest = [], {}
            for a in sorted(self.mail):
                q = self.mail[a]
                if not q:
                    continue
                ti = self.type_of(a)
                t = self.types[ti]
                # an actor that handles a full batch becomes overloaded and
                # mutes its senders: not modelled, so no set may get there
                assert len(q) < t.batch, f"actor {a}: {len(q)} messages reach the batch"
                jobs.append((ti, a, t.state[a - t.first], q))
            arrivals, log = [], {}
            for (ti, a, _, q), (st, sends, dropped, handled, ex) in zip(jobs, executor.step(self, jobs)):
                t = self.types[ti]
                t.state[a - t.first] = list(st)
                self.delivered += handled
                self.dropped += dropped
                self.sent += len(sends)
                if handled < len(q):
                    rest[a] = q[handled:]
                for (beh, _), n in zip(q, ex):
                    t.most_executed[beh & 15] = max(t.most_executed.get(beh & 15, 0), n)
                if sends:
                    log[a] = list(sends)
                arrivals += sends
            for to, beh, arg in arrivals:
                assert (beh & 15) in self.commutative.get(self.type_of(to), ()), \
                    f"send to behaviour {beh} of actor {to}, which is not declared commutative"
                rest.setdefault(to, []).append((beh, arg))
            self.mail = rest
            self.sends_log.append(log)
            self.steps += 1
            done += 1
        return done

    def counts(self):
        return {"steps": self.steps, "delivered": self.delivered, "sent": self.sent,
                "dropped": self.dropped, "pending": self.pending}
