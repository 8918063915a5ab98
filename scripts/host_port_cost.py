"""Cost of messages to the host where they are used:
1,048,576 program actors (ponyc_amd.program.emitter_program, BURST(1)), each
sending one message per step besides its own BURST, to
  a) one of 1,048,576 other program actors (ordinary mail: outbox, landing) —
     actor (index + c) % N, a spread target, not a drawn one: the program has
     no generator,
  b) one of 4 host ports,
  c) one host port.
Per case: the step time of gpu_actor_run_fixed (events around the launches;
ports: nothing collected inside) and the wall time per step of gpu_actor_run,
which collects after every step; their difference is the collection.

    python scripts/host_port_cost.py --precompile     # no GPU: warm the JIT cache
    python scripts/host_port_cost.py [--steps 8]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np                                   # noqa: E402

from ponyc_amd import program as P                   # noqa: E402
from ponyc_amd.engine import (Engine, HT_PROGRAM, HT_HOST_PORT, MSG_DTYPE, jit_compile)  # noqa: E402

N = 1 << 20


def idle_program() -> np.ndarray:
    p = P.Program()
    p.behaviour(0)
    p.addi(0, 0, 1)
    p.halt()
    return p.assemble()


def setup(e, case: str, steps: int) -> None:
    e.type_register(0, 8, HT_PROGRAM)
    e.type_program(0, P.emitter_program())
    first = e.create(0, N)
    if case == "a":
        e.type_register(1, 8, HT_PROGRAM)
        e.type_program(1, idle_program())
        targets = N
    else:
        e.type_register(1, 1, HT_HOST_PORT)
        targets = 4 if case == "b" else 1
    tfirst = e.create(1, targets)
    for k, v in enumerate([tfirst, targets, ((1 << 64) // targets + 1) & (2**64 - 1), first, steps]):
        e.type_param(0, k, v)
    m = np.empty(N, dtype=MSG_DTYPE)
    m["to"] = first + np.arange(N, dtype=np.uint32)
    m["behaviour"] = 0
    m["arg"] = 1
    e.sendv(m)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--precompile", action="store_true")
    a = ap.parse_args()
    if a.precompile:
        for z12 in (False, True):
            jit_compile([(0, P.emitter_program())], z12)
            jit_compile([(0, P.emitter_program()), (1, idle_program())], z12)
        return
    for case in "abc":
        out = {"case": case, "actors": N, "steps": a.steps}
        for mode in ("fixed", "run"):
            with Engine(max_actors=1 << 22) as e:
                if case != "a":
                    e.host_reserve(N * a.steps if mode == "fixed" else N)
                setup(e, case, a.steps + 1)
                e.run_fixed(1)                        # the first step (module load) apart
                e.recv()
                e.sync()
                t = time.perf_counter()
                if mode == "fixed":
                    e.run_fixed(a.steps - 1)
                    out["fixed_step_us"] = round(e.last_drain_ms() * 1e3, 1)
                    e.sync()
                    out["fixed_wall_step_us"] = round((time.perf_counter() - t) / (a.steps - 1) * 1e6, 1)
                    t = time.perf_counter()
                    got = e.recv()
                    out["deferred_collect_ms"] = round((time.perf_counter() - t) * 1e3, 2)
                else:
                    k = e.run(a.steps - 1)
                    out["run_wall_step_us"] = round((time.perf_counter() - t) / max(k, 1) * 1e6, 1)
                    got = e.recv()
                out[mode + "_received"] = int(got.shape[0])
                c = e.counts()
                out[mode + "_dropped"] = c["dropped"]
                out["jit"] = e.debug_info()["jit"]
        print("HOSTPORT_COST " + json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
