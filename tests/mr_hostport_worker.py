"""One rank of the two-rank host-port run (launched by
tests/test_gpu_host_port.py via torch.distributed.run; every rank drives the
same GPU through the host transport). Each rank receives the messages its own
actors sent to host ports; rank 0 gathers the lists, merges them by key, checks
the merged list against the oracle's stand-ins (tests/host_port_checks.py) and
prints one `MR_RESULT {json}` line."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np                       # noqa: E402
import torch.distributed as dist         # noqa: E402

import host_port_checks as H             # noqa: E402
from ponyc_amd.dist import GlooTransport, GlobalView   # noqa: E402
from ponyc_amd.engine import Engine      # noqa: E402


def main():
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    eng = Engine(device=0, n_ranks=world, rank=rank, transport=GlooTransport())
    w = H.world(eng, H.SMALL)
    steps = eng.run(0)
    msgs = eng.recv()
    c = eng.counts()                     # summed over ranks by the library
    emit = GlobalView(eng).state_read(w["emit_type"])
    eng.shutdown()
    parts = [None] * world
    dist.all_gather_object(parts, (rank, msgs))
    if rank == 0:
        parts.sort(key=lambda p: p[0])
        own = [bool((m["from"] % world == r).all()) for r, m in parts]
        merged = np.concatenate([m for _, m in parts])
        merged = merged[np.lexsort((merged["seq"], merged["from"], merged["step"]))]
        try:
            H.check_structure(merged, w)
            H.check_a(merged, steps, c, emit, H.SMALL)
            H.check_b(merged, H.SMALL)
            checks = "ok"
        except AssertionError as e:
            checks = f"failed: {e!r}"[:1500]
        out = {"world": world, "own_senders_only": own, "received": [int(m.shape[0]) for _, m in parts],
               "checks": checks, "remote": int(c["remote"]), "steps": int(steps)}
        print("MR_RESULT " + json.dumps(out), flush=True)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
