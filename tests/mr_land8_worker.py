"""One rank of tests/test_gpu_land8.py's two-rank cases (launched through
torch.distributed.run like tests/mr_worker.py, every rank on the one GPU over
the host transport). A rank's own zones take the plan path's records from the
compact landing lane; the peer's arrive as 16-byte exchange records in the
same zones. Rank 0 checks against the single-rank CPU oracle and prints one
`MR_RESULT {json}` line; the debug counters come as [rank 0, rank 1] lists.

  steady   2048 * 3 pingers x 5 pings, 8 steps
  grow     6144 pingers x 1 ping with a mailbox capacity of 1, 6 steps: a zone
           holds as many records as it has pingers, so about every second zone
           gets more than that from the two lanes together — the lane asks for
           the host on one rank, every rank's next step halts, and all ranks
           expand and grow together
  fixed    the steady shape through run_fixed(3), run(2), run_fixed(3)"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import numpy as np                       # noqa: E402
import torch                             # noqa: E402
import torch.distributed as dist         # noqa: E402

from ponyc_amd import workloads as W     # noqa: E402
from ponyc_amd.dist import GlooTransport, GlobalView   # noqa: E402
from ponyc_amd.engine import Engine      # noqa: E402


CASE = sys.argv[1]
STEPS = {"steady": 8, "grow": 6, "fixed": 8}[CASE]


def setup(e):
    if CASE == "grow":
        return W.ubench(e, 6144, 1, 1000, mailbox_cap=1)
    return W.ubench(e, 2048 * 3, 5, 100)


def main():
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    eng = Engine(device=0, n_ranks=world, rank=rank, transport=GlooTransport())
    w = setup(eng)
    if CASE == "fixed":
        eng.run_fixed(3)
        steps = 3 + eng.run(2)
        eng.run_fixed(3)
        eng.sync()
        steps += 3
    else:
        steps = eng.run(STEPS)
    c = eng.counts()
    d = eng.debug_info()
    keys = ["plan_zones", "land8_records", "fixups", "zones"]
    mine = torch.zeros(world, len(keys), dtype=torch.int64)
    mine[rank] = torch.tensor([d[k] for k in keys], dtype=torch.int64)
    dist.all_reduce(mine)
    res = W.ubench_result(GlobalView(eng), w)
    eng.shutdown()
    if rank == 0:
        import pyoracle
        o = pyoracle.Oracle()
        wo = setup(o)
        so = o.run(STEPS)
        co = o.counts()
        ro = W.ubench_result(o, wo)
        o.shutdown()
        out = {
            "world": world,
            "state_equal": bool(np.array_equal(res, ro)),
            "steps": [int(steps), int(so)],
            "delivered": [c["delivered"], co["delivered"]],
            "sent": [c["sent"], co["sent"]],
            "pending": [c["pending"], co["pending"]],
            "by_type": c["delivered_by_type"] == co["delivered_by_type"],
            "dropped": c["dropped"], "remote": c["remote"],
        }
        for i, k in enumerate(keys):
            out[k] = [int(v) for v in mine[:, i]]
        print("MR_RESULT " + json.dumps(out), flush=True)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
