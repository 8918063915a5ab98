"""One rank of tests/test_gpu_plan_pairs.py's two-rank case (launched through
torch.distributed.run like tests/mr_worker.py, every rank on the one GPU over
the host transport): 2048 * 3 pingers, so that every zone's sends to the peer
rank go through the plan path's exchange bucket. Rank 0 checks against the
single-rank CPU oracle and prints one `MR_RESULT {json}` line, with the zone
steps that took the plan path summed over the ranks."""
import ctypes
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


def setup(e):
    return W.ubench(e, 2048 * 3, 5, 20)


def main():
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    eng = Engine(device=0, n_ranks=world, rank=rank, transport=GlooTransport())
    w = setup(eng)
    steps = eng.run(0)
    c = eng.counts()
    out = (ctypes.c_uint64 * 21)()
    fn = eng.lib.gpu_actor_debug_info
    fn.argtypes = [ctypes.c_void_p, ctypes.c_uint64]
    fn.restype = ctypes.c_int
    assert fn(out, 21) == 0
    plan = torch.tensor([int(out[20])], dtype=torch.int64)
    dist.all_reduce(plan)
    res = W.ubench_result(GlobalView(eng), w)
    eng.shutdown()
    if rank == 0:
        import pyoracle
        o = pyoracle.Oracle()
        wo = setup(o)
        so = o.run(0)
        co = o.counts()
        ro = W.ubench_result(o, wo)
        o.shutdown()
        print("MR_RESULT " + json.dumps({
            "world": world,
            "state_equal": bool(np.array_equal(res, ro)),
            "steps": [int(steps), int(so)],
            "delivered": [c["delivered"], co["delivered"]],
            "sent": [c["sent"], co["sent"]],
            "pending": [c["pending"], co["pending"]],
            "by_type": c["delivered_by_type"] == co["delivered_by_type"],
            "dropped": c["dropped"], "remote": c["remote"], "plan_zones": int(plan[0]),
        }), flush=True)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
