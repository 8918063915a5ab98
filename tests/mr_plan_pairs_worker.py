"""One rank of tests/test_gpu_plan_pairs.py's two-rank case (launched through
torch.distributed.run like tests/mr_worker.py, every rank on the one GPU over
the host transport): 2048 * 3 pingers, so that every zone's sends to the peer
rank go through the plan path's exchange bucket. Rank 0 checks against the
single-rank CPU oracle and prints one `MR_RESULT {json}` line, with the zone
steps that took the plan path summed over the ranks.

With an argument `extra` (tests/test_gpu_limits.py): 4,096 pingers, 7 pings
each and one more to the first `extra` ids, run one step and then to
quiescence; the line also has the zone steps that planned in that first step
(each rank's one zone holds 14,336 + extra / 2 messages in it, on either side
of the two-rank sequence limit 16,382 at extra 4,090 and 4,092)."""
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
from test_gpu_plan_pairs import plan_zones   # noqa: E402  (this rank's zone steps that planned)


EXTRA = int(sys.argv[1]) if len(sys.argv) > 1 else None


def setup(e):
    if EXTRA is None:
        return W.ubench(e, 2048 * 3, 5, 20)
    w = W.ubench(e, 4096, 7, budget=40)
    W._sendv(e, W._msgs(w["first"] + np.arange(EXTRA, dtype=np.uint64), W.PINGER_PING, 42))
    return w


def main():
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    eng = Engine(device=0, n_ranks=world, rank=rank, transport=GlooTransport())
    w = setup(eng)
    steps, first = 0, 0
    if EXTRA is not None:
        steps = eng.run(1)
        first = plan_zones(eng)
    steps += eng.run(0)
    c = eng.counts()
    plan = torch.tensor([plan_zones(eng), first], dtype=torch.int64)
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
            "plan_zones_first": int(plan[1]),
        }), flush=True)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
