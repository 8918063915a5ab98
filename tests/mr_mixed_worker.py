"""One rank of a multi-rank run of a mixed world (tests/mixed_worlds.py),
launched by tests/test_gpu_mixed.py like tests/mr_worker.py: every rank drives
device 0 through the host transport. `--bits b` goes to Engine(block_bits=b);
without it the engine takes the default placement. Rank 0 runs the CPU oracle,
which knows no ranks, and prints one `MR_RESULT {json}` line: final state of
every part, counts and step count must match it bit for bit."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np                       # noqa: E402
import torch                             # noqa: E402
import torch.distributed as dist         # noqa: E402

import mixed_worlds as MW                # noqa: E402
from ponyc_amd.dist import GlooTransport, GlobalView   # noqa: E402
from ponyc_amd.engine import Engine      # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("world")
    ap.add_argument("--bits", type=int, default=None)
    a = ap.parse_args()
    dist.init_process_group("gloo")
    rank, world_size = dist.get_rank(), dist.get_world_size()
    world = MW.WORLDS[a.world]
    eng = Engine(device=0, n_ranks=world_size, rank=rank, transport=GlooTransport(),
                 block_bits=a.bits, **world.eng_kw)
    w = world.setup(eng)
    steps = eng.run(0)
    c = eng.counts()
    info = eng.debug_info()
    res = world.result(GlobalView(eng), w)
    # `remote` and the plan-path count are per rank: summed over the ranks
    both = torch.tensor([c["remote"], info["plan_zones"]], dtype=torch.int64)
    dist.all_reduce(both)
    eng.shutdown()
    if rank == 0:
        import pyoracle
        o = pyoracle.Oracle()
        wo = world.setup(o)
        so = o.run(0)
        co = o.counts()
        ro = world.result(o, wo)
        o.shutdown()
        out = {
            "world": a.world, "ranks": world_size,
            "state_equal": bool(np.array_equal(res, ro)),
            "steps": [int(steps), int(so)],
            "delivered": [c["delivered"], co["delivered"]],
            "sent": [c["sent"], co["sent"]],
            "pending": [c["pending"], co["pending"]],
            "by_type": c["delivered_by_type"] == co["delivered_by_type"],
            "dropped": c["dropped"], "remote": int(both[0]), "plan_zones": int(both[1]),
            "block_bits": info["block_bits"], "zone_bits": info["zone_bits"],
        }
        print("MR_RESULT " + json.dumps(out), flush=True)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
