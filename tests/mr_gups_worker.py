"""One rank of a multi-rank gups run (launched by tests/test_gpu_gups_sharded.py
via torch.distributed.run; every rank drives device 0 through the host
transport).  The shape `W.gups(e, logtable, updaters, streamers, chunk,
iterate)` comes from the command line.  Rank 0 runs the CPU oracle on the same
shape and prints one `MRG_RESULT {json}` line: the table and the counts against
the oracle's, and every rank's debug_info."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import numpy as np                       # noqa: E402
import torch.distributed as dist         # noqa: E402

from ponyc_amd import workloads as W     # noqa: E402
from ponyc_amd.dist import GlooTransport, GlobalView   # noqa: E402
from ponyc_amd.engine import Engine      # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("shape", type=int, nargs=5,
                    help="logtable updaters streamers chunk iterate")
    ap.add_argument("--one-step", action="store_true",
                    help="run(1) until it returns 0 instead of one run(0)")
    a = ap.parse_args()
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    eng = Engine(device=0, n_ranks=world, rank=rank, transport=GlooTransport())
    w = W.gups(eng, *a.shape)
    if a.one_step:
        steps = 0
        while True:
            k = eng.run(1)
            if k == 0:
                break
            steps += k
    else:
        steps = eng.run(0)
    c = eng.counts()
    table = W.gups_result(GlobalView(eng), w)
    debug = [None] * world
    dist.all_gather_object(debug, eng.debug_info())
    eng.shutdown()
    if rank == 0:
        import pyoracle
        o = pyoracle.Oracle()
        wo = W.gups(o, *a.shape)
        so = o.run(0)
        co = o.counts()
        want = W.gups_result(o, wo)
        o.shutdown()
        out = {
            "shape": a.shape, "world": world, "updates": w["updates"],
            "table_equal": bool(np.array_equal(table, want)),
            "steps": [int(steps), int(so)],
            "delivered": [c["delivered"], co["delivered"]],
            "sent": [c["sent"], co["sent"]],
            "pending": [c["pending"], co["pending"]],
            "by_type": c["delivered_by_type"] == co["delivered_by_type"],
            "dropped": c["dropped"], "remote": c["remote"],
            "debug": debug,
        }
        print("MRG_RESULT " + json.dumps(out), flush=True)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
