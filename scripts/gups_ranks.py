"""A gups shape run to quiescence on several ranks (scripts/bench_configs.py
is the one-rank form). Started under torch.distributed.run, as
tests/mr_worker.py is; every rank drives device 0 through the host transport
(ponyc_amd.dist.GlooTransport: staged through host memory, not a fast path),
so the figure compares paths on one box and predicts nothing for xGMI.

    python -m torch.distributed.run --nnodes=1 --nproc-per-node=2 \\
        scripts/gups_ranks.py 24 8 64 1024 100 [--peer-write]

The shape is W.gups(e, logtable, updaters, streamers, chunk, iterate).
PONYC_AMD_GUPS_DEFER=0 runs the record-per-update path. Rank 0 prints one JSON
line: updates, steps, wall seconds of the run (the slowest rank's), updates/s,
and over the ranks the summed gups_updates and gups_chunks_in and rank 0's
`remote`. The debug keys are read with .get: a build without them reports 0."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch.distributed as dist         # noqa: E402

from ponyc_amd import workloads as W     # noqa: E402
from ponyc_amd.dist import GlooTransport, allmax   # noqa: E402
from ponyc_amd.engine import Engine      # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("shape", type=int, nargs=5,
                    help="logtable updaters streamers chunk iterate")
    ap.add_argument("--peer-write", action="store_true",
                    help="cross-rank records stored straight into the peers' inboxes")
    a = ap.parse_args()
    if a.peer_write:
        os.environ["PONYC_AMD_PEER_WRITE"] = "1"
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    eng = Engine(device=0, n_ranks=world, rank=rank, transport=GlooTransport())
    w = W.gups(eng, *a.shape)
    eng.sync()
    dist.barrier()
    t0 = time.perf_counter()
    steps = eng.run(0)
    eng.sync()
    secs = allmax(time.perf_counter() - t0)
    c = eng.counts()
    debug = [None] * world
    dist.all_gather_object(debug, eng.debug_info())
    eng.shutdown()
    if rank == 0:
        line = {"shape": a.shape, "ranks": world, "updates": w["updates"], "steps": int(steps),
                "seconds": round(secs, 4), "updates_per_s": round(w["updates"] / secs, 1),
                "gups_updates": sum(d.get("gups_updates", 0) for d in debug),
                "gups_chunks_in": sum(d.get("gups_chunks_in", 0) for d in debug),
                "remote": c["remote"], "dropped": c["dropped"],
                "peer_write": debug[0].get("peer_write", 0),
                "defer": os.environ.get("PONYC_AMD_GUPS_DEFER", "1")}
        print(json.dumps(line), flush=True)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
