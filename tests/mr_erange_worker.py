"""One rank of tests/test_gpu_limits.py's two-rank over-limit case (launched
through torch.distributed.run like tests/mr_worker.py, every rank on the one
GPU over the host transport): FIFO sources that send 16,383 PUSHes in one
behaviour, one more than kXSeqMax = 16,382 (engine_dev.h).

  both: W.fifo(e, 2, 1, 1, 16383) — source ids 1 and 2, one on each rank
  one:  W.fifo(e, 1, 1, 1, 16383) — the only source, id 1, on rank 1

Every rank catches GpuActorError from run(), shuts its engine down and goes
on; rank 0 prints one `MR_RESULT {json}` line with every rank's code per case
(0: run returned normally) and its live device buffers after the shutdowns.
All ranks then meet in dist.barrier() and exit 0: a rank left waiting in one
of the run's collectives would fail the launch by its timeout instead."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch.distributed as dist         # noqa: E402

from ponyc_amd import workloads as W     # noqa: E402
from ponyc_amd.dist import GlooTransport   # noqa: E402
from ponyc_amd.engine import Engine, GpuActorError, live_buffers   # noqa: E402

OVER = 16383
CASES = {"both": 2, "one": 1}


def attempt(rank: int, world: int, sources: int) -> int:
    eng = Engine(device=0, n_ranks=world, rank=rank, transport=GlooTransport())
    try:
        W.fifo(eng, sources, 1, 1, OVER, mailbox_cap=2048)
        try:
            eng.run(0)
            return 0
        except GpuActorError as err:
            return err.code
    finally:
        eng.shutdown()


def main():
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    mine = {name: attempt(rank, world, sources) for name, sources in CASES.items()}
    mine["live"] = list(live_buffers())
    got = [None] * world
    dist.all_gather_object(got, mine)
    if rank == 0:
        out = {name: [g[name] for g in got] for name in [*CASES, "live"]}
        print("MR_RESULT " + json.dumps(out), flush=True)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
