"""One rank of a multi-rank parity run under a block-cyclic placement
(launched by tests/test_gpu_place.py like tests/mr_worker.py: every rank
drives device 0 through the host transport). The cases (and three larger
ones, below) and the driver are mr_worker's; `--bits b` goes to
Engine(block_bits=b). Rank 0 runs the CPU oracle, which knows no ranks, and
prints one `MR_RESULT {json}` line that also carries block_bits from
debug_info(), every rank's `remote` (a rank counts the cross-rank records it
received) and every rank's local_count per type.

`--refused`: the case's world is built under `--bits`, which must leave a rank
without an actor; run and run_fixed must fail with EINVAL on every rank, and
the engine must shut down clean. Prints one `MR_REFUSED {json}` line.

`--mismatch a,b,...`: rank r asks for the r-th value; init must fail with
EINVAL on every rank and leave no buffer behind, and an init with equal values
must work afterwards. Prints one `MR_MISMATCH {json}` line."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np                       # noqa: E402
import torch.distributed as dist         # noqa: E402

from mr_worker import CASES as MR_CASES, drive       # noqa: E402
from ponyc_amd import workloads as W     # noqa: E402
from ponyc_amd.dist import GlooTransport, GlobalView   # noqa: E402
from ponyc_amd.engine import Engine, GpuActorError, live_buffers   # noqa: E402


# mr_worker's cases, and three of them grown past 4096 ids, so that 4096-id
# blocks still give every rank actors (a rank without any is refused):
# storm and the muting FIFO world over three blocks (rank 0 owns two whole
# zones' worth, rank 1 one), the spreader's 8191-node tree over two
CASES = dict(MR_CASES)
CASES.update({
    "storm_9k": (lambda e: W.storm(e, 9000, 4, 12), lambda e, w: e.state_read(w["type"]), {}),
    "mute_9k": (lambda e: W.fifo(e, 9000, 3, 3, 2, batch=10, mailbox_cap=16), W.fifo_result, {}),
    "spreader_13": (lambda e: W.spreader(e, 13), W.spreader_result, {}),
})


def gathered(x):
    parts = [None] * dist.get_world_size()
    dist.all_gather_object(parts, x)
    return parts


def mismatch(bits):
    rank, world = dist.get_rank(), dist.get_world_size()
    code = 0
    try:
        Engine(device=0, n_ranks=world, rank=rank, transport=GlooTransport(), block_bits=bits[rank])
    except GpuActorError as e:
        code = e.code
    live = live_buffers()
    # the same value everywhere: a session, with that placement
    with Engine(device=0, n_ranks=world, rank=rank, transport=GlooTransport(),
                block_bits=bits[0]) as eng:
        again = eng.debug_info()["block_bits"]
    out = gathered({"code": code, "live": list(live), "again": again})
    if rank == 0:
        print("MR_MISMATCH " + json.dumps(out), flush=True)


def refused(case, bits):
    rank, world = dist.get_rank(), dist.get_world_size()
    setup, _result, kw, *_mode = CASES[case]
    codes = []
    eng = Engine(device=0, n_ranks=world, rank=rank, transport=GlooTransport(), block_bits=bits, **kw)
    setup(eng)
    local = sum(eng.local_count(t) for t in eng.first)
    for call in (lambda: eng.run(0), lambda: eng.run_fixed(1)):
        try:
            call()
            codes.append(0)
        except GpuActorError as e:
            codes.append(e.code)
    eng.shutdown()
    out = gathered({"codes": codes, "local": local, "live": list(live_buffers())})
    if rank == 0:
        print("MR_REFUSED " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("case")
    ap.add_argument("--bits", type=int, default=0)
    ap.add_argument("--mismatch", default="")
    ap.add_argument("--refused", action="store_true")
    a = ap.parse_args()
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    if a.mismatch:
        mismatch([int(v) for v in a.mismatch.split(",")])
        dist.barrier()
        dist.destroy_process_group()
        return
    if a.refused:
        refused(a.case, a.bits)
        dist.barrier()
        dist.destroy_process_group()
        return
    setup, result, kw, *mode = CASES[a.case]
    mode = mode[0] if mode else "run"
    eng = Engine(device=0, n_ranks=world, rank=rank, transport=GlooTransport(), block_bits=a.bits,
                 **kw)
    w = setup(eng)
    steps = drive(eng, mode)
    c = eng.counts()
    info = eng.debug_info()
    res = result(GlobalView(eng), w)
    local = gathered({str(t): eng.local_count(t) for t in sorted(eng.first)})
    ranges = {str(t): [eng.first[t], eng.count[t]] for t in sorted(eng.first)}
    remote = gathered(c["remote"])
    eng.shutdown()
    if rank == 0:
        import pyoracle
        o = pyoracle.Oracle()
        wo = setup(o)
        so = o.run(0)
        co = o.counts()
        ro = result(o, wo)
        o.shutdown()
        out = {
            "case": a.case, "world": world,
            "state_equal": bool(np.array_equal(res, ro)),
            "steps": [int(steps), int(so)],
            "delivered": [c["delivered"], co["delivered"]],
            "sent": [c["sent"], co["sent"]],
            "pending": [c["pending"], co["pending"]],
            "by_type": c["delivered_by_type"] == co["delivered_by_type"],
            "dropped": c["dropped"], "remote": remote, "peer_write": info["peer_write"],
            "block_bits": info["block_bits"], "zone_bits": info["zone_bits"],
            "local_count": local, "ranges": ranges,
        }
        print("MR_RESULT " + json.dumps(out), flush=True)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
