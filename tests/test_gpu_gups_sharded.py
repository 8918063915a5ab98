"""The fused GUPS update path at n_ranks > 1: streamers list
one 8-byte PolyRand state per chunk, every rank gathers every rank's list once
per step, and k_gups_apply_ranks applies of each chunk the updates whose
updater the rank owns.  2 or 3 ranks share the test box's GPU through the host
transport (tests/mr_gups_worker.py); the table and every count are checked
bit-exact against the single-rank CPU oracle, and debug_info's gups_* keys pin
which path ran on which rank.

Shapes are W.gups(e, logtable, updaters, streamers, chunk, iterate); streamer 0
is seeded PolyRand(0), the stream that stays on word 0 of updater 0."""
import json
import os
import socket
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))

EVEN = (14, 8, 64, 64, 3)
RAGGED = (12, 8, 5, 100, 2)


def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _run(nproc, shape, *flags, env=None):
    """one torch.distributed.run launch; the worker's result line, parsed"""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
           f"--nproc-per-node={nproc}", "--master-addr=127.0.0.1", f"--master-port={_port()}",
           os.path.join(HERE, "mr_gups_worker.py"), *[str(x) for x in shape], *flags]
    e = dict(os.environ, OMP_NUM_THREADS="1")
    for k in ("PONYC_AMD_GUPS_DEFER", "PONYC_AMD_GUPS_SEG", "PONYC_AMD_PEER_WRITE"):
        e.pop(k, None)
    e.update(env or {})
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=180, env=e)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    line = [l for l in p.stdout.splitlines() if l.startswith("MRG_RESULT ")]
    assert line, p.stdout[-2000:]
    r = json.loads(line[-1][len("MRG_RESULT "):])
    print(json.dumps(r))
    return r


def _exact(r, nproc):
    """the table and every summed count equal the oracle's; nothing dropped"""
    assert r["world"] == nproc and len(r["debug"]) == nproc
    assert r["dropped"] == 0
    assert r["table_equal"]
    assert r["steps"][0] == r["steps"][1]
    assert r["delivered"][0] == r["delivered"][1]
    assert r["sent"][0] == r["sent"][1]
    assert r["pending"][0] == r["pending"][1] == 0
    assert r["by_type"]


def _sum(r, key):
    return sum(d[key] for d in r["debug"])


def _fused_all(r):
    """every update went through the descriptor path: each applied once, by its
    owner; every descriptor listed reached every other rank"""
    n = r["world"]
    assert _sum(r, "gups_updates") == r["updates"]
    assert _sum(r, "gups_chunks_in") == (n - 1) * _sum(r, "gups_chunks_out")
    assert _sum(r, "gups_atomics") <= r["updates"]


@pytest.mark.gpu
def test_even_two_ranks():
    r = _run(2, EVEN)
    _exact(r, 2)
    assert r["updates"] == 64 * 64 * 4
    _fused_all(r)
    for d in r["debug"]:
        assert d["gups_updates"] > 0 and d["gups_chunks_in"] > 0
        assert d["peer_write"] == 0
    assert r["remote"] > 0
    assert r["remote"] == r["debug"][0]["gups_remote"]


@pytest.mark.gpu
def test_ragged_three_ranks():
    """updaters 3/3/2 and streamers 2/2/1 over the ranks; chunk 100: L = 16,
    7 lanes per chunk, the last lane with 4 updates"""
    r = _run(3, RAGGED)
    _exact(r, 3)
    _fused_all(r)
    assert _sum(r, "gups_chunks_out") == 5 * 3


@pytest.mark.gpu
def test_rank_without_streamer():
    """streamer ids 8 and 9 live on ranks 2 and 0: rank 1 lists nothing and
    still applies its share"""
    r = _run(3, (12, 8, 2, 64, 2))
    _exact(r, 3)
    _fused_all(r)
    assert r["debug"][1]["gups_chunks_out"] == 0
    assert r["debug"][1]["gups_updates"] > 0
    assert r["debug"][1]["gups_chunks_in"] == 2 * 3


@pytest.mark.gpu
def test_rank_without_updater():
    """two updaters on three ranks: rank 2 owns none, walks nothing, and still
    takes part in the gather"""
    r = _run(3, (10, 2, 6, 32, 2))
    _exact(r, 3)
    _fused_all(r)
    assert r["debug"][2]["gups_updates"] == 0
    assert r["debug"][2]["gups_chunks_out"] > 0


@pytest.mark.gpu
def test_list_full_mixes_both_paths():
    """two chunks per list segment: the other streamers apply their own chunks
    (local atomics, remote records) in the same steps, on both ranks"""
    r = _run(2, (12, 4, 1000, 64, 5), env={"PONYC_AMD_GUPS_SEG": "2"})
    _exact(r, 2)
    assert r["updates"] == 1000 * 64 * 6
    assert 0 < _sum(r, "gups_updates") < r["updates"]
    for d in r["debug"]:
        assert d["gups_chunks_out"] > 0
    assert r["remote"] > r["debug"][0]["gups_remote"] > 0


@pytest.mark.gpu
def test_off_matches_and_remote_equal():
    """PONYC_AMD_GUPS_DEFER=0 keeps the record-per-update path; `remote` (the
    updates applied on a rank other than their streamer's, rank 0's share)
    is the same number on either path"""
    on = _run(2, EVEN)
    off = _run(2, EVEN, env={"PONYC_AMD_GUPS_DEFER": "0"})
    _exact(on, 2)
    _exact(off, 2)
    assert _sum(off, "gups_updates") == 0
    assert _sum(off, "gups_chunks_in") == 0 and _sum(off, "gups_chunks_out") == 0
    assert _sum(off, "gups_remote") == 0
    assert off["remote"] > 0
    assert on["remote"] == off["remote"]


@pytest.mark.gpu
@pytest.mark.parametrize("nproc,shape", [(2, EVEN), (3, RAGGED)])
def test_peer_writes(nproc, shape):
    """the same with cross-rank records stored straight into the peers'
    inboxes: the descriptors still go through the collectives"""
    r = _run(nproc, shape, env={"PONYC_AMD_PEER_WRITE": "1"})
    _exact(r, nproc)
    _fused_all(r)
    for d in r["debug"]:
        assert d["peer_write"] == 1


@pytest.mark.gpu
def test_one_step_at_a_time():
    """run(1) until it returns 0: the last step's gather and apply are done
    before the table is read"""
    r = _run(2, EVEN, "--one-step")
    _exact(r, 2)
    _fused_all(r)
