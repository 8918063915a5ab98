"""Block-cyclic placement without a GPU (include/gpu_actor_place.h): the
library's pure functions gpu_actor_place_map / _global / _below against a
brute-force enumeration (each rank's owned ids in increasing order get slots
0, 1, 2, ...), for R in {1, 2, 3, 8} and b in {0, 1, 4, 11, 16}; b = 0 is
(id % R, id // R); Engine.owner_of / slot_of / below agree with the library
at type boundaries that are not block-aligned; the header, the Python export
list and pony/gpu_actor/placement.pony name the same entry points."""
import ctypes
import os
import re

import numpy as np
import pytest

from ponyc_amd import engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gpu_actor_place.h")
PONY = os.path.join(ROOT, "pony", "gpu_actor", "placement.pony")
EINVAL, ESTATE = -1, -6
RANKS = [1, 2, 3, 8]
BITS = [0, 1, 4, 11, 16]
MAX_IDS = 300_000


def n_ids(R, b):
    return min(3 * R * (1 << b) + 5, MAX_IDS)


def lib_map(lib, R, b, n):
    """(owner, slot) of ids 0 .. n - 1 from the library, one call per id"""
    owner = np.zeros(n, dtype=np.uint32)
    slot = np.zeros(n, dtype=np.uint64)
    r, s = ctypes.c_uint32(0), ctypes.c_uint64(0)
    fn = lib.gpu_actor_place_map
    for i in range(n):
        assert fn(R, b, i, ctypes.byref(r), ctypes.byref(s)) == 0
        owner[i], slot[i] = r.value, s.value
    return owner, slot


_MAPS = {}


def mapped(R, b):
    """the library's map of one (R, b), computed once for the tests that share it"""
    if (R, b) not in _MAPS:
        _MAPS[(R, b)] = lib_map(engine.load_library(), R, b, n_ids(R, b))
    return _MAPS[(R, b)]


@pytest.mark.parametrize("b", BITS)
@pytest.mark.parametrize("R", RANKS)
def test_map_is_brute_force_enumeration(R, b):
    owner, slot = mapped(R, b)
    ids = np.arange(owner.size, dtype=np.uint64)
    # blocks of 2^b consecutive ids, dealt round-robin
    assert np.array_equal(owner, (ids // np.uint64(1 << b)) % np.uint64(R))
    for r in range(R):
        mine = ids[owner == r]                      # increasing
        assert np.array_equal(slot[mine.astype(np.int64)], np.arange(mine.size, dtype=np.uint64)), (R, b, r)


@pytest.mark.parametrize("b", BITS)
@pytest.mark.parametrize("R", RANKS)
def test_global_inverts_map(R, b):
    lib = engine.load_library()
    owner, slot = mapped(R, b)
    g = ctypes.c_uint64(0)
    # every id near the block and round boundaries, and a stride through the rest
    B = 1 << b
    picks = set(range(0, owner.size, 97)) | {owner.size - 1}
    for k in range(0, owner.size, B):
        picks |= {k, k + 1, k + B - 1}
    for i in sorted(p for p in picks if p < owner.size):
        assert lib.gpu_actor_place_global(R, b, int(owner[i]), int(slot[i]), ctypes.byref(g)) == 0
        assert g.value == i, (R, b, i)


@pytest.mark.parametrize("R", RANKS)
def test_zero_bits_is_modulo(R):
    owner, slot = mapped(R, 0)
    ids = np.arange(owner.size, dtype=np.uint64)
    assert np.array_equal(owner, ids % np.uint64(R))
    assert np.array_equal(slot, ids // np.uint64(R))


class _Placed:
    """Engine's placement methods without an engine (they read these three fields)."""
    owner_of = engine.Engine.owner_of
    slot_of = engine.Engine.slot_of
    below = engine.Engine.below

    def __init__(self, n_ranks, rank, block_bits):
        self.n_ranks, self.rank, self.block_bits = n_ranks, rank, block_bits


@pytest.mark.parametrize("b", BITS)
@pytest.mark.parametrize("R", RANKS)
def test_engine_methods_and_below_agree(R, b):
    lib = engine.load_library()
    owner, slot = mapped(R, b)
    n = owner.size
    ids = np.arange(n, dtype=np.uint64)
    e0 = _Placed(R, 0, b)
    assert np.array_equal(e0.owner_of(ids), owner)
    assert np.array_equal(e0.slot_of(ids), slot)
    assert int(e0.owner_of(n - 1)) == owner[n - 1] and int(e0.slot_of(n - 1)) == slot[n - 1]
    # type boundaries off the block grid: below(r, x) = ids < x that r owns
    B = 1 << b
    firsts = sorted({0, 1, 3, B - 1, B + 1, B * R + 1, 2 * B * R - 3, 2 * B * R + B // 2 + 1, n - 2, n} &
                    set(range(n + 1)))
    cum = [np.concatenate([[0], np.cumsum(owner == r)]) for r in range(R)]
    v = ctypes.c_uint64(0)
    for x in firsts:
        for r in range(R):
            assert lib.gpu_actor_place_below(R, b, r, x, ctypes.byref(v)) == 0
            assert v.value == cum[r][x], (R, b, r, x)
            assert _Placed(R, r, b).below(x) == cum[r][x], (R, b, r, x)
    # a type [first, first + count) is one run of slots on every rank, from below(r, first)
    for first in firsts:
        if first >= n:
            continue
        for r in range(R):
            mine = slot[first:][owner[first:] == r]
            assert np.array_equal(mine, cum[r][first] + np.arange(mine.size, dtype=np.uint64))


def test_place_blocks_limits():
    lib = engine.load_library()
    assert engine.PLACE_MAX_BITS == 16
    assert lib.gpu_actor_place_blocks(17) == EINVAL
    assert lib.gpu_actor_place_blocks(0xFFFFFFFF) == EINVAL
    r, s, g = ctypes.c_uint32(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
    assert lib.gpu_actor_place_map(2, 17, 0, ctypes.byref(r), ctypes.byref(s)) == EINVAL
    assert lib.gpu_actor_place_map(0, 0, 0, ctypes.byref(r), ctypes.byref(s)) == EINVAL
    assert lib.gpu_actor_place_global(2, 0, 2, 0, ctypes.byref(g)) == EINVAL
    # no session is live: accepted (and put back to the default)
    assert lib.gpu_actor_place_blocks(16) == 0
    assert lib.gpu_actor_place_blocks(0) == 0


def header_names():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"GPU_ACTOR_API\s+[\w\s\*]+?\b(gpu_actor_\w+)\s*\(", src)))


def test_exports_match_header_and_pony():
    names = header_names()
    assert sorted(engine.PLACE_EXPORTS) == names
    assert not set(engine.PLACE_EXPORTS) & (set(engine.EXPORTS) | set(engine.HOST_EXPORTS))
    lib = engine.load_library()
    for name in names:
        assert hasattr(lib, name), name
    pony = open(PONY).read()
    assert sorted(set(re.findall(r"use @(gpu_actor_\w+)\[", pony))) == names
    m = re.search(r"#define\s+GPU_ACTOR_PLACE_MAX_BITS\s+(\d+)", open(HEADER).read())
    assert m and int(m.group(1)) == engine.PLACE_MAX_BITS
