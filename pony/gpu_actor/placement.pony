"""
Which rank an actor lives on (include/gpu_actor_place.h): block-cyclic
placement of the global id space over the ranks of a multi-rank engine.
Blocks of 2^block_bits consecutive ids share a rank, so a ring's `id + 1`
neighbour is on the sender's own rank on all but one hop in 2^block_bits —
the locality a CPU actor has by staying with its scheduler thread
(scheduler.c:752-948). block_bits 0, the default, is id % n_ranks.

Declared with exact prototypes like gpu_actor.pony's entry points (gencall.c:
1196-1198); every call returns an I32 error code, never a Pony error.
"""
use @gpu_actor_place_blocks[I32](block_bits: U32)
use @gpu_actor_place_map[I32](n_ranks: U32, block_bits: U32, id: U64,
  rank: Pointer[U32], slot: Pointer[U64])
use @gpu_actor_place_global[I32](n_ranks: U32, block_bits: U32, rank: U32,
  slot: U64, id: Pointer[U64])
use @gpu_actor_place_below[I32](n_ranks: U32, block_bits: U32, rank: U32,
  id: U64, n: Pointer[U64])

class val GpuPlacement
  """
  One placement: `GpuPlacement(n_ranks, block_bits).use()` before
  gpu_actor_init on every rank (all ranks must choose alike), then `owner`,
  `slot` and `global` answer where ids live — pure functions, usable before
  init and without a GPU.
  """
  let n_ranks: U32
  let block_bits: U32

  new val create(n_ranks': U32, block_bits': U32 = 0) =>
    n_ranks = n_ranks'.max(1)
    block_bits = block_bits'

  fun use(): I32 =>
    """EINVAL above 16 bits, ESTATE while a session is live."""
    @gpu_actor_place_blocks(block_bits)

  fun owner(id: U64): U32 =>
    var r: U32 = 0
    var s: U64 = 0
    @gpu_actor_place_map(n_ranks, block_bits, id, addressof r, addressof s)
    r

  fun slot(id: U64): U64 =>
    var r: U32 = 0
    var s: U64 = 0
    @gpu_actor_place_map(n_ranks, block_bits, id, addressof r, addressof s)
    s

  fun global(rank: U32, slot': U64): U64 =>
    var id: U64 = 0
    @gpu_actor_place_global(n_ranks, block_bits, rank, slot', addressof id)
    id

  fun below(rank: U32, id: U64): U64 =>
    """Ids below `id` that `rank` owns: where a type created at `id` starts there."""
    var n: U64 = 0
    @gpu_actor_place_below(n_ranks, block_bits, rank, id, addressof n)
    n
