/*
 * gpu_actor_place.h — which rank an actor lives on (libgpuactor.so).
 *
 * A multi-rank engine (gpu_actor_config_t::n_ranks = R > 1) deals the global
 * id space over its ranks block-cyclically: blocks of B = 2^b consecutive ids
 * live together on one rank, block q on rank q % R. With q = id >> b and
 * o = id & (B - 1):
 *
 *     owner(id)       = q % R
 *     slot(id)        = ((q / R) << b) | o
 *     global(r, slot) = ((((slot >> b) * R) + r) << b) | (slot & (B - 1))
 *     below(r, x)     = ids < x owned by r
 *                     = B * (f > r ? (f - r + R - 1) / R : 0)
 *                       + (f % R == r ? x & (B - 1) : 0),        f = x >> b
 *
 * slot is dense and increasing in id on every rank, so a type's id range is
 * one contiguous run of local slots everywhere, gpu_actor_state_read/_write
 * keep their meaning (the owned actors in id order), and spawned ids keep
 * landing at their owner's next slot. b = 0, the default, is id % R and
 * id / R. A send to id + 1 crosses ranks on one hop in 2^b instead of on
 * every hop (an actor's scheduler affinity in the reference runtime,
 * scheduler.c:752-948); uniformly random targets cross on (R - 1) / R of the
 * sends whatever b is. Results do not depend on b: it moves actors, not
 * messages' order.
 *
 * Conventions are those of gpu_actor.h: 0 ok, < 0 a GPU_ACTOR_E* code.
 */
#ifndef GPU_ACTOR_PLACE_H
#define GPU_ACTOR_PLACE_H

#include "gpu_actor.h"

#if defined(__cplusplus)
extern "C" {
#endif

#define GPU_ACTOR_PLACE_MAX_BITS 16

/* The placement of the next gpu_actor_init and every later one until changed:
 * blocks of 1 << block_bits ids. GPU_ACTOR_EINVAL above
 * GPU_ACTOR_PLACE_MAX_BITS, GPU_ACTOR_ESTATE while a session is live. When
 * never called, the environment variable PONYC_AMD_BLOCK_BITS gives the
 * default (a test hook), else 0. Every rank must pass the same value: init
 * checks it across the ranks and fails on all of them with GPU_ACTOR_EINVAL
 * otherwise. With one rank the value is accepted and changes nothing.
 * Every rank must own at least one actor: with fewer blocks of ids than
 * ranks (under the default too: fewer actors than ranks), gpu_actor_run,
 * _run_async and _run_fixed return GPU_ACTOR_EINVAL on every rank before any
 * collective (a rank without actors would take no part in a step's
 * exchange). */
GPU_ACTOR_API int gpu_actor_place_blocks(uint32_t block_bits);

/* owner(id) and slot(id) above; pure, usable before init and without a GPU.
 * Either output may be NULL. GPU_ACTOR_EINVAL for n_ranks == 0 or block_bits
 * above the limit. */
GPU_ACTOR_API int gpu_actor_place_map(uint32_t n_ranks, uint32_t block_bits, uint64_t id,
  uint32_t* rank, uint64_t* slot);

/* global(rank, slot) above: the inverse of gpu_actor_place_map. */
GPU_ACTOR_API int gpu_actor_place_global(uint32_t n_ranks, uint32_t block_bits, uint32_t rank,
  uint64_t slot, uint64_t* id);

/* below(rank, id) above: a type created at id `first` starts at local slot
 * below(rank, first) of every rank. */
GPU_ACTOR_API int gpu_actor_place_below(uint32_t n_ranks, uint32_t block_bits, uint32_t rank,
  uint64_t id, uint64_t* n);

#if defined(__cplusplus)
}
#endif

#endif /* GPU_ACTOR_PLACE_H */
