// step_entry.h — the compiled instantiations of k_step (zone_dev.h), listed
// once: GPA_STEP_TABLES below. The declarations here, the host's table of
// entries and its lookup (engine.hip: step_rows, step_entry) and the check of
// every unit against the list (step_tu.h) are generated from it.
//
// Each instantiation lives in a translation unit of its own (step_<name>.hip),
// so the library builds them in parallel; each such unit is its own code
// object with its own copy of the engine constants (c_types, c_eng), which the
// host uploads to every entry of the table (engine.hip: upload_types).
//
// Two zone geometries are compiled: 2048-actor zones with 512-thread
// workgroups (namespace gpa, step_<name>.hip) and 4096-actor zones with
// 1024-thread workgroups (namespace gpa_z12, step_<name>_z12.hip: the same
// unit behind step_tu.h's GPA_STEP_Z12). The host picks one per engine
// (engine.hip: relayout_zones).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/gpu_actor.h"

// X(name, handler table): the unit step_<name>.hip exports step_entry_<name>(),
// whose kernel is k_step<handler table>. The table is a preprocessor integer
// (step_tu.h and engine_dev.h test it in #if): -1 is any mix of tables, 64 the
// FIFO sources + sinks pair (zone_dev.h kHtFifoPair).
#define GPA_STEP_TABLES(X)                       \
  X(any, -1)                                     \
  X(ring, GPU_ACTOR_HT_RING)                     \
  X(pinger, GPU_ACTOR_HT_PINGER)                 \
  X(pinger_det, GPU_ACTOR_HT_PINGER_DET)         \
  X(fanin_sender, GPU_ACTOR_HT_FANIN_SENDER)     \
  X(gups_streamer, GPU_ACTOR_HT_GUPS_STREAMER)   \
  X(storm, GPU_ACTOR_HT_STORM)                   \
  X(spreader, GPU_ACTOR_HT_SPREADER)             \
  X(fifo_pair, 64)                               \
  X(program, GPU_ACTOR_HT_PROGRAM)

typedef void (*step_kernel_t)(uint32_t, uint32_t, uint32_t);

// Geometry-neutral (outside the renamed namespace): the host holds entries of
// both geometries. upload() takes the host's TypeDev[GPU_ACTOR_MAX_TYPES] and
// EngDev, whose layout both geometries share.
struct StepEntry {
  step_kernel_t kernel;
  hipError_t (*upload)(const void* types, const void* eng, hipStream_t s);
  bool stub;               // not compiled in this (experiment) build
  uint32_t zone_bits;      // actors per zone = 1 << zone_bits
  uint32_t threads;        // workgroup size
  uint32_t sort_work;      // u32 of dynamic LDS the hot-group sort borrows
  uint32_t bucket_words;   // u32 of dynamic LDS per destination bucket (6: a table with dp zones)
  bool hot;                // takes zones prepared by k_hot (hot_dev.h): any-mix and FIFO pair
  // split tables: the step as two launches (zone_dev.h k_step PM 1, 2), or
  // as one that calls the second's code (PM 3); nullptr for the other tables
  step_kernel_t plan, rest, fused;
  // a two-pass table whose sends all carry one constant argument: its engines
  // keep a compact landing lane, and plan_arg is that argument (zone_dev.h
  // plan_const_arg), which k_land_expand puts back
  bool const_arg;
  uint64_t plan_arg;
};

// the handler table of each name, for step_tu.h's check of its unit
enum : int {
#define GPA_STEP_X(name, ht) kStepHt_##name = (ht),
  GPA_STEP_TABLES(GPA_STEP_X)
#undef GPA_STEP_X
};

#define GPA_STEP_X(name, ht) StepEntry step_entry_##name();
namespace gpa { GPA_STEP_TABLES(GPA_STEP_X) }
namespace gpa_z12 { GPA_STEP_TABLES(GPA_STEP_X) }
#undef GPA_STEP_X
