// engine.hip — the gpu_actor engine for gfx950: kernels (zone_dev.h) and the
// C-ABI declared in include/gpu_actor.h.
//
// One superstep = one k_step launch (one workgroup per 2048-actor zone; see
// zone_dev.h). With n_ranks > 1, the records a step produced for actors on
// other ranks are swapped with RCCL after it (counts all-to-all, then grouped
// ncclSend/ncclRecv over xGMI) and k_xinject lands them before the next step.
// The launch boundary is the BSP barrier; quiescence ("no pending mail on any
// rank") replaces the CNF/ACK protocol (scheduler.c:303-480).
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <rccl/rccl.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <atomic>
#include <condition_variable>
#include <map>
#include <mutex>
#include <new>
#include <thread>
#include <vector>

#include "../../include/gpu_actor_host.h"
#include "../../include/gpu_actor_place.h"
#include "engine_dev.h"
#include "zone_dev.h"
#include "sparse_dev.h"
#include "hot_dev.h"
#include "step_entry.h"
#include "jit_host.h"
#include "dev_buf.h"

using namespace gpa;

// gups Updater tables (gups_basic/main.pony:145-155: table[k] = k + index*size),
// one thread per word (field-major state[k * lcount + li]).
__global__ void __launch_bounds__(kBlock) k_construct_table(uint32_t t, uint32_t live)
{
  const TypeDev& T = c_types[t];
  const uint64_t n = T.lcount;
  const uint64_t size = T.params[0] < T.words ? T.params[0] : T.words;
  const uint64_t total = size * n;
  for(uint64_t x = (uint64_t)blockIdx.x * kBlock + threadIdx.x; x < total;
      x += (uint64_t)gridDim.x * kBlock)
  {
    const uint64_t k = x / n, li = x - k * n;
    const uint64_t L = T.lfirst + li;
    const uint64_t i = global_of((uint32_t)L) - T.first;
    if(i >= live) continue;
    T.state[x] = k + i * size;
  }
}

// pony_create's constructor run: initial state of a freshly created type;
// the first `live` ids of the type (the rest are reserved for actors its
// behaviours create, and stay zeroed until then).
__global__ void __launch_bounds__(kBlock) k_construct(uint32_t t, uint32_t live)
{
  const TypeDev& T = c_types[t];
  const uint32_t li = blockIdx.x * kBlock + threadIdx.x;
  if(li >= T.lcount) return;
  const uint32_t L = T.lfirst + li;
  const uint64_t i = global_of(L) - T.first;   // index in type
  if(i >= live) return;
  const size_t n = T.lcount;
  uint64_t* st = T.state;
  switch(T.ht)
  {
    case GPU_ACTOR_HT_RING: {
      const uint64_t size = T.params[0] ? T.params[0] : 1;
      const uint64_t ring = i / size, p = i % size;
      st[li] = (p == 0) ? GPU_ACTOR_NONE : T.first + ring * size + (p + 1) % size;
      st[n + li] = p + 1;
      break;
    }
    case GPU_ACTOR_HT_PINGER: {
      uint64_t x, y;
      xoro_create(x, y, T.params[3] + i + 1, 0x9E3779B97F4A7C15ull);
      (void)rand_int(x, y, 100); (void)rand_int(x, y, 100); (void)rand_int(x, y, 100);
      st[li] = x; st[n + li] = y;
      break;
    }
    case GPU_ACTOR_HT_FANIN_SENDER: {
      uint64_t x, y;
      xoro_create(x, y, T.params[3] ? 5489 + i : 5489, 0);
      st[li] = x; st[n + li] = y; st[2 * n + li] = T.params[2];
      break;
    }
    case GPU_ACTOR_HT_GUPS_STREAMER:
      st[li] = polyrand_seeded(T.params[5] * i);
      break;
    case GPU_ACTOR_HT_GUPS_UPDATER:      // the table: k_construct_table
      break;
    case GPU_ACTOR_HT_FIFO_SRC: {
      const uint64_t ns = T.params[1] ? T.params[1] : 1;
      st[li] = T.params[0] + i % ns;
      st[2 * n + li] = T.params[2];
      break;
    }
    case GPU_ACTOR_HT_FIFO_SINK:
      st[li] = 0xcbf29ce484222325ull;
      break;
    default:
      break;
  }
}

// Copy each zone's old buffer into its slot of a new layout (one block per zone).
__global__ void __launch_bounds__(kBlock) k_zone_copy(const ZRec* src, const uint64_t* src_off,
  const uint32_t* src_cap, ZRec* dst, const uint64_t* dst_off)
{
  const uint32_t z = blockIdx.x;
  const ZRec* s = src + src_off[z];
  ZRec* d = dst + dst_off[z];
  for(uint32_t i = threadIdx.x; i < src_cap[z]; i += kBlock) d[i] = s[i];
}

// ---- actors spawned by behaviours (gpu_actor_type_reserve) -------------------
// After a step: the spawn records, sorted by key (type, creator, seq), get ids
// first + live[type] + (rank within the type); each new actor's constructor
// message lands like any other arrival for the next step.
__global__ void __launch_bounds__(kBlock) k_spawn_scan(const uint64_t* key, uint32_t n,
  uint32_t* tstart, uint32_t* tcnt)
{
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if(i >= n) return;
  const uint32_t t = (uint32_t)(key[i] >> 52);
  atomicMin(&tstart[t], i);
  atomicAdd(&tcnt[t], 1u);
}

__global__ void __launch_bounds__(kLandThreads) k_spawn_land(const uint64_t* key, const uint64_t* arg,
  uint32_t n, const uint32_t* tstart, const unsigned long long* live, uint32_t cur)
{
  __shared__ uint32_t s_hist[kMaxZones];
  __shared__ uint32_t s_base[kMaxZones];
  LandRec r[kLandPer];
#pragma unroll
  for(int u = 0; u < kLandPer; ++u)
  {
    const uint64_t i = (uint64_t)blockIdx.x * kLandRecs + (uint64_t)u * kLandThreads + threadIdx.x;
    r[u].valid = false;
    if(i < n)
    {
      const uint64_t k = key[i];
      const uint32_t t = (uint32_t)(k >> 52);
      const TypeDev& T = c_types[t];
      const uint64_t slot = live[t] + (i - tstart[t]);
      if(slot < T.count)
      {
        // every rank numbers the same gathered list; it lands its own actors
        r[u].valid = !is_remote(T.first + (uint32_t)slot);
        r[u].to = T.first + (uint32_t)slot;
        r[u].w = (uint32_t)(((k >> 4) & 0xFFFFull) << 16) | (uint32_t)((k & 0xFu) << 12);
        r[u].from = (uint32_t)(k >> 20);
        r[u].arg = arg[i];
      }
      else if(c_eng.rank == 0)
        atomicAdd(&c_eng.stats[ST_DROPPED], 1ull);     // reserve exhausted
    }
  }
  land_records(r, cur, s_hist, s_base);
}

__global__ void k_spawn_commit(const uint32_t* tcnt, unsigned long long* live)
{
  const uint32_t t = threadIdx.x;
  if(t >= GPU_ACTOR_MAX_TYPES || tcnt[t] == 0) return;
  const unsigned long long room = c_types[t].count - live[t];
  live[t] += tcnt[t] < room ? tcnt[t] : room;
}

// ---- messages to the host (include/gpu_actor_host.h; engine_dev.h send_host) --
// Before every step of an engine with port types: the step's index since the
// last collection, shifted above the key's sender bits (EngDev::host_step).
__global__ void k_host_begin(uint64_t* step_word, uint64_t v)
{
  *step_word = v;
}

// The listed messages of the kHostShards segments as one run: off[s] is where
// segment s's records start in it (the host read the segments' counts); the
// run's keys, and for each its place in the list, go to the sort.
struct HostOff { uint32_t off[kHostShards + 1]; };
__global__ void __launch_bounds__(kBlock) k_host_compact(const uint64_t* key, HostOff o, uint32_t seg,
  uint64_t* key_out, uint32_t* idx_out)
{
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if(i >= o.off[kHostShards]) return;
  uint32_t lo = 0, hi = kHostShards - 1;         // last segment with off <= i
  while(lo < hi)
  {
    const uint32_t mid = (lo + hi + 1) / 2;
    if(o.off[mid] <= i) lo = mid; else hi = mid - 1;
  }
  const uint32_t at = lo * seg + (i - o.off[lo]);  // < kHostShards * seg: i - off[lo] < the segment's count <= seg
  key_out[i] = key[at];
  idx_out[i] = at;
}

// The first n records in key order as gpu_host_msg_t (32 B: two 16-byte
// stores a lane, consecutive lanes consecutive records): key = step since
// `base` << kshift | from << 16 | seq, idx the record's place in the list.
__global__ void __launch_bounds__(kBlock) k_host_gather(const uint64_t* key, const uint32_t* idx,
  const uint4* rec, gpu_host_msg_t* out, uint32_t n, uint64_t base, uint32_t kshift)
{
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if(i >= n) return;
  const uint64_t k = key[i];
  const uint4 r = rec[idx[i]];
  const uint64_t step = base + (k >> kshift);
  const uint32_t from = (uint32_t)((k & ((1ull << kshift) - 1ull)) >> 16);
  uint4* o = reinterpret_cast<uint4*>(out + i);
  o[0] = make_uint4((uint32_t)step, (uint32_t)(step >> 32), from, (uint32_t)(k & 0xFFFFull));
  o[1] = r;                                        // to, behaviour, arg
}
static_assert(sizeof(gpu_host_msg_t) == 32, "gpu_host_msg_t is 32 B");

// messages a collection held more of than the reserve (gpu_actor_host_reserve)
__global__ void k_host_lost(unsigned long long n)
{
  c_eng.stats[ST_DROPPED] += n;
}

// an empty compact lane's counters: low word 0, high word land_n (EngDev::landc_n)
__global__ void __launch_bounds__(kBlock) k_land8_mirror(const uint32_t* land_n,
  unsigned long long* landc_n, uint32_t n)
{
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if(i < n) landc_n[i] = (unsigned long long)land_n[i] << 32;
}

// ---- records past a zone's capacity (SpillRec, engine_dev.h) ----------------
// need[z] = largest position + 1 spilled into zone z (either buffer)
__global__ void __launch_bounds__(kBlock) k_spill_need(const SpillRec* s, uint32_t n, uint32_t* need)
{
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if(i >= n) return;
  atomicMax(&need[s[i].z], (s[i].tag & kSpillPosMask) + 1u);
}

// after the zones have grown: every spilled record to its own position
__global__ void __launch_bounds__(kBlock) k_spill_place(const SpillRec* s, uint32_t n, uint32_t p)
{
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if(i >= n) return;
  const SpillRec r = s[i];
  ZRec* base = (r.tag & kSpillCarry) ? c_eng.carry[p] : c_eng.land[p];
  base[c_eng.zoff[r.z] + (r.tag & kSpillPosMask)] = r.rec;
}

// The compact landing lane (EngDev::landc) of parity p back into 16-byte
// records, one workgroup per zone: every compact record of the zone goes
// behind its 16-byte ones in land[p] with the table's constant argument `arg`
// (past the zone's capacity: the spill list, like any landing record); holes
// (a chunk that did not fit the lane) are skipped. The zone's lane is then
// empty. Launched by the host ahead of everything that reads landing buffers
// but the step of the lane's own table (land8_flush).
__global__ void __launch_bounds__(kBlock) k_land_expand(uint32_t p, uint64_t arg)
{
  // The records keep the lane's order (holes closed up): each round of kBlock
  // places goes behind the rounds before it, a record at the number of
  // records before it in its round (ballot per wave, the waves' counts in LDS).
  constexpr uint32_t kWaves = kBlock / 64;
  __shared__ uint32_t s_wave[kWaves];
  const uint32_t z = blockIdx.x;
  const uint32_t nlc = min((uint32_t)c_eng.landc_n[p][z], c_eng.zcapz[z]);
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  uint32_t pos0 = c_eng.land_n[p][z];
  const uint2* const Lc = c_eng.landc[p] + c_eng.zoff[z];
  for(uint32_t i0 = 0; i0 < nlc; i0 += kBlock)          // uniform bounds: every thread takes every round
  {
    const uint32_t i = i0 + threadIdx.x;
    const uint2 r = i < nlc ? Lc[i] : make_uint2(kLand8Hole, 0u);
    const bool rec = r.x != kLand8Hole;
    const unsigned long long m = __ballot(rec);
    if(lane == 0) s_wave[wv] = (uint32_t)__popcll(m);
    __syncthreads();
    uint32_t before = 0, round = 0;
    for(uint32_t w = 0; w < kWaves; ++w)
    {
      const uint32_t c = s_wave[w];
      if(w < wv) before += c;
      round += c;
    }
    if(rec)
      land_store(p, z, pos0 + before + (uint32_t)__popcll(m & ((1ull << lane) - 1ull)),
        make_uint4(r.x, r.y, (uint32_t)arg, (uint32_t)(arg >> 32)));
    pos0 += round;
    __syncthreads();
  }
  if(threadIdx.x == 0)
  {
    c_eng.land_n[p][z] = pos0;
    c_eng.landc_n[p][z] = (unsigned long long)pos0 << 32;
    if(z == 0) atomicAnd(c_eng.lc_over, ~(1u << p));
  }
}

// Backlog copies listed by k_step (EngDev::bigc, defer_big): the listed
// records form one flat range (each copy's base, in slot order), cut into
// equal contiguous chunks, one per workgroup; a workgroup finds the first copy
// its chunk touches (binary search over the bases) and walks on from there,
// so one overloaded receiver's remainder moves at the whole GPU's bandwidth
// and no workgroup visits copies outside its chunk. With nothing listed the
// kernel returns at once. The list's counter is kept per step parity (cur):
// the next step's k_step clears this one (its zone 0, at its start), so no
// workgroup here signals another (the last-finisher count and fence took
// ~6 us a step: 512 adds on one word).
constexpr uint32_t kBigCopyCap = 4096;
constexpr uint32_t kBigCopyBlocks = 512;
__global__ void __launch_bounds__(kBlock) k_carry_big(uint32_t cur)
{
  // a step that did not run listed nothing (its counter may hold a list of
  // two steps before, already copied)
  const bool halt_now = c_eng.nranks == 1 ? step_halted(cur) : (*c_eng.spill_flag != 0u);
  if(halt_now) return;
  const unsigned long long v = c_eng.bigc_n[cur];  // final: k_step ran to completion before
  const uint32_t n = min((uint32_t)(v >> 32), c_eng.bigc_cap);
  if(n == 0) return;
  // the listed copies' records: the last one's base + its length (bigc_n's
  // low word also counts copies past bigc_cap, which their zones made)
  const uint32_t total = c_eng.bigc[n - 1].base + c_eng.bigc[n - 1].rem;
  const uint32_t per = (total + gridDim.x - 1) / gridDim.x;
  const uint32_t c0 = blockIdx.x * per, c1 = min(c0 + per, total);
  if(c0 < c1)
  {
    uint32_t lo = 0, hi = n - 1;                   // last copy with base <= c0
    while(lo < hi)
    {
      const uint32_t mid = (lo + hi + 1) / 2;
      if(c_eng.bigc[mid].base <= c0) lo = mid; else hi = mid - 1;
    }
    for(uint32_t d = lo; d < n; ++d)
    {
      const BigCopy b = c_eng.bigc[d];
      if(b.base >= c1) break;
      const uint32_t j0 = c0 > b.base ? c0 - b.base : 0u;       // b.base < c1 here
      const uint32_t j1 = min(c1 - b.base, b.rem);
      for(uint32_t j = j0 + threadIdx.x; j < j1; j += kBlock)
      {
        const uint32_t k = b.from + j;
        const uint32_t q = k - b.ncc;
        const uint4 r = k < b.ncc ? *reinterpret_cast<const uint4*>(b.c + k)
                      : *reinterpret_cast<const uint4*>(b.p + (b.perm ? (uint32_t)(b.perm[q] & 0xFFFFFull) : q));
        *reinterpret_cast<uint4*>(b.dst + j) = r;
      }
    }
  }
}

// ===========================================================================
// Host side
// ===========================================================================

namespace {

constexpr uint32_t kChunk = 16;          // steps between quiescence readbacks
constexpr uint32_t kPendSlots = 4096;    // pend[] entries
constexpr uint32_t kPendPre = kPendSlots - 1;

struct HostType {
  bool registered = false, created = false;
  uint32_t words = 0, ht = 0, batch = 0, cap = 0;
  uint64_t params[GPU_ACTOR_MAX_PARAMS] = {};
  uint64_t first = 0, count = 0;
  uint32_t lfirst = 0, lcount = 0;
  uint64_t reserve = 0;                 // ids for actors spawned by behaviours
  int32_t priority = 0;                 // the fork's _priority() hint
  DevBuf<uint64_t> d_state;
  DevBuf<uint64_t> d_prog;              // GPU_ACTOR_HT_PROGRAM: the behaviours' program
  uint32_t prog_n = 0;
  bool prog_yields = false;             // it holds a YIELD or a SPAWN: the small-step path leaves it
  std::vector<uint64_t> prog_host;      // the program's words (the run-time compiled step, jit_host.h)
};

// Records past zone capacity: the spill lists' counters (Session::d_sstat)
struct SpillStat {
  unsigned int spill_n[2];
  unsigned int halt;
  unsigned int lc_over;        // bit p: the compact lane of parity p needs the host (EngDev::lc_over)
  unsigned long long skipped;
};

// The hot-zone scratch words (hot_dev.h) of Session::d_hot, as word offsets in
// the order the device's arrays lie: upload_types hands them to the device,
// init fills the aux key ranges. bar is the grid barrier's [0] arrivals, [1]
// finished workgroups, [2] missed phases, [3] zones given back after a miss.
struct HotLayout {
  size_t prep = 0;
  size_t slot = prep + kMaxZones;
  size_t cnt = slot + kMaxZones;
  size_t aux = cnt + (size_t)kMaxHot * kHotActors;        // kMaxHot x 3 x kHotActors
  size_t hist = aux + (size_t)kMaxHot * 3 * kHotActors;
  size_t bcnt = hist + kHotBins;
  size_t cur = bcnt + kHotBins;                           // kHotBins + kHotActors
  size_t bar = cur + kHotBins + kHotActors;
  size_t words = bar + 64;
};
constexpr HotLayout kHotLayout{};

// What lives across gpu_actor_init / gpu_actor_shutdown: the locks, the
// progress threads of asynchronous runs, and the host transport (set before
// init, kept by shutdown).
struct Process {
  std::mutex mu;
  // asynchronous run (gpu_actor_run_async): one progress thread at a time;
  // wmu guards the thread object (joined or detached by whoever reaps it)
  std::mutex wmu;
  std::thread worker;
  // progress threads that chained a run from their own completion callback:
  // they cannot join themselves; gpu_actor_shutdown joins them
  std::vector<std::thread> detached;
  std::atomic<bool> async_busy{false};   // read without the lock
  std::atomic<bool> async_started{false};  // the progress thread holds mu
  int async_rc = 0;
  uint64_t async_steps = 0;
  // host transport (gpu_actor_set_transport)
  gpu_actor_alltoallv_fn xp_a2a = nullptr;
  gpu_actor_allreduce_fn xp_ar = nullptr;
  void* xp_ctx = nullptr;
  // placement of the sessions to come (gpu_actor_place_blocks; -1: never
  // called, PONYC_AMD_BLOCK_BITS or 0)
  int place_bits = -1;
};

// What a superstep launches, decided once per configuration (types, programs,
// geometry, zones, ranks, environment knobs) by plan_step() at every constants
// upload, which each change of the configuration ends in; launch_step reads it.
struct StepPlan {
  StepEntry entry{};                    // the compiled-in step of the engine's tables
  // a stub: an experiment build without this table (GPU_ACTOR_EINVAL); fits:
  // static LDS + dyn within a workgroup's LDS (GPU_ACTOR_ERANGE otherwise)
  bool stub = false, fits = false;
  size_t dyn = 0;                       // dynamic LDS of each k_step launch
  // the compiled-in launches: the whole step (PM 0), or a split table's as
  // one launch (PM 3: first) or two (PM 1: first, PM 2: second)
  step_kernel_t first = nullptr, second = nullptr;
  // the run-time compiled step taken instead where it builds and fits
  // (jit_host.h): 0 none, 1 the programs', 2 the any-mix step of the tables
  // in jit_mask; jit_key names the module. Built or loaded at the first
  // launch (jit_ready), whose answer stands for this plan.
  int jit_kind = 0;
  uint32_t jit_mask = 0;
  uint64_t jit_key = 0;
  bool jit_asked = false, jit_ok = false;
};

// One engine, from gpu_actor_init to gpu_actor_shutdown (or to a failed init):
// every field starts from its initialiser here, the buffers free themselves
// (dev_buf.h), and session_end() replaces the whole value — nothing below is
// named in a teardown list.
struct Session {
  bool init = false;
  gpu_actor_config_t cfg{};
  int device = 0;
  hipStream_t stream = nullptr;
  HostType types[GPU_ACTOR_MAX_TYPES];
  uint32_t n_types = 0;                 // 1 + highest created type id
  uint64_t n_actors = 0;                // global ids handed out
  uint32_t n_local = 0;
  // placement of this session (gpu_actor_place_blocks, verified equal on
  // every rank by init)
  uint32_t block_bits = 0;
  // zones
  uint32_t n_zones = 0;
  uint64_t zone_records = 0;
  DevBuf<uint64_t> d_zoff;
  DevBuf<uint32_t> d_zcap;
  DevBuf<ZRec> d_land[2], d_carry[2];
  DevBuf<uint32_t> d_land_n[2], d_carry_n[2];
  // the compact landing lane (EngDev::landc): allocated with
  // the zone buffers for a table whose sends carry a constant argument;
  // land8: the step uses it (one rank; PONYC_AMD_LAND8=0 turns it off);
  // land8_dirty: a step ran since the lane was last expanded (land8_flush)
  DevBuf<uint2> d_landc[2];
  DevBuf<unsigned long long> d_landc_n[2];
  bool land8 = false, land8_dirty = false;
  uint64_t land8_arg = 0;               // the lane's table's constant argument (StepEntry::plan_arg)
  DevBuf<ZRec> d_S;
  DevBuf<ORec> d_O;
  uint32_t par = 0;                     // parity the next step reads
  DevBuf<unsigned long long> d_stats;
  DevBuf<unsigned long long> d_pend;
  DevBuf<unsigned long long> d_pend_sh;    // [kPendSlots][kShards]: k_step's adds
  DevBuf<unsigned long long> d_stats_sh;   // [ST_COUNT][kShards]
  // hot zones (hot_dev.h k_hot): one allocation, carved into EngDev's arrays
  // (HotLayout)
  DevBuf<uint32_t> d_hot;
  bool hot_on = false;
  int hot_fits = -1;                    // hot_resident()'s answer (-1: not asked yet)
  DevBuf<unsigned long long> d_dbg;     // phase stamps of the diagnostic build
  PinBuf<gpu_msg_t> h_msgs;
  // gpu_actor_send appends here; flushed (one H2D + k_inject) before the
  // next operation that observes device state, so a send costs no sync
  std::vector<gpu_msg_t> deferred;
  DevBuf<gpu_msg_t> d_msgs;
  uint64_t host_seq = 0;
  uint64_t steps_total = 0;
  int sticky = 0;
  // behaviours as programs compiled at run time (jit_host.h): the module of
  // the current program set and geometry, the set a build failed for (kept
  // on the interpreter), the constants last uploaded (for a module loaded
  // later), and how many modules were built or loaded
  jit::Module jit;
  uint64_t jit_set = 0;                 // the program set (and geometry) the module is for
  uint64_t jit_failed = 0;
  uint32_t jit_builds = 0;
  bool jit_used = false;                // the last step ran the compiled module
  TypeDev td_host[GPU_ACTOR_MAX_TYPES] = {};
  EngDev eng_host = {};
  bool consts_host = false;
  // GUPS streamers' chunks for k_gups_apply (EngDev::gups_*; gups_type -1: none)
  DevBuf<uint64_t> d_gups_list;
  DevBuf<unsigned int> d_gups_n;
  DevBuf<uint64_t> d_gups_jump;
  DevBuf<unsigned long long> d_gups_stat;
  uint64_t gups_jump_host[65] = {};
  int gups_type = -1;
  // n_ranks > 1: this rank's chunks packed to one run (k_gups_pack), every
  // rank's runs gathered in rank order for k_gups_apply_ranks; chunks received
  // from peers and listed here since init (gpu_actor_debug_info)
  DevBuf<uint64_t> d_gups_send;
  DevBuf<uint64_t> d_gups_all;
  uint32_t gups_parts = 0;
  uint64_t gups_in_total = 0, gups_out_total = 0;
  // One rank: device work that can change the spill status or the counters
  // bumps dev_epoch; a host read of either records the epoch it saw, so a
  // read that nothing could have changed since is skipped (run_fixed's and
  // gpu_actor_sync's host round trips, bench.py's timed region).
  uint64_t dev_epoch = 1, sstat_epoch = 0, sticky_epoch = 0;
  hipError_t last_hip = hipSuccess;
  std::vector<hipEvent_t> ev;
  double last_drain_ms = 0.0;
  // multi-rank exchange
  ncclComm_t comm = nullptr;
  DevBuf<XRec> d_xout;
  DevBuf<XRec> d_xin;
  // [3R + 3]: send counts, receive counts, two scratch words, the GUPS chunks
  // this rank listed in the step (k_gups_pack), every rank's such count
  DevBuf<unsigned long long> d_xc;
  unsigned long long* d_xcount = nullptr;  // d_xc
  unsigned long long* d_xrecv = nullptr;   // d_xc + R
  PinBuf<unsigned long long> h_xc;         // pinned mirror of d_xc
  DevBuf<unsigned int> d_spill_flag;       // spill lists in use on any rank (summed)
  uint32_t xcap = 0;                       // records per peer segment of xout
  DevBuf<XSpillRec> d_xspill;              // cross-rank records past xcap
  DevBuf<unsigned int> d_xspill_n;
  uint32_t xspill_cap = 0;
  std::vector<unsigned long long> h_xcount, h_xrecv;   // host transport
  uint64_t remote_total = 0;
  // peer writes (PONYC_AMD_PEER_WRITE=1, EngDev::peer_write): this rank's
  // inbox [R][xcap] (segment p: peer p's records, stored by peer p's k_step),
  // every peer's inbox mapped over IPC, and a small collective scratch
  bool peer_write = false;
  DevBuf<XRec> d_pin;
  XRec* peer_ptr[kMaxRanks] = {};
  DevBuf<unsigned long long> d_hx;         // [1 + R]
  // host transport staging (pinned): what this rank sends, what it receives
  PinBuf<uint8_t> h_sbuf, h_rbuf;
  // spawned actors (gpu_actor_type_reserve)
  uint32_t spawn_cap = 0;
  DevBuf<uint64_t> d_skey[2], d_sarg[2];
  DevBuf<unsigned int> d_spawn_n;
  DevBuf<uint32_t> d_tstart, d_tcnt;
  DevBuf<unsigned long long> d_live;     // [GPU_ACTOR_MAX_TYPES] live actors per type
  DevBuf<uint8_t> d_sort_tmp;            // hipcub's scratch (sort_room)
  // backpressure: trigger bytes per global id and parity
  // (d_trig_own: this rank's own bytes when n_ranks > 1, merged into d_trig),
  // the receiver each muted local actor waits on, per-zone trigger counts,
  // per-step counts (index = step mod 3), and the step index
  DevBuf<uint8_t> d_trig[2], d_trig_own[2];
  uint64_t trig_bytes = 0;
  bool trig_stale[2] = {false, false};
  DevBuf<uint32_t> d_muted_on;
  DevBuf<uint32_t> d_ztrig[2];
  DevBuf<unsigned int> d_trig_n;
  // zones the step's two-pass launch ran (EngDev::zplan)
  DevBuf<uint32_t> d_zplan;
  // what a step launches in this configuration (plan_step, from upload_types)
  StepPlan plan;
  uint32_t sidx = 0;
  // backlog copies handed to k_carry_big (EngDev::bigc)
  DevBuf<BigCopy> d_bigc;
  DevBuf<unsigned long long> d_bigc_n;
  bool defer_big = false;
  // records past zone capacity: spill lists, their counters, and the minimum
  // capacity each zone has grown to
  DevBuf<SpillRec> d_spill[2];
  uint32_t spill_cap = 0;
  DevBuf<SpillStat> d_sstat;
  PinBuf<SpillStat> h_sstat;
  DevBuf<uint32_t> d_need;
  std::vector<uint32_t> zcap_min, zcap_host;
  uint64_t fixups = 0;
  // small-step path (k_sparse)
  DevBuf<SparseCtl> d_ctl;
  PinBuf<SparseCtl> h_ctl;
  uint64_t sparse_launches = 0, sparse_steps = 0;
  // zone geometry: actors per zone = 1 << zbits (step_entry.h; chosen by
  // relayout_zones)
  uint32_t zbits = kZoneBits;
  // messages to the host (include/gpu_actor_host.h): host_ports once a port
  // type exists (nothing below is allocated, launched or waited for before);
  // host_dirty: steps ran since the last collection, the first of them step
  // host_base; host_defer: gpu_actor_run_fixed is launching (it collects
  // nothing itself). The list (EngDev::host_*: kHostShards segments of
  // host_seg records), the compacted and the sorted keys and places, the
  // gathered messages and their pinned mirror; the key's step field starts
  // at bit host_kshift (16 sequence bits + the bits of max_actors - 1).
  bool host_ports = false, host_dirty = false, host_defer = false;
  uint32_t host_base = 0;
  uint64_t host_reserve = GPU_ACTOR_HOST_RESERVE_DEFAULT;
  uint32_t host_seg = 0, host_kshift = 48;
  struct HostLists {                       // sized by host_reserve (host_alloc)
    DevBuf<uint64_t> d_host_key, d_host_kc, d_host_ks;
    DevBuf<uint32_t> d_host_ic, d_host_is;
    DevBuf<uint4> d_host_rec;
    DevBuf<gpu_host_msg_t> d_host_out;
    PinBuf<gpu_host_msg_t> h_host_out;
  } hl;
  DevBuf<unsigned int> d_host_n;
  PinBuf<unsigned int> h_host_n;
  DevBuf<uint64_t> d_host_step;
  // collected messages not yet received (gpu_actor_recv), from hostq_head on;
  // or the callback that takes them instead (gpu_actor_host_notify)
  std::vector<gpu_host_msg_t> hostq;
  size_t hostq_head = 0;
  gpu_actor_host_fn host_fn = nullptr;
  void* host_ctx = nullptr;
};

Process gp;
// On the heap and never destroyed: a process that exits without
// gpu_actor_shutdown runs no HIP call from a static destructor.
Session& g = *new Session;

#define HIPCK(expr)                                                    \
  do {                                                                 \
    hipError_t e_ = (expr);                                            \
    if(e_ != hipSuccess) {                                             \
      g.last_hip = e_;                                                 \
      fprintf(stderr, "gpu_actor: %s failed: %s (%s:%d)\n", #expr,     \
        hipGetErrorString(e_), __FILE__, __LINE__);                    \
      return GPU_ACTOR_EHIP;                                           \
    }                                                                  \
  } while(0)

#define NCCLCK(expr)                                                   \
  do {                                                                 \
    ncclResult_t r_ = (expr);                                          \
    if(r_ != ncclSuccess) {                                            \
      fprintf(stderr, "gpu_actor: %s failed: %s\n", #expr,            \
        ncclGetErrorString(r_));                                       \
      return GPU_ACTOR_ECOMM;                                          \
    }                                                                  \
  } while(0)

inline uint32_t R() { return g.cfg.n_ranks; }
inline uint32_t rank() { return g.cfg.rank; }

// The placement (include/gpu_actor_place.h): blocks of 2^b consecutive ids
// dealt round-robin over n ranks. Pure functions of (n, b): the public
// gpu_actor_place_map / _global and the session's own bookkeeping.
inline uint32_t place_owner(uint32_t n, uint32_t b, uint64_t id) { return (uint32_t)((id >> b) % n); }
inline uint64_t place_slot(uint32_t n, uint32_t b, uint64_t id)
{
  return (((id >> b) / n) << b) | (id & ((1ull << b) - 1));
}
inline uint64_t place_global(uint32_t n, uint32_t b, uint32_t r, uint64_t slot)
{
  return ((((slot >> b) * n) + r) << b) | (slot & ((1ull << b) - 1));
}
// number of ids < x owned by rank r: its whole blocks below x's block, and
// the part of x's block below x if that block is r's
inline uint64_t place_below(uint32_t n, uint32_t b, uint32_t r, uint64_t x)
{
  const uint64_t f = x >> b;
  return ((f > r ? (f - r + n - 1) / n : 0) << b) + (f % n == r ? x & ((1ull << b) - 1) : 0);
}

// number of ids < x owned by this rank
inline uint64_t owned_below(uint64_t x)
{
  return place_below(R(), g.block_bits, rank(), x);
}

// n_ranks > 1: some rank owns none of the ids handed out (fewer blocks of
// ids than ranks, under any placement). Such a rank has no zone and launches
// no step, and a step's exchange needs every rank: the run calls refuse such
// a world (run_locked, gpu_actor_run_fixed). Every rank computes the same
// answer from the same global values, so all refuse alike, before any
// collective. (A world without any actor has nothing to run on any rank.)
inline bool rank_without_actors()
{
  if(R() == 1 || g.n_actors == 0) return false;
  for(uint32_t r = 0; r < R(); ++r)
    if(place_below(R(), g.block_bits, r, g.n_actors) == 0) return true;
  return false;
}

inline uint32_t blocks_for(uint64_t n, uint32_t bs = kBlock) { return (uint32_t)((n + bs - 1) / bs); }

// actors per zone in this engine's geometry
inline uint32_t zone_actors() { return 1u << g.zbits; }

// tables whose actors are no serial actors: they have no mailbox and never
// run, take no zone capacity, and do not count towards the step kernel's
// choice — the reducible types, and host ports (include/gpu_actor_host.h)
inline bool reducible_ht(uint32_t ht)
{
  return ht == GPU_ACTOR_HT_FANIN_ANALYZER || ht == GPU_ACTOR_HT_GUPS_UPDATER ||
         ht == GPU_ACTOR_HT_HOST_PORT;
}

// The compiled steps (step_entry.h GPA_STEP_TABLES): a row per table, its
// entry at each zone geometry.
struct StepRow {
  int ht;
  StepEntry geo[2];        // [0]: 2048-actor zones, [1]: 4096-actor zones
};
// the handler tables of the engine's serial actors, a bit per table id
uint32_t serial_tables()
{
  uint32_t set = 0;
  for(const HostType& t : g.types)
    if(t.created && !reducible_ht(t.ht)) set |= 1u << t.ht;
  return set;
}

const std::vector<StepRow>& step_rows()
{
  static const std::vector<StepRow> v = {
#define GPA_STEP_X(name, ht) {ht, {gpa::step_entry_##name(), gpa_z12::step_entry_##name()}},
    GPA_STEP_TABLES(GPA_STEP_X)
#undef GPA_STEP_X
  };
  return v;
}

// The step of handler table ht (kHtFifoPair: the FIFO pair; -1, and every
// table without a step of its own: the any-mix step) at a geometry.
const StepEntry& step_entry(int ht, bool z12)
{
  const StepEntry* any = nullptr;
  for(const StepRow& r : step_rows())
  {
    if(r.ht == ht) return r.geo[z12];
    if(r.ht == -1) any = &r.geo[z12];
  }
  return *any;
}

// k_step compiled for the one handler table all serial actors share, when
// they do (smaller code, no spills); the any-mix instantiation otherwise.
StepEntry step_entry_for(bool z12)
{
  const uint32_t set = serial_tables();
  // the FIFO pair's rule comes first: sources and sinks, and nothing else
  if(set == ((1u << GPU_ACTOR_HT_FIFO_SRC) | (1u << GPU_ACTOR_HT_FIFO_SINK)))
    return step_entry(kHtFifoPair, z12);
  return step_entry(set && !(set & (set - 1)) ? __builtin_ctz(set) : -1, z12);
}

StepEntry pick_step_entry() { return step_entry_for(g.zbits == 12); }

// LDS a workgroup may hold on gfx950 (the CU's whole 160 KB; two 512-thread
// zones per CU at <= 80 KB each)
constexpr size_t kLdsPerWorkgroup = 160 * 1024;

// Dynamic LDS of a step launch with nb destination buckets: the bucket
// arrays (zone_dev.h: histogram, chunk bases, tile counts, tile starts, and
// the two-pass table's round counts) or the hot-group sort's work area.
size_t step_dyn_bytes(const StepEntry& se, uint64_t nb)
{
  return sizeof(uint32_t) * std::max<uint64_t>((uint64_t)se.bucket_words * nb, se.sort_work);
}

// Whether a step launch with nb buckets fits a workgroup's LDS: static LDS of
// every kernel of the entry (hipFuncGetAttributes) + the dynamic part.
bool step_fits(const StepEntry& se, uint64_t nb)
{
  static std::map<step_kernel_t, size_t> cache;     // (callers hold gp.mu)
  size_t st = 0;
  for(step_kernel_t k : {se.kernel, se.plan, se.rest, se.fused})
  {
    if(!k) continue;
    auto it = cache.find(k);
    if(it == cache.end())
    {
      hipFuncAttributes a;
      if(hipFuncGetAttributes(&a, reinterpret_cast<const void*>(k)) != hipSuccess) return false;
      it = cache.emplace(k, a.sharedSizeBytes).first;
    }
    st = std::max<size_t>(st, it->second);
  }
  return st + step_dyn_bytes(se, nb) <= kLdsPerWorkgroup;
}

// Backlog copies go to k_carry_big (the whole GPU copies them right after
// k_step) in engines whose serial actors run more than one handler table —
// the fan-in shapes (sources and sinks of different kinds) that build
// backlogs of thousands of records per actor. The extra launch per step costs
// 2.4 % of a C2-det step and 1 % of a C5 step (profiles/r04j_hot_msd.txt,
// PONYC_AMD_DEFER_BIG=0/1), where backlogs over 128 records are rare and a
// zone copies one itself. PONYC_AMD_DEFER_BIG=0/1 forces it (tests, A/B).
bool defer_big_wanted()
{
  if(const char* f = getenv("PONYC_AMD_DEFER_BIG")) return atoi(f) != 0;
  const uint32_t set = serial_tables();
  return (set & (set - 1)) != 0;
}

inline uint32_t* hot_bar_words() { return g.d_hot + kHotLayout.bar; }

// k_hot's workgroups must all be resident at once (its phases meet at grid
// barriers, hot_dev.h): kHotBlocks workgroups of kHotThreads with the LDS of
// the larger zone geometry, against the occupancy the runtime reports for
// this device (one workgroup per CU on half the CUs is what it needs; the
// reported figure can exceed the hardware's by one workgroup per CU,
// MI355X_MICROARCH.md, so one is taken off). Asked once per engine.
bool hot_resident()
{
  int& cached = g.hot_fits;
  if(cached >= 0) return cached != 0;
  int per_cu = 0, cus = 0;
  const size_t lds = 5u * kHotActors * sizeof(uint32_t);
  if(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, reinterpret_cast<const void*>(k_hot),
       (int)kHotThreads, lds) != hipSuccess ||
     hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, g.device) != hipSuccess)
  {
    (void)hipGetLastError();
    cached = 0;
    return false;
  }
  cached = (uint64_t)std::max(per_cu - 1, per_cu > 0 ? 1 : 0) * (uint64_t)cus >= kHotBlocks ? 1 : 0;
  return cached != 0;
}

constexpr uint32_t kGupsBlocks = 1024;
constexpr uint32_t kGupsPackBlocks = 256;
__global__ void __launch_bounds__(256) k_gups_apply();
__global__ void __launch_bounds__(256) k_gups_pack(uint64_t* out, unsigned long long* count);
__global__ void __launch_bounds__(256) k_gups_apply_ranks(const uint64_t* list, uint64_t n,
  uint64_t own_lo, uint64_t own_n);

// The GUPS streamer type whose chunks k_gups_apply makes (EngDev::gups_*): the
// first with a nonzero chunk, at any rank count (PONYC_AMD_GUPS_DEFER=0: none,
// every streamer applies its own chunk, for A/B runs; the ranks of one engine
// must agree on it, as on every setting). Chunks of L >= 16 updates per lane,
// at most 64 lanes per chunk. With n_ranks > 1 the listed chunks are packed,
// gathered by every rank and applied by k_gups_apply_ranks (gups_gather_apply).
int gups_setup(EngDev& e)
{
  g.gups_type = -1;
  e.gups_type = -1;
  const char* f = getenv("PONYC_AMD_GUPS_DEFER");
  if(f && atoi(f) == 0) return 0;
  int t_def = -1;
  for(uint32_t t = 0; t < GPU_ACTOR_MAX_TYPES && t_def < 0; ++t)
    if(g.types[t].created && g.types[t].ht == GPU_ACTOR_HT_GUPS_STREAMER && g.types[t].params[0] > 0 &&
       g.types[t].params[0] <= 0xFFFFFFFFull)
      t_def = (int)t;
  if(t_def < 0) return 0;
  const HostType& h = g.types[t_def];
  const uint64_t chunk = h.params[0];
  const uint64_t L = std::max<uint64_t>(16, (chunk + 63) / 64);
  const uint64_t parts = (chunk + L - 1) / L;
  // kGupsShards segments, each at least 2^16 chunks (k_sparse lists from its
  // few waves' segments only)
  const uint64_t cap = std::min<uint64_t>(std::max<uint64_t>(1ull << 22, 2ull * h.lcount), 1ull << 28);
  if(cap > g.d_gups_list.size())
  {
    HIPCK(hipStreamSynchronize(g.stream));      // no k_gups_apply still reads the old list
    HIPCK(g.d_gups_list.alloc(cap));
    // the packed run holds what the list holds (between steps both are empty)
    g.d_gups_send.reset();
  }
  if(R() > 1 && !g.d_gups_send)
    HIPCK(g.d_gups_send.alloc(g.d_gups_list.size()));
  if(!g.d_gups_n)
  {
    HIPCK(g.d_gups_n.alloc(kGupsShards + 1));
    HIPCK(hipMemsetAsync(g.d_gups_n, 0, (kGupsShards + 1) * sizeof(unsigned int), g.stream));
    HIPCK(g.d_gups_jump.alloc(65));
    HIPCK(g.d_gups_stat.alloc(3 * kGupsBlocks));
    HIPCK(hipMemsetAsync(g.d_gups_stat, 0, 3 * kGupsBlocks * sizeof(unsigned long long), g.stream));
  }
  uint64_t jump[65] = {};
  for(uint64_t p = 0; p < parts; ++p) jump[p] = gpa::polyrand_xpow(p * L);
  jump[parts] = gpa::polyrand_xpow(chunk);
  if(memcmp(jump, g.gups_jump_host, sizeof(jump)) != 0)
  {
    HIPCK(hipStreamSynchronize(g.stream));      // no launch still reads the old table
    memcpy(g.gups_jump_host, jump, sizeof(jump));
    HIPCK(hipMemcpyAsync(g.d_gups_jump, g.gups_jump_host, sizeof(jump), hipMemcpyHostToDevice,
      g.stream));
  }
  e.gups_list = g.d_gups_list; e.gups_n = g.d_gups_n; e.gups_jump = g.d_gups_jump;
  e.gups_stat = g.d_gups_stat;
  e.gups_seg = (uint32_t)(g.d_gups_list.size() / kGupsShards);
  {
    // (tests: PONYC_AMD_GUPS_SEG=n lists at most n chunks per segment, so that
    // full segments send the rest through the streamers' own path)
    const char* sg = getenv("PONYC_AMD_GUPS_SEG");
    if(sg && atoi(sg) > 0) e.gups_seg = std::min<uint32_t>(e.gups_seg, (uint32_t)atoi(sg));
  }
  e.gups_l = (uint32_t)L; e.gups_parts = (uint32_t)parts;
  e.gups_type = t_def;
  g.gups_type = t_def;
  g.gups_parts = (uint32_t)parts;
  return 0;
}

// k_gups_apply behind a step's kernels (engines with a chunk-listing streamer
// type, one rank; with more the chunks are applied after the exchange,
// gups_gather_apply)
int gups_apply_launch()
{
  if(g.gups_type < 0 || R() > 1) return 0;
  hipLaunchKernelGGL(k_gups_apply, dim3(kGupsBlocks), dim3(256), 0, g.stream);
  HIPCK(hipGetLastError());
  return 0;
}

bool land8_table();
void plan_step(const StepEntry& se);

int upload_types()
{
  const StepEntry se = pick_step_entry();
  plan_step(se);
  TypeDev td[GPU_ACTOR_MAX_TYPES];
  memset(td, 0, sizeof(td));
  for(uint32_t t = 0; t < GPU_ACTOR_MAX_TYPES; ++t)
  {
    const HostType& h = g.types[t];
    TypeDev& d = td[t];
    if(!h.created) continue;
    d.first = (uint32_t)h.first; d.count = (uint32_t)h.count;
    d.lfirst = h.lfirst; d.lcount = h.lcount;
    d.ht = h.ht; d.words = h.words; d.batch = h.batch; d.cap = h.cap;
    d.reducible = reducible_ht(h.ht);
    d.prio = h.priority > 0 ? 1u : 0u;
    d.state = h.d_state;
    memcpy(d.params, h.params, sizeof(d.params));
    d.prog = h.d_prog;
    d.prog_n = h.prog_n;
    d.prog_pad = h.prog_yields ? 1u : 0u;
  }
  HIPCK(hipMemcpyToSymbolAsync(HIP_SYMBOL(c_types), td, sizeof(td), 0,
    hipMemcpyHostToDevice, g.stream));
  EngDev e;
  memset(&e, 0, sizeof(e));
  e.n_types = g.n_types; e.rank = rank(); e.nranks = R(); e.n_local = g.n_local;
  e.n_zones = g.n_zones; e.zoff = g.d_zoff; e.zcapz = g.d_zcap;
  e.n_ids = (uint32_t)std::min<uint64_t>(g.n_actors, 0xFFFFFFFFull);
  e.r_magic = R() > 1 ? ~0ull / R() + 1 : 0;
  for(int p = 0; p < 2; ++p)
  {
    e.land[p] = g.d_land[p]; e.carry[p] = g.d_carry[p];
    e.land_n[p] = g.d_land_n[p]; e.carry_n[p] = g.d_carry_n[p];
  }
  e.S = g.d_S; e.O = g.d_O;
  e.stats = g.d_stats; e.pend = g.d_pend;
  e.pend_sh = g.d_pend_sh; e.stats_sh = g.d_stats_sh;
  {
    uint32_t* h = g.d_hot;
    const HotLayout& L = kHotLayout;
    e.hot_prep = h + L.prep; e.hot_slot = h + L.slot; e.hot_cnt = h + L.cnt; e.hot_aux = h + L.aux;
    e.hot_hist = h + L.hist; e.hot_bcnt = h + L.bcnt; e.hot_cur = h + L.cur; e.hot_bar = h + L.bar;
  }
  e.xout = g.d_xout; e.xcount = g.d_xcount; e.xcap = g.xcap;
  e.peer_write = g.peer_write ? 1u : 0u;
  for(uint32_t p = 0; p < R() && p < kMaxRanks; ++p)
    e.xdst[p] = g.peer_write ? (g.peer_ptr[p] ? g.peer_ptr[p] + (size_t)rank() * g.xcap : nullptr)
                             : (g.d_xout ? g.d_xout + (size_t)p * g.xcap : nullptr);
  e.seq_max = R() > 1 ? kXSeqMax : kSeqMax;
  e.dbg = g.d_dbg;
  e.spawn_key = g.d_skey[0]; e.spawn_arg = g.d_sarg[0];
  e.spawn_n = g.d_spawn_n; e.spawn_cap = g.spawn_cap;
  for(int p = 0; p < 2; ++p)
  {
    e.trig[p] = g.d_trig[p];
    e.trig_own[p] = R() > 1 ? g.d_trig_own[p] : g.d_trig[p];
    e.ztrig[p] = g.d_ztrig[p];
  }
  e.muted_on = g.d_muted_on;
  e.spill_flag = g.d_spill_flag;
  e.trig_n = g.d_trig_n;
  e.spill[0] = g.d_spill[0]; e.spill[1] = g.d_spill[1];
  e.spill_n = g.d_sstat ? g.d_sstat->spill_n : nullptr;
  e.halt = g.d_sstat ? &g.d_sstat->halt : nullptr;
  e.skipped = g.d_sstat ? &g.d_sstat->skipped : nullptr;
  e.spill_cap = g.spill_cap;
  e.xspill = g.d_xspill; e.xspill_n = g.d_xspill_n; e.xspill_cap = g.xspill_cap;
  e.zbits = g.zbits;
  e.block_bits = g.block_bits;
  {
    g.land8 = land8_table() && g.d_landc[0] && g.d_landc[1] && g.d_sstat;
    if(g.land8) g.land8_arg = se.plan_arg;
    e.land8 = g.land8 ? 1u : 0u;
    for(int p = 0; p < 2; ++p) { e.landc[p] = g.d_landc[p]; e.landc_n[p] = g.d_landc_n[p]; }
    e.lc_over = g.d_sstat ? &g.d_sstat->lc_over : nullptr;
  }
  g.defer_big = defer_big_wanted();
  // k_hot runs where backlogs build (the same engines as defer_big);
  // PONYC_AMD_HOT=0/1 forces it (tests, A/B)
  // It runs only where its grid is resident at once (hot_resident): its
  // phases meet at grid barriers.
  {
    const char* f = getenv("PONYC_AMD_HOT");
    g.hot_on = se.hot && (f ? atoi(f) != 0 : g.defer_big) && hot_resident();
    e.hot_on = g.hot_on ? 1u : 0u;
    const char* t = getenv("PONYC_AMD_HOT_TEST");
    e.hot_test = (t && atoi(t) != 0) ? 1u : 0u;
  }
  e.bigc = g.d_bigc; e.bigc_n = g.d_bigc_n; e.bigc_cap = kBigCopyCap;
  e.defer_big = g.defer_big ? 1u : 0u;
  {
    const char* f = getenv("PONYC_AMD_TWO_PASS");
    e.two_pass = (f && atoi(f) == 0) ? 0u : 1u;
  }
  e.zplan = g.d_zplan;
  if(g.host_ports && g.host_seg)     // (host_seg 0: the lists could not be allocated)
  {
    uint64_t lo = ~0ull, hi = 0;
    for(uint32_t t = 0; t < GPU_ACTOR_MAX_TYPES; ++t)
    {
      const HostType& h = g.types[t];
      if(!h.created || h.ht != GPU_ACTOR_HT_HOST_PORT) continue;
      e.host_rng[e.host_nrng].first = (uint32_t)h.first;
      e.host_rng[e.host_nrng].count = (uint32_t)h.count;
      e.host_rng[e.host_nrng].type = t;
      e.host_nrng++;
      lo = std::min(lo, h.first);
      hi = std::max(hi, h.first + h.count);
    }
    e.host_first = e.host_nrng ? (uint32_t)lo : 0u;
    e.host_span = e.host_nrng ? (uint32_t)(hi - lo) : 0u;
    e.host_seg = g.host_seg;
    e.host_key = g.hl.d_host_key; e.host_rec = g.hl.d_host_rec; e.host_n = g.d_host_n;
    e.host_step = g.d_host_step;
  }
  {
    const int rc = gups_setup(e);
    if(rc) return rc;
  }
  HIPCK(hipMemcpyToSymbolAsync(HIP_SYMBOL(c_eng), &e, sizeof(e), 0,
    hipMemcpyHostToDevice, g.stream));
  // every k_step code object holds its own copy of the constants
  for(const StepRow& r : step_rows())
    for(const StepEntry& u : r.geo)
      HIPCK(u.upload(td, &e, g.stream));
  memcpy(g.td_host, td, sizeof(td));
  g.eng_host = e;
  g.consts_host = true;
  if(g.jit.mod)
  {
    HIPCK(hipMemcpyHtoDAsync(g.jit.types, g.td_host, sizeof(g.td_host), g.stream));
    HIPCK(hipMemcpyHtoDAsync(g.jit.eng, &g.eng_host, sizeof(g.eng_host), g.stream));
  }
  return 0;
}

// Spill lists of at least `cap` records per parity (they start empty between
// steps, so growing them moves nothing).
int ensure_spill(uint64_t cap)
{
  cap = std::min<uint64_t>(cap, 0x7FFFFFFFull);
  if(cap <= g.spill_cap) return 0;
  g.spill_cap = 0;
  for(int p = 0; p < 2; ++p) HIPCK(g.d_spill[p].alloc(cap));
  g.spill_cap = (uint32_t)cap;
  return 0;
}

int relayout_zones(bool geometry = false);
int land8_flush();
int pend_read(uint32_t first, uint32_t n, std::vector<unsigned long long>& out);

// Spill list length for the current zone layout: a quarter of its records.
inline uint64_t spill_cap_for_zones()
{
  return std::max<uint64_t>(1u << 20, g.zone_records / 4);
}

int read_sstat()
{
  HIPCK(hipMemcpyAsync(g.h_sstat, g.d_sstat, sizeof(SpillStat), hipMemcpyDeviceToHost,
    g.stream));
  HIPCK(hipStreamSynchronize(g.stream));
  g.sstat_epoch = g.dev_epoch;
  return 0;
}

inline bool spill_pending()
{
  return g.h_sstat->spill_n[0] || g.h_sstat->spill_n[1] || g.h_sstat->halt || g.h_sstat->lc_over;
}

// Whether the engine's step is that of a table with a compact landing lane.
// (With n_ranks > 1 only a rank's own zones have one: a peer's records stay
// 16-byte XRecs, which k_xinject lands in land[]; a lane that needs the host
// on any rank halts every rank's next step, k_spill_flag.)
bool land8_table()
{
  const char* f = getenv("PONYC_AMD_LAND8");
  return pick_step_entry().const_arg && !(f && atoi(f) == 0);
}

// Empty the compact lane of both parities into the 16-byte landing buffers
// (k_land_expand), when a step may have written it since the last time.
int land8_flush()
{
  if(!g.land8 || !g.land8_dirty || g.n_zones == 0) return 0;
  for(uint32_t p = 0; p < 2; ++p)
    hipLaunchKernelGGL(k_land_expand, dim3(g.n_zones), dim3(kBlock), 0, g.stream, p, g.land8_arg);
  HIPCK(hipGetLastError());
  g.land8_dirty = false;
  g.dev_epoch++;
  return 0;
}

// Grow every zone that spilled, land the spilled records at the positions
// they were given, and release the halt (SpillRec, engine_dev.h). Uses the
// status last read into h_sstat. Nothing is dropped unless a spill list
// itself overflowed (counted; the run then fails with GPU_ACTOR_EMAILBOX).
// With n_ranks > 1 every rank calls it together (the decision is summed over
// ranks: settle_spills, run_locked) and it always clears the spill flag, even
// with nothing of its own to land, so that every rank's next step runs alike.
int fixup_spill()
{
  // the compact lane first: what does not fit its zone joins the spill lists
  // (this rank's own word: a rank whose lanes fit has nothing to expand)
  if(g.h_sstat->lc_over)
  {
    g.land8_dirty = true;
    int rc = land8_flush();
    if(rc) return rc;
    rc = read_sstat();
    if(rc) return rc;
  }
  const SpillStat st = *g.h_sstat;
  g.dev_epoch++;
  if(R() == 1 && !st.spill_n[0] && !st.spill_n[1] && !st.halt) return 0;
  uint32_t n[2], most = 0;
  for(int p = 0; p < 2; ++p)
  {
    n[p] = std::min(st.spill_n[p], g.spill_cap);
    most = std::max(most, st.spill_n[p]);
  }
  if(n[0] || n[1])
  {
    const uint32_t nz = g.n_zones;
    HIPCK(hipMemsetAsync(g.d_need, 0, nz * sizeof(uint32_t), g.stream));
    for(int p = 0; p < 2; ++p)
      if(n[p])
        hipLaunchKernelGGL(k_spill_need, dim3(blocks_for(n[p])), dim3(kBlock), 0, g.stream,
          (const SpillRec*)g.d_spill[p], n[p], g.d_need);
    HIPCK(hipGetLastError());
    std::vector<uint32_t> need(nz);
    HIPCK(hipMemcpyAsync(need.data(), g.d_need, nz * sizeof(uint32_t), hipMemcpyDeviceToHost,
      g.stream));
    HIPCK(hipStreamSynchronize(g.stream));
    bool grow = false;
    for(uint32_t z = 0; z < nz; ++z)
      if(need[z] > g.zcap_host[z])
      {
        // double, or 1.5x what this step needed: a burst seldom grows a zone twice
        const uint64_t want = std::max<uint64_t>(2ull * g.zcap_host[z], need[z] + need[z] / 2);
        g.zcap_min[z] = (uint32_t)std::min<uint64_t>((want + 15) & ~15ull, kSpillPosMask);
        grow = true;
      }
    if(grow)
    {
      int rc = relayout_zones();
      if(rc) return rc;
      rc = upload_types();
      if(rc) return rc;
    }
    for(int p = 0; p < 2; ++p)
      if(n[p])
        hipLaunchKernelGGL(k_spill_place, dim3(blocks_for(n[p])), dim3(kBlock), 0, g.stream,
          (const SpillRec*)g.d_spill[p], n[p], (uint32_t)p);
    HIPCK(hipGetLastError());
  }
  HIPCK(hipMemsetAsync(g.d_sstat, 0, sizeof(SpillStat), g.stream));
  HIPCK(hipMemsetAsync(g.d_spill_flag, 0, sizeof(unsigned int), g.stream));
  HIPCK(hipStreamSynchronize(g.stream));
  memset(g.h_sstat, 0, sizeof(SpillStat));
  g.fixups++;
  // Only now, with every spilled record placed, may the lists be re-sized
  // (ensure_spill drops their contents): to the grown zones' share, and
  // larger when a list overflowed (those records were counted as dropped).
  // Re-sizing them inside relayout_zones, before k_spill_place had read them,
  // lost every spilled record of a burst that grew the zones past 4 M records
  // (round 3's 2048-sink backlog gap).
  const uint64_t want = std::max<uint64_t>(spill_cap_for_zones(),
                                           most > g.spill_cap ? 2ull * most : 0ull);
  if(want > g.spill_cap)
  {
    const int rc = ensure_spill(want);
    if(rc) return rc;
    return upload_types();
  }
  return 0;
}

// Re-lay the zone buffers after actors were created: zone z holds
// Σ_{serial actors in z} cap(type) records. Capacities only grow, so mail
// already landed or carried is copied zone by zone into the new layout.
// The zone geometry for n local actors (step_entry.h): 2048-actor zones with
// two 512-thread workgroups per CU while the buckets are few; past ~640
// buckets their four LDS bucket arrays no longer leave room for two
// workgroups per CU, and 4096-actor zones (half the buckets, twice the run
// length per bucket, one 1024-thread workgroup per CU) are faster — C5's 8M
// actors: 2.20 -> 1.58 ms per step (profiles/r03_general.txt). Their LDS
// holds up to ~2300 buckets.
uint32_t pick_zone_bits(uint64_t n)
{
  const uint64_t rb = R() > 1 ? R() : 0;
  const uint64_t nz11 = (n + 2047) / 2048, nz12 = (n + 4095) / 4096;
  if(const char* f = getenv("PONYC_AMD_ZONE_BITS"))      // test hook: force a geometry
    return atoi(f) == 12 ? 12u : 11u;
  // 4096-actor zones while their bucket arrays fit the LDS beside the z12
  // kernels' static LDS (~2,200 buckets; ~1,500 for a dp table's six
  // arrays); past that, 2048-actor zones at one workgroup per CU
  return (nz11 + rb > 640 && step_fits(step_entry_for(true), nz12 + rb)) ? 12u : 11u;
}

// No mail anywhere (landing or carried, either parity): a geometry change
// then moves nothing.
bool zones_empty()
{
  if(g.n_zones == 0) return true;
  if(land8_flush() != 0) return false;
  std::vector<uint32_t> v(g.n_zones);
  for(int p = 0; p < 2; ++p)
    for(const uint32_t* src : {g.d_land_n[p].get(), g.d_carry_n[p].get()})
    {
      if(hipMemcpy(v.data(), src, g.n_zones * sizeof(uint32_t), hipMemcpyDeviceToHost) != hipSuccess)
        return false;
      for(uint32_t x : v)
        if(x) return false;
    }
  return true;
}

// geometry: the zone geometry may be re-chosen (gpu_actor_create only: every
// rank creates alike, so the collective below is reached by all of them; a
// spill fixup can run on one rank alone and keeps the geometry).
int relayout_zones(bool geometry)
{
  // the geometry may change only before any step ran, with no mail landed
  // (zone buffers are copied zone by zone below)
  // Every rank must pick the same geometry (the trigger-byte merge and the
  // bucket layout assume it), so the choice follows the largest rank's share
  // (rank 0's: ceil(n_actors / R) with single-id blocks), not this rank's own
  // count, which can be less; and
  // whether mail has landed anywhere is summed over ranks (create is called
  // by every rank alike, so this collective is reached by all of them).
  bool fresh = false;
  // (the compact lane's records move as 16-byte ones: expanded in the old layout)
  {
    const int rc = land8_flush();
    if(rc) return rc;
  }
  {
    const uint32_t want = pick_zone_bits(place_below(R(), g.block_bits, 0, g.n_actors));
    if(geometry && want != g.zbits && g.steps_total == 0 && g.sparse_launches == 0)
    {
      HIPCK(hipStreamSynchronize(g.stream));
      bool empty = zones_empty();
      if(R() > 1)
      {
        const unsigned long long mine = empty ? 0ull : 1ull;
        HIPCK(hipMemcpyAsync(g.d_pend + kPendPre, &mine, sizeof(mine), hipMemcpyHostToDevice,
          g.stream));
        std::vector<unsigned long long> pv;
        const int rc = pend_read(kPendPre, 1, pv);
        if(rc) return rc;
        empty = pv[0] == 0;
      }
      if(empty)
      {
        g.zbits = want;
        g.zcap_min.clear();
        fresh = true;
      }
    }
  }
  const uint32_t za = zone_actors();
  const uint32_t nz = (uint32_t)((g.n_local + za - 1) / za);
  if(nz > kMaxZones) return GPU_ACTOR_ERANGE;
  std::vector<uint64_t> cap64(nz, 0);
  for(const HostType& t : g.types)
  {
    if(!t.created || reducible_ht(t.ht)) continue;
    for(uint64_t L = t.lfirst; L < (uint64_t)t.lfirst + t.lcount; )
    {
      const uint64_t z = L / za;
      const uint64_t hi = std::min<uint64_t>((z + 1) * za, (uint64_t)t.lfirst + t.lcount);
      cap64[z] += (hi - L) * t.cap;
      L = hi;
    }
  }
  std::vector<uint32_t> cap(nz);
  std::vector<uint64_t> off(nz);
  uint64_t total = 0;
  if(g.zcap_min.size() < nz) g.zcap_min.resize(nz, 0);
  for(uint32_t z = 0; z < nz; ++z)
  {
    cap64[z] = std::max<uint64_t>(cap64[z], g.zcap_min[z]);
    if(cap64[z] > (uint64_t)kSpillPosMask) return GPU_ACTOR_ERANGE;
    cap[z] = (uint32_t)cap64[z];
    off[z] = total;
    total += (cap[z] + 15u) & ~15u;          // keep every zone 256-B aligned
  }
  // The new layout is built in local buffers and swapped in after the last
  // call that can fail: a failure leaves the old layout as it was.
  const size_t recs = std::max<uint64_t>(total, 16), nzn = std::max<size_t>(nz, 1);
  DevBuf<uint64_t> d_off;
  DevBuf<uint32_t> d_cap, ln[2], cn[2], mo;
  DevBuf<ZRec> land[2], carry[2], S;
  DevBuf<ORec> O;
  HIPCK(d_off.alloc(nzn));
  HIPCK(d_cap.alloc(nzn));
  HIPCK(hipMemcpyAsync(d_off, off.data(), nz * sizeof(uint64_t), hipMemcpyHostToDevice, g.stream));
  HIPCK(hipMemcpyAsync(d_cap, cap.data(), nz * sizeof(uint32_t), hipMemcpyHostToDevice, g.stream));
  for(int p = 0; p < 2; ++p)
  {
    HIPCK(land[p].alloc(recs));
    HIPCK(carry[p].alloc(recs));
    HIPCK(ln[p].alloc(nzn));
    HIPCK(cn[p].alloc(nzn));
    HIPCK(hipMemsetAsync(ln[p], 0, nzn * sizeof(uint32_t), g.stream));
    HIPCK(hipMemsetAsync(cn[p], 0, nzn * sizeof(uint32_t), g.stream));
    if(g.n_zones && !fresh)
    {
      hipLaunchKernelGGL(k_zone_copy, dim3(g.n_zones), dim3(kBlock), 0, g.stream,
        (const ZRec*)g.d_land[p], g.d_zoff, g.d_zcap, land[p], (const uint64_t*)d_off);
      hipLaunchKernelGGL(k_zone_copy, dim3(g.n_zones), dim3(kBlock), 0, g.stream,
        (const ZRec*)g.d_carry[p], g.d_zoff, g.d_zcap, carry[p], (const uint64_t*)d_off);
      HIPCK(hipGetLastError());
      HIPCK(hipMemcpyAsync(ln[p], g.d_land_n[p], g.n_zones * sizeof(uint32_t),
        hipMemcpyDeviceToDevice, g.stream));
      HIPCK(hipMemcpyAsync(cn[p], g.d_carry_n[p], g.n_zones * sizeof(uint32_t),
        hipMemcpyDeviceToDevice, g.stream));
    }
    HIPCK(hipStreamSynchronize(g.stream));
  }
  DevBuf<uint2> lc[2];
  DevBuf<unsigned long long> lcn[2];
  if(land8_table())
    for(int p = 0; p < 2; ++p)
    {
      HIPCK(lc[p].alloc(recs));
      HIPCK(lcn[p].alloc(nzn));
      // empty lane; the high words mirror land_n
      hipLaunchKernelGGL(k_land8_mirror, dim3(blocks_for(nzn)), dim3(kBlock), 0, g.stream,
        (const uint32_t*)ln[p], (unsigned long long*)lcn[p], (uint32_t)nzn);
      HIPCK(hipGetLastError());
      HIPCK(hipStreamSynchronize(g.stream));
    }
  HIPCK(S.alloc(3 * recs));                // 2 x: records of a zone; 1 x: sort scratch
  HIPCK(O.alloc(recs));
  // the receiver each muted actor waits on, one word per local slot
  const uint64_t slots = (uint64_t)nz * za;
  if(slots > g.d_muted_on.size())
  {
    HIPCK(mo.alloc(slots));
    HIPCK(hipMemsetAsync(mo, 0, slots * sizeof(uint32_t), g.stream));
    if(g.d_muted_on)
    {
      HIPCK(hipMemcpyAsync(mo, g.d_muted_on, g.d_muted_on.size() * sizeof(uint32_t),
        hipMemcpyDeviceToDevice, g.stream));
      HIPCK(hipStreamSynchronize(g.stream));
    }
    g.d_muted_on.swap(mo);
  }
  for(int p = 0; p < 2; ++p)
  {
    g.d_land[p].swap(land[p]); g.d_carry[p].swap(carry[p]);
    g.d_land_n[p].swap(ln[p]); g.d_carry_n[p].swap(cn[p]);
    g.d_landc[p].swap(lc[p]); g.d_landc_n[p].swap(lcn[p]);
  }
  g.d_S.swap(S);
  g.d_O.swap(O);
  g.d_zoff.swap(d_off);
  g.d_zcap.swap(d_cap);
  g.zone_records = total;
  g.n_zones = nz;
  g.zcap_host = cap;
  // (the spill lists are re-sized by the callers, once nothing is left in
  // them: fixup_spill relays the zones while its spilled records wait there)
  return 0;
}

uint32_t required_words(uint32_t ht)
{
  switch(ht)
  {
    case GPU_ACTOR_HT_RING: return 4;
    case GPU_ACTOR_HT_PINGER: return 3;
    case GPU_ACTOR_HT_PINGER_DET: return 2;
    case GPU_ACTOR_HT_FANIN_SENDER: return 4;
    case GPU_ACTOR_HT_FANIN_ANALYZER: return 2;
    case GPU_ACTOR_HT_GUPS_STREAMER: return 2;
    case GPU_ACTOR_HT_GUPS_UPDATER: return 1;
    case GPU_ACTOR_HT_STORM: return 2;
    case GPU_ACTOR_HT_FIFO_SRC: return 3;
    case GPU_ACTOR_HT_FIFO_SINK: return 11;
    case GPU_ACTOR_HT_SPREADER: return 5;
    case GPU_ACTOR_HT_PROGRAM: return 8;
    case GPU_ACTOR_HT_HOST_PORT: return 1;
    default: return 0;
  }
}

// Sum the sharded per-step counters of k_step (EngDev::pend_sh / stats_sh)
// into pend[first, first + n) and stats[], and clear the shards. One block;
// stream-ordered behind the steps, so plain adds.
__global__ void __launch_bounds__(kBlock) k_fold(uint32_t first, uint32_t n)
{
  for(uint32_t s = first + threadIdx.x; s < first + n; s += kBlock)
  {
    unsigned long long* sh = c_eng.pend_sh + (size_t)s * kShards;
    unsigned long long v = 0;
    for(uint32_t k = 0; k < kShards; ++k) { v += sh[k]; sh[k] = 0; }
    if(v) c_eng.pend[s] += v;
  }
  for(uint32_t i = threadIdx.x; i < ST_COUNT; i += kBlock)
  {
    unsigned long long* sh = c_eng.stats_sh + (size_t)i * kShards;
    unsigned long long v = 0;
    for(uint32_t k = 0; k < kShards; ++k) { v += sh[k]; sh[k] = 0; }
    if(v) c_eng.stats[i] += v;
  }
}

// k_step's sharded counters folded into pend[first, first + n) and stats[]
// (n == 0: stats only), ahead of a host read of either.
int fold_counters(uint32_t first, uint32_t n)
{
  hipLaunchKernelGGL(k_fold, dim3(1), dim3(kBlock), 0, g.stream, first, n);
  HIPCK(hipGetLastError());
  return 0;
}

// Zero pend[first, first + n) and their shards.
int pend_clear(uint32_t first, uint32_t n)
{
  HIPCK(hipMemsetAsync(g.d_pend + first, 0, n * sizeof(unsigned long long), g.stream));
  HIPCK(hipMemsetAsync(g.d_pend_sh + (size_t)first * kShards, 0,
    (size_t)n * kShards * sizeof(unsigned long long), g.stream));
  return 0;
}

void sticky_from(const unsigned long long* st)
{
  if(st[ST_DROPPED] || st[ST_XCHG_OVERFLOW]) g.sticky = GPU_ACTOR_EMAILBOX;
  else if(st[ST_SEQ_OVERFLOW]) g.sticky = GPU_ACTOR_ERANGE;
}

int check_sticky()
{
  if(R() == 1 && g.sticky_epoch == g.dev_epoch) return g.sticky;   // nothing ran since
  unsigned long long st[ST_COUNT];
  {
    const int rc = fold_counters(0, 0);
    if(rc) return rc;
  }
  HIPCK(hipMemcpyAsync(st, g.d_stats, sizeof(st), hipMemcpyDeviceToHost, g.stream));
  HIPCK(hipStreamSynchronize(g.stream));
  g.sticky_epoch = g.dev_epoch;
  sticky_from(st);
  return g.sticky;
}

// Cross-rank exchange after a step (n_ranks > 1), with ONE synchronisation:
//   device: counts all-to-all, trigger count summed (RCCL), then one pinned
//   readback of send counts, receive counts, the trigger count, the exchange
//   spill count and the spill status; host: grow xout / xin if this step
//   needs more room (exchange_room: records past xcap were kept in the
//   exchange spill list and are placed now — nothing is dropped, as
//   messageq.c:31-59 drops nothing), then grouped ncclSend/ncclRecv of the
//   records over xGMI; device: k_xinject lands them; the trigger bytes are
//   merged when any actor triggers muting (or did last time on this parity);
//   a spill flag summed over ranks (k_spill_flag + allreduce, no readback)
//   lets every rank's next k_step halt alike when any zone overflowed.
// The host transport (gpu_actor_set_transport) does the same through its
// callbacks, with the records staged through pinned host memory.
// (a compact lane that needs the host counts like a spill list in use: EngDev::lc_over)
__global__ void k_spill_flag(unsigned int* flag)
{
  *flag = c_eng.spill_n[0] + c_eng.spill_n[1] + (c_eng.land8 ? *c_eng.lc_over : 0u);
}

// This rank's spill status as one number (zone spill lists, halt, and the
// summed flag of the last exchange): summed over ranks by pend_read, it is
// the same on every rank, so every rank decides alike whether to fix up.
// The GUPS streamers' chunks listed since the last launch (EngDev::gups_list,
// one rank): gups_parts lanes per chunk, 64 / gups_parts chunks per wave; lane
// p regenerates updates p * L + 1 .. (p + 1) * L of its chunk (L = gups_l)
// from state * x^(p * L) — one GF(2) product, PolyRand._seed's own jump
// (gups_basic/main.pony:182-216) — and XORs each into its updater's word
// (Updater.apply, main.pony:145-155). Per update instruction the wave combines
// the lanes that share the first (then the second) remaining lane's word into
// one atomic, and issues no atomic for an XOR of 0 (the identity: a stream
// _seed left at 0 repeats word 0 of updater 0). The last workgroup to finish
// empties the list.
__global__ void __launch_bounds__(256) k_gups_apply()
{
  // the segments' chunk counts, and their prefix: chunk e (in segment order)
  // is entry e - s_pre[s] of the segment s with s_pre[s] <= e < s_pre[s + 1]
  __shared__ uint32_t s_pre[kGupsShards + 1];
  if(threadIdx.x < kGupsShards)
  {
    uint32_t c = min(__atomic_load_n(&c_eng.gups_n[threadIdx.x], __ATOMIC_RELAXED), c_eng.gups_seg);
    for(int off = 1; off < (int)kGupsShards; off <<= 1)
    {
      const uint32_t o = __shfl_up(c, off);
      if((int)threadIdx.x >= off) c += o;
    }
    s_pre[threadIdx.x + 1] = c;
    if(threadIdx.x == 0) s_pre[0] = 0;
  }
  __syncthreads();
  const uint32_t n = s_pre[kGupsShards];
  const TypeDev& S = c_types[c_eng.gups_type];
  const uint64_t chunk = S.params[0], shift = S.params[1], mask = S.params[2];
  const uint32_t ubase = (uint32_t)S.params[3];
  const uint32_t L = c_eng.gups_l, parts = c_eng.gups_parts, per_wave = 64u / parts;
  const uint32_t lane = threadIdx.x & 63u, sub = lane / parts, p = lane - sub * parts;
  const uint64_t jump = c_eng.gups_jump[p];
  const uint64_t first = (uint64_t)p * L;
  const uint32_t cnt = first < chunk ? (uint32_t)min<uint64_t>(L, chunk - first) : 0u;
  const uint64_t wave = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const uint64_t waves = (uint64_t)gridDim.x * (blockDim.x >> 6);
  // the updater type last written (gups updaters are one type in practice)
  uint32_t u_first = 0, u_count = 0, u_lfirst = 0, u_lcount = 0;
  uint64_t* u_state = nullptr;
  uint64_t u_mask = 0;
  uint32_t made = 0, issued = 0;
  for(uint64_t e0 = wave * per_wave; e0 < n; e0 += waves * per_wave)
  {
    const uint64_t e = e0 + sub;
    const bool live = sub < per_wave && e < n;
    uint64_t v = 0;
    if(live)
    {
      uint32_t lo = 0, hi = kGupsShards;
      while(hi - lo > 1u)
      {
        const uint32_t mid = (lo + hi) >> 1;
        if(s_pre[mid] <= e) lo = mid; else hi = mid;
      }
      v = c_eng.gups_list[(size_t)lo * c_eng.gups_seg + (e - s_pre[lo])];
    }
    if(live && p) v = polyrand_mulmod(v, jump);
    for(uint32_t j = 0; j < L; ++j)
    {
      unsigned long long* w = nullptr;
      if(live && j < cnt)
      {
        (void)polyrand_next(v);
        ++made;
        const uint32_t to = ubase + (uint32_t)((v >> shift) & mask);
        if(to - u_first >= u_count)
        {
          const int t = type_of_global(to);
          if(t >= 0)
          {
            const TypeDev& U = c_types[t];
            u_first = U.first; u_count = U.count; u_lfirst = U.lfirst; u_lcount = U.lcount;
            u_state = U.state; u_mask = U.params[0] - 1;
          }
        }
        if(to - u_first < u_count)
          w = reinterpret_cast<unsigned long long*>(&u_state[(v & u_mask) * u_lcount + (to - u_lfirst)]);
      }
      // the wave's update instruction: up to two combined words, then the rest
      const uint64_t wa = reinterpret_cast<uint64_t>(w);
      uint64_t left = __ballot(w != nullptr);
      for(int round = 0; round < 2 && left; ++round)
      {
        const uint32_t lead = (uint32_t)__ffsll((long long)left) - 1u;
        const uint64_t lw = __shfl(wa, (int)lead);
        const uint64_t peers = __ballot(((left >> lane) & 1ull) && wa == lw);
        uint64_t r = ((peers >> lane) & 1ull) ? v : 0ull;
        if(__popcll(peers) > 1)
          for(int off = 32; off; off >>= 1) r ^= __shfl_xor(r, off);
        if(lane == lead && r != 0)
        {
          atomicXor(w, (unsigned long long)r);
          ++issued;
        }
        left &= ~peers;
      }
      if(((left >> lane) & 1ull) && v != 0)
      {
        atomicXor(w, (unsigned long long)v);
        ++issued;
      }
    }
  }
  // per workgroup: updates made, atomics issued (each slot written by its own
  // workgroup only, summed by the host)
  __shared__ uint32_t s_sum[2];
  if(threadIdx.x < 2) s_sum[threadIdx.x] = 0;
  __syncthreads();
  if(made) atomicAdd(&s_sum[0], made);
  if(issued) atomicAdd(&s_sum[1], issued);
  __syncthreads();
  if(threadIdx.x == 0)
  {
    c_eng.gups_stat[blockIdx.x] += s_sum[0];
    c_eng.gups_stat[kGupsBlocks + blockIdx.x] += s_sum[1];
    __threadfence();
    const unsigned int done = atomicAdd(&c_eng.gups_n[kGupsShards], 1u);
    if(done == gridDim.x - 1u)
      for(uint32_t s = 0; s <= kGupsShards; ++s) atomicExch(&c_eng.gups_n[s], 0u);
  }
}

// n_ranks > 1: the chunks this rank's streamers listed in the step, packed in
// segment order to out[0 .. *count) — the run every peer receives — with the
// prefix k_gups_apply builds. The last workgroup to finish empties the list.
__global__ void __launch_bounds__(256) k_gups_pack(uint64_t* out, unsigned long long* count)
{
  __shared__ uint32_t s_pre[kGupsShards + 1];
  if(threadIdx.x < kGupsShards)
  {
    uint32_t c = min(__atomic_load_n(&c_eng.gups_n[threadIdx.x], __ATOMIC_RELAXED), c_eng.gups_seg);
    for(int off = 1; off < (int)kGupsShards; off <<= 1)
    {
      const uint32_t o = __shfl_up(c, off);
      if((int)threadIdx.x >= off) c += o;
    }
    s_pre[threadIdx.x + 1] = c;
    if(threadIdx.x == 0) s_pre[0] = 0;
  }
  __syncthreads();
  const uint32_t n = s_pre[kGupsShards];
  for(uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n;
      e += (uint64_t)gridDim.x * blockDim.x)
  {
    uint32_t lo = 0, hi = kGupsShards;
    while(hi - lo > 1u)
    {
      const uint32_t mid = (lo + hi) >> 1;
      if(s_pre[mid] <= e) lo = mid; else hi = mid;
    }
    out[e] = c_eng.gups_list[(size_t)lo * c_eng.gups_seg + (e - s_pre[lo])];
  }
  if(threadIdx.x == 0)
  {
    if(blockIdx.x == 0) *count = n;
    const unsigned int done = atomicAdd(&c_eng.gups_n[kGupsShards], 1u);
    if(done == gridDim.x - 1u)
      for(uint32_t s = 0; s <= kGupsShards; ++s) atomicExch(&c_eng.gups_n[s], 0u);
  }
}

// k_gups_apply for n_ranks > 1: list[0 .. n) holds every rank's chunks of the
// step in rank order (gups_gather_apply), this rank's own at [own_lo, own_lo +
// own_n). Every rank regenerates every chunk, lane p from state * x^(p * L) as
// above, and keeps the updates whose updater it owns (is_remote), addressed
// through the owner-local slot; the wave's same-word combine and the skipped
// XOR of 0 are k_gups_apply's. gups_stat counts the kept updates, their
// atomics, and (third row) the kept updates of peers' chunks: the updates a
// record per update would have carried across ranks.
__global__ void __launch_bounds__(256) k_gups_apply_ranks(const uint64_t* list, uint64_t n,
  uint64_t own_lo, uint64_t own_n)
{
  const TypeDev& S = c_types[c_eng.gups_type];
  const uint64_t chunk = S.params[0], shift = S.params[1], mask = S.params[2];
  const uint32_t ubase = (uint32_t)S.params[3];
  const uint32_t L = c_eng.gups_l, parts = c_eng.gups_parts, per_wave = 64u / parts;
  const uint32_t lane = threadIdx.x & 63u, sub = lane / parts, p = lane - sub * parts;
  const uint64_t jump = c_eng.gups_jump[p];
  const uint64_t first = (uint64_t)p * L;
  const uint32_t cnt = first < chunk ? (uint32_t)min<uint64_t>(L, chunk - first) : 0u;
  const uint64_t wave = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const uint64_t waves = (uint64_t)gridDim.x * (blockDim.x >> 6);
  uint32_t u_first = 0, u_count = 0, u_lfirst = 0, u_lcount = 0;
  uint64_t* u_state = nullptr;
  uint64_t u_mask = 0;
  uint32_t made = 0, issued = 0, far = 0;
  for(uint64_t e0 = wave * per_wave; e0 < n; e0 += waves * per_wave)
  {
    const uint64_t e = e0 + sub;
    const bool live = sub < per_wave && e < n;
    const uint32_t peer = e - own_lo >= own_n ? 1u : 0u;
    uint64_t v = live ? list[e] : 0ull;
    if(live && p) v = polyrand_mulmod(v, jump);
    for(uint32_t j = 0; j < L; ++j)
    {
      unsigned long long* w = nullptr;
      if(live && j < cnt)
      {
        (void)polyrand_next(v);
        const uint32_t to = ubase + (uint32_t)((v >> shift) & mask);
        if(!is_remote(to))
        {
          ++made;
          far += peer;
          if(to - u_first >= u_count)
          {
            const int t = type_of_global(to);
            if(t >= 0)
            {
              const TypeDev& U = c_types[t];
              u_first = U.first; u_count = U.count; u_lfirst = U.lfirst; u_lcount = U.lcount;
              u_state = U.state; u_mask = U.params[0] - 1;
            }
          }
          if(to - u_first < u_count)
            w = reinterpret_cast<unsigned long long*>(
              &u_state[(v & u_mask) * u_lcount + (slot_of(to) - u_lfirst)]);
        }
      }
      const uint64_t wa = reinterpret_cast<uint64_t>(w);
      uint64_t left = __ballot(w != nullptr);
      for(int round = 0; round < 2 && left; ++round)
      {
        const uint32_t lead = (uint32_t)__ffsll((long long)left) - 1u;
        const uint64_t lw = __shfl(wa, (int)lead);
        const uint64_t peers = __ballot(((left >> lane) & 1ull) && wa == lw);
        uint64_t r = ((peers >> lane) & 1ull) ? v : 0ull;
        if(__popcll(peers) > 1)
          for(int off = 32; off; off >>= 1) r ^= __shfl_xor(r, off);
        if(lane == lead && r != 0)
        {
          atomicXor(w, (unsigned long long)r);
          ++issued;
        }
        left &= ~peers;
      }
      if(((left >> lane) & 1ull) && v != 0)
      {
        atomicXor(w, (unsigned long long)v);
        ++issued;
      }
    }
  }
  __shared__ uint32_t s_sum[3];
  if(threadIdx.x < 3) s_sum[threadIdx.x] = 0;
  __syncthreads();
  if(made) atomicAdd(&s_sum[0], made);
  if(issued) atomicAdd(&s_sum[1], issued);
  if(far) atomicAdd(&s_sum[2], far);
  __syncthreads();
  if(threadIdx.x == 0)
  {
    c_eng.gups_stat[blockIdx.x] += s_sum[0];
    c_eng.gups_stat[kGupsBlocks + blockIdx.x] += s_sum[1];
    c_eng.gups_stat[2 * kGupsBlocks + blockIdx.x] += s_sum[2];
  }
}

__global__ void k_spill_local(unsigned long long* out)
{
  *out = (unsigned long long)c_eng.spill_n[0] + c_eng.spill_n[1] + *c_eng.halt +
         (c_eng.land8 ? *c_eng.lc_over : 0u) + (c_eng.nranks > 1 ? *c_eng.spill_flag : 0u);
}

// Only when the exchange spill list itself overflowed (records were lost and
// counted): send what xout holds, and count the kept spill records as lost too.
__global__ void k_xprep()
{
  const unsigned int xs = *c_eng.xspill_n;
  if(xs <= c_eng.xspill_cap) return;
  const uint32_t p = threadIdx.x;
  if(p < c_eng.nranks)
    c_eng.xcount[p] = min(c_eng.xcount[p], (unsigned long long)c_eng.xcap);
  if(p == 0) atomicAdd(&c_eng.stats[ST_XCHG_OVERFLOW], (unsigned long long)c_eng.xspill_cap);
}

__global__ void __launch_bounds__(kBlock) k_xspill_place(uint32_t n)
{
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if(i >= n) return;
  const XSpillRec r = c_eng.xspill[i];
  xrec_put(c_eng.xdst[r.peer] + r.pos, r.rec);
}

int alloc_xspill(uint32_t cap)
{
  g.xspill_cap = 0;
  HIPCK(g.d_xspill.alloc(cap));
  g.xspill_cap = cap;
  return 0;
}

// Room for this step's exchange: max_send records to one peer, total_recv
// records from all peers, xs records kept in the exchange spill list. xout's
// peer segments grow (kept records are copied to the new stride) and the
// spilled records go to their reserved positions; xin grows. Local decisions
// only: each side sizes its own buffers.
int peer_room(uint64_t max_send, uint64_t xs);
int exchange_room(uint64_t max_send, uint64_t total_recv, uint64_t xs)
{
  if(g.peer_write) return peer_room(max_send, xs);
  const bool lost = xs > g.xspill_cap;     // k_xprep clipped the counts to xcap
  if(max_send > g.xcap || lost)
  {
    uint64_t cap = std::max<uint64_t>(2ull * g.xcap, max_send + max_send / 2);
    cap = std::min<uint64_t>((cap + 63) & ~63ull, 0x40000000ull);
    DevBuf<XRec> nx;
    HIPCK(nx.alloc((size_t)R() * cap));
    HIPCK(hipMemcpy2DAsync(nx, cap * sizeof(XRec), g.d_xout, (size_t)g.xcap * sizeof(XRec),
      (size_t)g.xcap * sizeof(XRec), R(), hipMemcpyDeviceToDevice, g.stream));
    HIPCK(hipStreamSynchronize(g.stream));
    g.d_xout = std::move(nx);
    g.xcap = (uint32_t)cap;
    const int rc = upload_types();
    if(rc) return rc;
  }
  if(xs)
  {
    if(!lost)
    {
      hipLaunchKernelGGL(k_xspill_place, dim3(blocks_for(xs)), dim3(kBlock), 0, g.stream,
        (uint32_t)xs);
      HIPCK(hipGetLastError());
    }
    HIPCK(hipMemsetAsync(g.d_xspill_n, 0, sizeof(unsigned int), g.stream));
    if(xs > g.xspill_cap / 2)
    {
      // a burst this large may come again: keep room for twice as much
      HIPCK(hipStreamSynchronize(g.stream));
      const int rc = alloc_xspill((uint32_t)std::min<uint64_t>(4ull * std::max<uint64_t>(xs,
        g.xspill_cap), 1ull << 27));
      if(rc) return rc;
      const int rc2 = upload_types();
      if(rc2) return rc2;
    }
  }
  if(total_recv > g.d_xin.size())
  {
    const uint64_t cap = std::max<uint64_t>(2ull * g.d_xin.size(), total_recv + total_recv / 2);
    HIPCK(hipStreamSynchronize(g.stream));
    HIPCK(g.d_xin.alloc(cap));
  }
  return 0;
}

// ---- cross-rank collectives on device buffers ---------------------
// Every cross-rank step of the engine — the exchange's counts and records,
// the trigger-byte and spill-flag merges, the spawn gather, the pending and
// counter sums — calls only these four, on device buffers in stream order.
// Each has two implementations: RCCL on the engine's stream (ncclAllReduce /
// ncclAllToAll / ncclAllGather / grouped ncclSend+ncclRecv over xGMI), and
// the host transport (gpu_actor_set_transport: the same device buffers
// staged through pinned host memory and the two callbacks). The control flow
// around them is one path, so the host-transport tests run it all; only the
// nccl* calls inside these functions are left to the RCCL runs.
enum XcType { XC_U8 = 0, XC_U32 = 1, XC_U64 = 2 };

int stage_room(uint64_t sbytes, uint64_t rbytes)
{
  if(sbytes > g.h_sbuf.size()) HIPCK(g.h_sbuf.alloc(std::max<uint64_t>(sbytes, 2 * g.h_sbuf.size())));
  if(rbytes > g.h_rbuf.size()) HIPCK(g.h_rbuf.alloc(std::max<uint64_t>(rbytes, 2 * g.h_rbuf.size())));
  return 0;
}

// d_out[i] = Σ over ranks of d_in[i], i < count (in place when d_in == d_out).
// XC_U8 on the host transport sums 8 bytes per word: every byte must have
// one nonzero contributor (the trigger bytes: each rank writes its own ids).
int xc_allreduce_sum(const void* d_in, void* d_out, uint64_t count, XcType t)
{
  if(count == 0) return 0;
  if(!gp.xp_ar)
  {
    const ncclDataType_t nt = t == XC_U8 ? ncclUint8 : t == XC_U32 ? ncclUint32 : ncclUint64;
    NCCLCK(ncclAllReduce(d_in, d_out, count, nt, ncclSum, g.comm, g.stream));
    return 0;
  }
  const uint64_t esz = t == XC_U8 ? 1 : t == XC_U32 ? 4 : 8;
  const uint64_t bytes = count * esz;
  const uint64_t words = t == XC_U64 ? count : t == XC_U8 ? (bytes + 7) / 8 : count;
  int rc = stage_room(words * 8, bytes);
  if(rc) return rc;
  uint64_t* w = reinterpret_cast<uint64_t*>(g.h_sbuf.get());
  if(t == XC_U8) memset(w, 0, words * 8);
  HIPCK(hipMemcpyAsync(t == XC_U32 ? g.h_rbuf : g.h_sbuf, d_in, bytes, hipMemcpyDeviceToHost,
    g.stream));
  HIPCK(hipStreamSynchronize(g.stream));
  if(t == XC_U32)
    for(uint64_t i = 0; i < count; ++i) w[i] = reinterpret_cast<const uint32_t*>(g.h_rbuf.get())[i];
  if(gp.xp_ar(gp.xp_ctx, w, words) != 0) return GPU_ACTOR_ECOMM;
  if(t == XC_U32)
  {
    for(uint64_t i = 0; i < count; ++i)
      reinterpret_cast<uint32_t*>(g.h_rbuf.get())[i] = (uint32_t)std::min<uint64_t>(w[i], 0xFFFFFFFFull);
    HIPCK(hipMemcpyAsync(d_out, g.h_rbuf, bytes, hipMemcpyHostToDevice, g.stream));
  }
  else
    HIPCK(hipMemcpyAsync(d_out, g.h_sbuf, bytes, hipMemcpyHostToDevice, g.stream));
  HIPCK(hipStreamSynchronize(g.stream));       // the staging is reused by the next call
  return 0;
}

// d_recv[p] = peer p's d_send[rank] (one u64 per peer).
int xc_alltoall_u64(const unsigned long long* d_send, unsigned long long* d_recv)
{
  const uint32_t n = R();
  if(!gp.xp_a2a)
  {
    NCCLCK(ncclAllToAll(d_send, d_recv, 1, ncclUint64, g.comm, g.stream));
    return 0;
  }
  int rc = stage_room(n * 8, n * 8);
  if(rc) return rc;
  HIPCK(hipMemcpyAsync(g.h_sbuf, d_send, n * 8, hipMemcpyDeviceToHost, g.stream));
  HIPCK(hipStreamSynchronize(g.stream));
  std::vector<uint64_t> b8(n, 8);
  if(gp.xp_a2a(gp.xp_ctx, g.h_sbuf, b8.data(), g.h_rbuf, b8.data()) != 0) return GPU_ACTOR_ECOMM;
  HIPCK(hipMemcpyAsync(d_recv, g.h_rbuf, n * 8, hipMemcpyHostToDevice, g.stream));
  HIPCK(hipStreamSynchronize(g.stream));
  return 0;
}

// d_out[p] = rank p's d_in[0] (one u64 per rank).
int xc_allgather_u64(const unsigned long long* d_in, unsigned long long* d_out)
{
  const uint32_t n = R();
  if(!gp.xp_a2a)
  {
    NCCLCK(ncclAllGather(d_in, d_out, 1, ncclUint64, g.comm, g.stream));
    return 0;
  }
  int rc = stage_room(n * 8, n * 8);
  if(rc) return rc;
  HIPCK(hipMemcpyAsync(g.h_sbuf, d_in, 8, hipMemcpyDeviceToHost, g.stream));
  HIPCK(hipStreamSynchronize(g.stream));
  uint64_t* sw = reinterpret_cast<uint64_t*>(g.h_sbuf.get());
  for(uint32_t p = 1; p < n; ++p) sw[p] = sw[0];
  std::vector<uint64_t> b8(n, 8);
  if(gp.xp_a2a(gp.xp_ctx, g.h_sbuf, b8.data(), g.h_rbuf, b8.data()) != 0) return GPU_ACTOR_ECOMM;
  HIPCK(hipMemcpyAsync(d_out, g.h_rbuf, n * 8, hipMemcpyHostToDevice, g.stream));
  HIPCK(hipStreamSynchronize(g.stream));
  return 0;
}

// One grouped exchange: to each peer p != rank, send[p] bytes from d_send[p];
// from it, recv[p] bytes into d_recv[p] (either may be 0).
struct XcPeer {
  const void* d_send = nullptr;
  uint64_t send = 0;
  void* d_recv = nullptr;
  uint64_t recv = 0;
};
int xc_sendrecv(const std::vector<XcPeer>& pp)
{
  const uint32_t n = R();
  if(!gp.xp_a2a)
  {
    NCCLCK(ncclGroupStart());
    for(uint32_t p = 0; p < n; ++p)
    {
      if(p == rank()) continue;
      if(pp[p].send) NCCLCK(ncclSend(pp[p].d_send, pp[p].send, ncclUint8, p, g.comm, g.stream));
      if(pp[p].recv) NCCLCK(ncclRecv(pp[p].d_recv, pp[p].recv, ncclUint8, p, g.comm, g.stream));
    }
    NCCLCK(ncclGroupEnd());
    return 0;
  }
  std::vector<uint64_t> sb(n, 0), rb(n, 0);
  uint64_t st = 0, rt = 0;
  for(uint32_t p = 0; p < n; ++p)
  {
    if(p == rank()) continue;
    sb[p] = pp[p].send;
    rb[p] = pp[p].recv;
    st += sb[p];
    rt += rb[p];
  }
  int rc = stage_room(std::max<uint64_t>(st, 8), std::max<uint64_t>(rt, 8));
  if(rc) return rc;
  uint64_t off = 0;
  for(uint32_t p = 0; p < n; ++p)
  {
    if(sb[p]) HIPCK(hipMemcpyAsync(g.h_sbuf + off, pp[p].d_send, sb[p], hipMemcpyDeviceToHost, g.stream));
    off += sb[p];
  }
  HIPCK(hipStreamSynchronize(g.stream));
  if(gp.xp_a2a(gp.xp_ctx, g.h_sbuf, sb.data(), g.h_rbuf, rb.data()) != 0) return GPU_ACTOR_ECOMM;
  off = 0;
  for(uint32_t p = 0; p < n; ++p)
  {
    if(rb[p]) HIPCK(hipMemcpyAsync(pp[p].d_recv, g.h_rbuf + off, rb[p], hipMemcpyHostToDevice, g.stream));
    off += rb[p];
  }
  HIPCK(hipStreamSynchronize(g.stream));
  return 0;
}

// Trigger bytes in use: a rank writes the bytes of its own actors' global ids
// (global_of of its local slots below n_local), all below n_actors under any
// placement (the same count on every rank, as the merge needs).
uint64_t trig_live_bytes()
{
  return std::min<uint64_t>(g.trig_bytes, (g.n_actors + 7) & ~7ull);
}

// Peer writes: map every peer's inbox (hipIpcGetMemHandle / hipIpcOpenMemHandle),
// the handles gathered word by word over the engine's collectives (RCCL or the
// host transport). Collective: every rank calls it at the same point.
void peer_close()
{
  for(uint32_t p = 0; p < kMaxRanks; ++p)
  {
    if(g.peer_ptr[p] && p != rank()) (void)hipIpcCloseMemHandle(g.peer_ptr[p]);
    g.peer_ptr[p] = nullptr;
  }
}

int peer_open()
{
  hipIpcMemHandle_t h;
  HIPCK(hipIpcGetMemHandle(&h, g.d_pin));
  static_assert(sizeof(hipIpcMemHandle_t) % 8 == 0, "IPC handle in u64 words");
  constexpr uint32_t kW = sizeof(hipIpcMemHandle_t) / 8;
  const uint32_t n = R();
  std::vector<unsigned long long> all((size_t)kW * n), got(n);
  for(uint32_t w = 0; w < kW; ++w)
  {
    unsigned long long v;
    memcpy(&v, reinterpret_cast<const char*>(&h) + 8 * w, 8);
    HIPCK(hipMemcpyAsync(g.d_hx, &v, 8, hipMemcpyHostToDevice, g.stream));
    HIPCK(hipStreamSynchronize(g.stream));
    const int rc = xc_allgather_u64(g.d_hx, g.d_hx + 1);
    if(rc) return rc;
    HIPCK(hipMemcpyAsync(got.data(), g.d_hx + 1, n * 8, hipMemcpyDeviceToHost, g.stream));
    HIPCK(hipStreamSynchronize(g.stream));
    for(uint32_t p = 0; p < n; ++p) all[(size_t)p * kW + w] = got[p];
  }
  for(uint32_t p = 0; p < n; ++p)
  {
    if(p == rank())
    {
      g.peer_ptr[p] = g.d_pin;
      continue;
    }
    hipIpcMemHandle_t hp;
    memcpy(&hp, &all[(size_t)p * kW], sizeof(hp));
    void* ptr = nullptr;
    HIPCK(hipIpcOpenMemHandle(&ptr, hp, hipIpcMemLazyEnablePeerAccess));
    g.peer_ptr[p] = static_cast<XRec*>(ptr);
  }
  return 0;
}

// exchange_room with peer writes: a segment lives in its receiver's inbox, so
// the segments grow on every rank alike — to the largest size any rank needs
// (one gather of each rank's need and whether it kept records in its exchange
// spill list), the kept records moved to the new stride by each inbox's owner,
// the inboxes mapped again; then the spilled records go to their peers, and
// when any rank placed some, one more collective orders those stores before
// every owner's k_xinject.
int peer_room(uint64_t max_send, uint64_t xs)
{
  const bool lost = xs > g.xspill_cap;     // k_xprep clipped the counts to xcap
  uint64_t want = 0;
  if(max_send > g.xcap || lost)
  {
    want = std::max<uint64_t>(2ull * g.xcap, max_send + max_send / 2);
    want = std::min<uint64_t>((want + 63) & ~63ull, 0x40000000ull);
  }
  const uint32_t n = R();
  const unsigned long long mine = want << 1 | (xs ? 1ull : 0ull);
  HIPCK(hipMemcpyAsync(g.d_hx, &mine, 8, hipMemcpyHostToDevice, g.stream));
  HIPCK(hipStreamSynchronize(g.stream));
  int rc = xc_allgather_u64(g.d_hx, g.d_hx + 1);
  if(rc) return rc;
  std::vector<unsigned long long> all(n);
  HIPCK(hipMemcpyAsync(all.data(), g.d_hx + 1, n * 8, hipMemcpyDeviceToHost, g.stream));
  HIPCK(hipStreamSynchronize(g.stream));
  uint64_t cap = g.xcap;
  bool any_xs = false;
  for(uint32_t p = 0; p < n; ++p)
  {
    cap = std::max<uint64_t>(cap, all[p] >> 1);
    any_xs |= (all[p] & 1ull) != 0;
  }
  if(cap > g.xcap)
  {
    DevBuf<XRec> nx;
    HIPCK(nx.alloc((size_t)n * cap));
    HIPCK(hipMemcpy2DAsync(nx, cap * sizeof(XRec), g.d_pin, (size_t)g.xcap * sizeof(XRec),
      (size_t)g.xcap * sizeof(XRec), n, hipMemcpyDeviceToDevice, g.stream));
    HIPCK(hipStreamSynchronize(g.stream));
    peer_close();
    g.d_pin = std::move(nx);
    g.xcap = (uint32_t)cap;
    rc = peer_open();
    if(rc) return rc;
    rc = upload_types();
    if(rc) return rc;
  }
  if(xs)
  {
    if(!lost)
    {
      hipLaunchKernelGGL(k_xspill_place, dim3(blocks_for(xs)), dim3(kBlock), 0, g.stream,
        (uint32_t)xs);
      HIPCK(hipGetLastError());
    }
    HIPCK(hipMemsetAsync(g.d_xspill_n, 0, sizeof(unsigned int), g.stream));
    if(xs > g.xspill_cap / 2)
    {
      HIPCK(hipStreamSynchronize(g.stream));
      rc = alloc_xspill((uint32_t)std::min<uint64_t>(4ull * std::max<uint64_t>(xs, g.xspill_cap),
        1ull << 27));
      if(rc) return rc;
      rc = upload_types();
      if(rc) return rc;
    }
  }
  if(any_xs)
  {
    rc = xc_allreduce_sum(g.d_hx, g.d_hx, 1, XC_U64);
    if(rc) return rc;
  }
  return 0;
}

int exchange_step(uint32_t step_sidx)
{
  const uint32_t n = R(), land_par = g.par, tslot = (step_sidx + 1) % 3;
  unsigned int tcount = 0;
  uint64_t total = 0;
  hipLaunchKernelGGL(k_xprep, dim3(1), dim3(64), 0, g.stream);
  HIPCK(hipGetLastError());
  // send counts to every peer (device), the step's trigger count summed
  int rc = xc_alltoall_u64(g.d_xcount, g.d_xrecv);
  if(rc) return rc;
  rc = xc_allreduce_sum(g.d_trig_n + tslot, g.d_trig_n + tslot, 1, XC_U32);
  if(rc) return rc;
  // the GUPS chunks listed in the step, packed, and every rank's count of
  // them (the chunks themselves move after the halt check: gups_gather_apply)
  if(g.gups_type >= 0)
  {
    hipLaunchKernelGGL(k_gups_pack, dim3(kGupsPackBlocks), dim3(256), 0, g.stream, g.d_gups_send,
      g.d_xc + 2 * n + 2);
    HIPCK(hipGetLastError());
    rc = xc_allgather_u64(g.d_xc + 2 * n + 2, g.d_xc + 2 * n + 3);
    if(rc) return rc;
    HIPCK(hipMemcpyAsync(g.h_xc + 2 * n + 2, g.d_xc + 2 * n + 2, (n + 1) * sizeof(unsigned long long),
      hipMemcpyDeviceToHost, g.stream));
  }
  // the step's one readback: send and receive counts, trigger count, kept
  // exchange-spill records, spill status, GUPS chunk counts
  g.h_xc[2 * n] = 0;
  g.h_xc[2 * n + 1] = 0;
  HIPCK(hipMemcpyAsync(g.h_xc, g.d_xc, 2 * n * sizeof(unsigned long long), hipMemcpyDeviceToHost,
    g.stream));
  HIPCK(hipMemcpyAsync(g.h_xc + 2 * n, g.d_trig_n + tslot, sizeof(unsigned int),
    hipMemcpyDeviceToHost, g.stream));
  HIPCK(hipMemcpyAsync(g.h_xc + 2 * n + 1, g.d_xspill_n, sizeof(unsigned int),
    hipMemcpyDeviceToHost, g.stream));
  HIPCK(hipMemcpyAsync(g.h_sstat, g.d_sstat, sizeof(SpillStat), hipMemcpyDeviceToHost,
    g.stream));
  HIPCK(hipStreamSynchronize(g.stream));
  tcount = (unsigned int)(g.h_xc[2 * n] & 0xFFFFFFFFull);
  const uint64_t xs = g.h_xc[2 * n + 1] & 0xFFFFFFFFull;
  std::vector<uint64_t> roff(n);
  uint64_t max_send = 0;
  for(uint32_t p = 0; p < n; ++p)
  {
    roff[p] = total;
    if(p == rank()) continue;
    total += g.h_xc[n + p];
    max_send = std::max<uint64_t>(max_send, g.h_xc[p]);
  }
  rc = exchange_room(max_send, total, xs);
  if(rc) return rc;
  // the records: each peer's segment of xout to it, its records into xin in
  // rank order (k_xinject tells the sender of a record by its segment)
  // (with peer writes they are in this rank's inbox already: every peer's
  // k_step stored them there before its counts went out)
  if(!g.peer_write)
  {
    std::vector<XcPeer> pp(n);
    for(uint32_t p = 0; p < n; ++p)
    {
      if(p == rank()) continue;
      pp[p].d_send = g.d_xout + (size_t)p * g.xcap;
      pp[p].send = g.h_xc[p] * sizeof(XRec);
      pp[p].d_recv = g.d_xin + roff[p];
      pp[p].recv = g.h_xc[n + p] * sizeof(XRec);
    }
    rc = xc_sendrecv(pp);
    if(rc) return rc;
  }
  g.remote_total += total;
  if(total)
  {
    hipLaunchKernelGGL(k_xinject, dim3(blocks_for(total, kLandRecs)), dim3(kLandThreads), 0, g.stream,
      (const XRec*)(g.peer_write ? g.d_pin : g.d_xin), total, land_par,
      (const unsigned long long*)g.d_xrecv, g.peer_write ? (uint64_t)g.xcap : 0ull);
    HIPCK(hipGetLastError());
  }
  HIPCK(hipMemsetAsync(g.d_xcount, 0, n * sizeof(unsigned long long), g.stream));
  // trigger bytes of parity land_par: every rank's own bytes summed (each
  // byte has one writer, so the sum is the merge), over the ids in use only
  if(tcount || g.trig_stale[land_par])
  {
    rc = xc_allreduce_sum(g.d_trig_own[land_par], g.d_trig[land_par], trig_live_bytes(), XC_U8);
    if(rc) return rc;
  }
  g.trig_stale[land_par] = tcount != 0;
  // did any rank's zone overflow (this step or its landing)? summed on device
  hipLaunchKernelGGL(k_spill_flag, dim3(1), dim3(1), 0, g.stream, g.d_spill_flag);
  HIPCK(hipGetLastError());
  return xc_allreduce_sum(g.d_spill_flag, g.d_spill_flag, 1, XC_U32);
}

// Ids and landing for the actors the last step's behaviours created: the
// records are sorted by (type, creator, seq) — the canonical order — and
// numbered after each type's live actors (k_spawn_*). One small readback per
// step, only for engines with a reserve. With n_ranks > 1 every rank gathers
// every rank's records (count allgather, then grouped send/recv, or the host
// transport), sorts the same list, numbers alike, and lands the constructor
// messages of the actors it owns (owner = id % n_ranks): the ids equal a
// single rank's (pony_create inside behaviours is rank-agnostic,
// actor.c:688-734).
// hipcub's scratch for the sorts of spawn_process and host_collect
hipError_t sort_room(size_t bytes)
{
  return bytes > g.d_sort_tmp.size() ? g.d_sort_tmp.alloc(bytes) : hipSuccess;
}

int spawn_process(uint32_t cur)
{
  unsigned int n = 0;
  HIPCK(hipMemcpyAsync(&n, g.d_spawn_n, sizeof(n), hipMemcpyDeviceToHost, g.stream));
  HIPCK(hipStreamSynchronize(g.stream));
  n = std::min(n, g.spawn_cap);
  uint64_t* key = g.d_skey[0];
  uint64_t* arg = g.d_sarg[0];
  uint32_t total = n;
  if(R() > 1)
  {
    const uint32_t nr = R();
    std::vector<uint64_t> cnt(nr, 0);
    {
      unsigned long long* dc = g.d_xc + 2 * nr;     // scratch words of the counts block
      const unsigned long long mine = n;
      HIPCK(hipMemcpyAsync(dc, &mine, sizeof(mine), hipMemcpyHostToDevice, g.stream));
      DevBuf<unsigned long long> dall;
      HIPCK(dall.alloc(nr));
      int rc = xc_allgather_u64(dc, dall);
      if(rc) return rc;
      HIPCK(hipMemcpyAsync(cnt.data(), dall, nr * sizeof(uint64_t), hipMemcpyDeviceToHost, g.stream));
      HIPCK(hipStreamSynchronize(g.stream));
    }
    // every rank's whole list, in rank order (each list holds at most
    // spawn_cap records; past that its own device counted the drops): the
    // reserve is applied per type after the canonical sort (k_spawn_land), so
    // which spawns get ids never depends on the rank layout
    std::vector<uint64_t> off(nr);
    uint64_t acc = 0;
    for(uint32_t p = 0; p < nr; ++p)
    {
      cnt[p] = std::min<uint64_t>(cnt[p], g.spawn_cap);
      off[p] = acc;
      acc += cnt[p];
    }
    if(acc > 0x7FFFFFFFull) return GPU_ACTOR_ERANGE;
    total = (uint32_t)acc;
    if(total == 0) return 0;
    n = (uint32_t)cnt[rank()];
    // gathered into [1], local records first copied to their own slot
    if(n)
    {
      HIPCK(hipMemcpyAsync(g.d_skey[1] + off[rank()], g.d_skey[0], n * sizeof(uint64_t),
        hipMemcpyDeviceToDevice, g.stream));
      HIPCK(hipMemcpyAsync(g.d_sarg[1] + off[rank()], g.d_sarg[0], n * sizeof(uint64_t),
        hipMemcpyDeviceToDevice, g.stream));
    }
    // every peer gets our n records; we get each peer's (keys, then args)
    for(int part = 0; part < 2; ++part)
    {
      uint64_t* mine_d = part ? g.d_sarg[0] : g.d_skey[0];
      uint64_t* all_d = part ? g.d_sarg[1] : g.d_skey[1];
      std::vector<XcPeer> pp(nr);
      for(uint32_t p = 0; p < nr; ++p)
      {
        if(p == rank()) continue;
        pp[p].d_send = mine_d;
        pp[p].send = (uint64_t)n * sizeof(uint64_t);
        pp[p].d_recv = all_d + off[p];
        pp[p].recv = cnt[p] * sizeof(uint64_t);
      }
      const int rc = xc_sendrecv(pp);
      if(rc) return rc;
    }
    // sort input: the gathered list
    HIPCK(hipMemcpyAsync(g.d_skey[0], g.d_skey[1], total * sizeof(uint64_t),
      hipMemcpyDeviceToDevice, g.stream));
    HIPCK(hipMemcpyAsync(g.d_sarg[0], g.d_sarg[1], total * sizeof(uint64_t),
      hipMemcpyDeviceToDevice, g.stream));
  }
  if(total == 0) return 0;
  size_t need = 0;
  uint64_t *key_out = g.d_skey[1], *arg_out = g.d_sarg[1];
  HIPCK(hipcub::DeviceRadixSort::SortPairs(nullptr, need, key, key_out, arg, arg_out, (int)total, 0, 56,
    g.stream));
  HIPCK(sort_room(need));
  HIPCK(hipcub::DeviceRadixSort::SortPairs(g.d_sort_tmp, need, key, key_out, arg, arg_out, (int)total, 0,
    56, g.stream));
  HIPCK(hipMemsetAsync(g.d_tstart, 0xFF, GPU_ACTOR_MAX_TYPES * sizeof(uint32_t), g.stream));
  HIPCK(hipMemsetAsync(g.d_tcnt, 0, GPU_ACTOR_MAX_TYPES * sizeof(uint32_t), g.stream));
  hipLaunchKernelGGL(k_spawn_scan, dim3(blocks_for(total)), dim3(kBlock), 0, g.stream,
    (const uint64_t*)g.d_skey[1], total, g.d_tstart, g.d_tcnt);
  hipLaunchKernelGGL(k_spawn_land, dim3(blocks_for(total, kLandRecs)), dim3(kLandThreads), 0,
    g.stream, (const uint64_t*)g.d_skey[1], (const uint64_t*)g.d_sarg[1], total,
    (const uint32_t*)g.d_tstart, (const unsigned long long*)g.d_live, cur);
  hipLaunchKernelGGL(k_spawn_commit, dim3(1), dim3(64), 0, g.stream,
    (const uint32_t*)g.d_tcnt, g.d_live);
  HIPCK(hipGetLastError());
  HIPCK(hipMemsetAsync(g.d_spawn_n, 0, sizeof(unsigned int), g.stream));
  return 0;
}

// ---- messages to the host (include/gpu_actor_host.h) -------------------------
// Device room for g.host_reserve messages: kHostShards segments whose sizes
// sum to at least the reserve (send_host fills a full segment's neighbours, so
// nothing is lost before every segment is full; a collection keeps at most
// the reserve). Called with nothing listed (between collections).
int host_alloc()
{
  HIPCK(hipStreamSynchronize(g.stream));        // no step still lists into the old segments
  g.hl = {};
  g.host_seg = 0;
  if(!g.d_host_n)
  {
    HIPCK(g.d_host_n.alloc(kHostShards));
    HIPCK(hipMemsetAsync(g.d_host_n, 0, kHostShards * sizeof(unsigned int), g.stream));
    HIPCK(g.h_host_n.alloc(kHostShards));
    HIPCK(g.d_host_step.alloc(1));
    HIPCK(hipMemsetAsync(g.d_host_step, 0, sizeof(uint64_t), g.stream));
  }
  const uint64_t n = g.host_reserve;
  const uint32_t seg = (uint32_t)((n + kHostShards - 1) / kHostShards);
  const size_t room = (size_t)seg * kHostShards;
  auto ck = [](hipError_t e) { if(e != hipSuccess) (void)hipGetLastError(); return e == hipSuccess; };
  if(!ck(g.hl.d_host_key.alloc(room)) || !ck(g.hl.d_host_kc.alloc(room)) || !ck(g.hl.d_host_ks.alloc(room)) ||
     !ck(g.hl.d_host_ic.alloc(room)) || !ck(g.hl.d_host_is.alloc(room)) || !ck(g.hl.d_host_rec.alloc(room)) ||
     !ck(g.hl.d_host_out.alloc(n)) || !ck(g.hl.h_host_out.alloc(n)))
  {
    g.hl = {};                                  // no room: none of the lists is kept
    return GPU_ACTOR_ENOMEM;
  }
  g.host_seg = seg;
  // the key: 16 sequence bits, the bits of an id below max_actors, the step
  // since the last collection above them
  uint32_t fbits = 1;
  while(fbits < 32 && (1ull << fbits) < g.cfg.max_actors) ++fbits;
  g.host_kshift = 16 + fbits;
  return 0;
}

// steps one collection's keys can tell apart (gpu_actor_run_fixed checks)
inline uint64_t host_step_room()
{
  return std::min<uint64_t>(1ull << (64 - g.host_kshift), 1ull << 31);
}

// The messages listed since the last collection, made canonical and handed to
// the host: one readback of the segments' counts (the wait that engines with
// spawning types make in spawn_process); then, when there are any, the
// segments compacted to one run, sorted by key (step, sender, sequence),
// gathered as gpu_host_msg_t, copied out in one piece, and the counts cleared
// on the stream. They go to the notify callback, or the queue gpu_actor_recv
// empties. A collection that holds more than the reserve keeps the first
// `reserve` in key order; the rest count as dropped.
int host_collect()
{
  if(!g.host_dirty) return 0;
  HIPCK(hipMemcpyAsync(g.h_host_n, g.d_host_n, kHostShards * sizeof(unsigned int),
    hipMemcpyDeviceToHost, g.stream));
  HIPCK(hipStreamSynchronize(g.stream));
  const uint32_t steps = g.sidx - g.host_base;
  g.host_dirty = false;
  HostOff o;
  uint64_t total = 0;
  for(uint32_t s = 0; s < kHostShards; ++s)
  {
    o.off[s] = (uint32_t)total;
    total += std::min<unsigned int>(g.h_host_n[s], g.host_seg);
  }
  o.off[kHostShards] = (uint32_t)total;
  if(total == 0) return 0;
  const uint32_t n = (uint32_t)total;
  hipLaunchKernelGGL(k_host_compact, dim3(blocks_for(n)), dim3(kBlock), 0, g.stream,
    (const uint64_t*)g.hl.d_host_key, o, g.host_seg, g.hl.d_host_kc, g.hl.d_host_ic);
  HIPCK(hipGetLastError());
  int end_bit = (int)g.host_kshift;
  while(end_bit < 64 && (uint64_t)steps > (1ull << (end_bit - (int)g.host_kshift))) ++end_bit;
  size_t need = 0;
  uint64_t *kc = g.hl.d_host_kc, *ks = g.hl.d_host_ks;
  uint32_t *ic = g.hl.d_host_ic, *is = g.hl.d_host_is;
  HIPCK(hipcub::DeviceRadixSort::SortPairs(nullptr, need, kc, ks, ic, is, (int)n, 0, end_bit, g.stream));
  HIPCK(sort_room(need));
  HIPCK(hipcub::DeviceRadixSort::SortPairs(g.d_sort_tmp, need, kc, ks, ic, is, (int)n, 0, end_bit,
    g.stream));
  const uint32_t keep = (uint32_t)std::min<uint64_t>(n, g.host_reserve);
  hipLaunchKernelGGL(k_host_gather, dim3(blocks_for(keep)), dim3(kBlock), 0, g.stream,
    (const uint64_t*)g.hl.d_host_ks, (const uint32_t*)g.hl.d_host_is, (const uint4*)g.hl.d_host_rec,
    g.hl.d_host_out, keep, (uint64_t)g.host_base, g.host_kshift);
  if(n > keep)
  {
    hipLaunchKernelGGL(k_host_lost, dim3(1), dim3(1), 0, g.stream, (unsigned long long)(n - keep));
    g.dev_epoch++;
  }
  HIPCK(hipGetLastError());
  HIPCK(hipMemcpyAsync(g.hl.h_host_out, g.hl.d_host_out, (size_t)keep * sizeof(gpu_host_msg_t),
    hipMemcpyDeviceToHost, g.stream));
  HIPCK(hipMemsetAsync(g.d_host_n, 0, kHostShards * sizeof(unsigned int), g.stream));
  HIPCK(hipStreamSynchronize(g.stream));
  if(g.host_fn)
    g.host_fn(g.host_ctx, g.hl.h_host_out, keep);
  else
  {
    if(g.hostq_head == g.hostq.size()) { g.hostq.clear(); g.hostq_head = 0; }
    try { g.hostq.insert(g.hostq.end(), g.hl.h_host_out.get(), g.hl.h_host_out + keep); }
    catch(...) { return GPU_ACTOR_ENOMEM; }
  }
  return 0;
}

// The plan of a step (StepPlan) for the configuration as it stands: the
// compiled-in entry `se` and its launch form, and the run-time compiled step
// it takes instead (jit_host.h), with PONYC_AMD_JIT not 0: 1 — every serial
// actor runs a program: the programs compiled (two launches, PM 1 plain zones
// and PM 2 the rest, with the split launches on); 2 — a mix of tables the
// any-mix kernel would run: that kernel with only those tables' drains;
// 0 — neither. The environment knobs are read here, once per configuration.
void plan_step(const StepEntry& se)
{
  StepPlan p;
  p.entry = se;
  p.stub = se.stub;
  // bucket arrays (4 x buckets — an order-free zone's two passes need no
  // more: zone_dev.h two_pass; six for a message-local table's, dp_table)
  // and, for hot receivers, the sort's work area
  const uint64_t nb = g.n_zones + (R() > 1 ? R() : 0);
  p.fits = step_fits(se, nb);
  p.dyn = step_dyn_bytes(se, nb);
  // a two-pass table's step as two launches: its two-pass zones, then the
  // rest (zone_dev.h k_step PM; PONYC_AMD_SPLIT_PLAN=0: one launch of the
  // whole), or fused: one launch of PM 3 in their place (PONYC_AMD_FUSE=0: two)
  const char* sp = getenv("PONYC_AMD_SPLIT_PLAN");
  const char* fu = getenv("PONYC_AMD_FUSE");
  const bool split_plan = !(sp && atoi(sp) == 0);
  const bool fused = se.plan && split_plan && !(fu && atoi(fu) == 0) && se.fused;
  const bool split = se.plan && split_plan && !fused;
  p.first = fused ? se.fused : split ? se.plan : se.kernel;
  p.second = split ? se.rest : nullptr;
  g.plan = p;
  const char* f = getenv("PONYC_AMD_JIT");
  if(f && atoi(f) == 0) return;
  const bool z12 = g.zbits == 12;
  const uint64_t geo = jit::fnv1a(z12 ? "z12" : "z11");
  uint64_t key = geo;                   // of the programs, while every serial type has one
  p.jit_mask = serial_tables();
  bool all_prog = p.jit_mask == 1u << GPU_ACTOR_HT_PROGRAM;
  for(uint32_t t = 0; t < GPU_ACTOR_MAX_TYPES && all_prog; ++t)
  {
    const HostType& h = g.types[t];
    if(!h.created || reducible_ht(h.ht)) continue;
    all_prog = !h.prog_host.empty();
    key = jit::fnv1a(std::string(reinterpret_cast<const char*>(h.prog_host.data()), h.prog_host.size() * 8),
                     jit::fnv1a(std::to_string(t), key));
  }
  if(all_prog && split_plan)
  {
    p.jit_kind = 1;
    p.jit_key = key;
  }
  else if(se.kernel == step_entry(-1, z12).kernel && p.jit_mask)
  {
    p.jit_kind = 2;
    p.jit_key = jit::fnv1a("mix" + std::to_string(p.jit_mask), geo);
  }
  g.plan = p;
}

// The plan's run-time compiled module, built or loaded once per set (a set
// whose build fails stays on the compiled-in kernels; one seen before in this
// process, or on disk, loads at once), with this engine's constants in it.
bool jit_load(const StepPlan& p)
{
  if(g.jit.mod && g.jit_set == p.jit_key) return true;
  if(g.jit_failed == p.jit_key) return false;
  jit::unload(g.jit);
  hipDeviceProp_t prop;
  if(hipGetDeviceProperties(&prop, g.device) != hipSuccess) { (void)hipGetLastError(); return false; }
  std::string arch = prop.gcnArchName;
  arch = arch.substr(0, arch.find(':'));
  const bool z12 = g.zbits == 12;
  std::string log;
  int rc;
  if(p.jit_kind == 1)
  {
    std::vector<jit::Prog> progs;
    for(uint32_t t = 0; t < GPU_ACTOR_MAX_TYPES; ++t)
      if(g.types[t].created && !reducible_ht(g.types[t].ht)) progs.push_back({t, g.types[t].prog_host});
    rc = jit::build(progs, z12, arch, g.jit, log);
  }
  else
    rc = jit::build_mix(p.jit_mask, z12, arch, g.jit, log);
  if(getenv("PONYC_AMD_JIT_LOG"))
    fprintf(stderr, "gpu_actor jit: %s %s%s (rc %d) %s\n", p.jit_kind == 1 ? "programs" : "mix",
            p.jit_kind == 2 ? ("mask " + std::to_string(p.jit_mask) + " ").c_str() : "", z12 ? "z12" : "z11", rc,
            log.c_str());
  if(rc != 0)
  {
    g.jit_failed = p.jit_key;
    return false;
  }
  g.jit_set = p.jit_key;
  g.jit_builds++;
  if(hipMemcpyHtoDAsync(g.jit.types, g.td_host, sizeof(g.td_host), g.stream) != hipSuccess ||
     hipMemcpyHtoDAsync(g.jit.eng, &g.eng_host, sizeof(g.eng_host), g.stream) != hipSuccess)
  {
    (void)hipGetLastError();
    jit::unload(g.jit);
    g.jit_failed = p.jit_key;
    return false;
  }
  return true;
}

// Whether the step runs the plan's run-time compiled module: it is wanted,
// it builds, and its static LDS leaves room for the bucket arrays. Asked at
// the first launch under a plan; the answer stands until the next plan.
bool jit_ready()
{
  StepPlan& p = g.plan;
  if(!p.jit_kind || !g.consts_host) return false;
  if(!p.jit_asked)
  {
    p.jit_asked = true;
    p.jit_ok = jit_load(p) && g.jit.static_lds + p.dyn <= kLdsPerWorkgroup;
  }
  return p.jit_ok;
}

int step_after_launch(uint32_t slot);

// One superstep: the plan's launches on parity g.par (+ exchange), then flip
// parity.
int launch_step(uint32_t slot)
{
  if(g.n_zones == 0) return 0;
  g.dev_epoch++;
  const StepPlan& p = g.plan;
  const StepEntry& se = p.entry;
  if(p.stub) return GPU_ACTOR_EINVAL;       // an experiment build without this table
  if(g.land8) g.land8_dirty = true;
  if(!p.fits) return GPU_ACTOR_ERANGE;      // more buckets than a workgroup's LDS holds
  // an engine with host ports: this step's place in the keys of the messages
  // it sends out (send_host reads it), counted from the first step since the
  // last collection
  if(g.host_ports)
  {
    if(!g.host_seg) return GPU_ACTOR_ENOMEM;     // a failed gpu_actor_host_reserve left no lists
    if(!g.host_dirty) { g.host_base = g.sidx; g.host_dirty = true; }
    hipLaunchKernelGGL(k_host_begin, dim3(1), dim3(1), 0, g.stream, g.d_host_step,
      (uint64_t)(g.sidx - g.host_base) << g.host_kshift);
    HIPCK(hipGetLastError());
  }
  // hot zones first (hot_dev.h): the whole GPU prepares them for k_step
  const size_t hot_lds = 5u * zone_actors() * sizeof(uint32_t);
  // the run-time compiled step: the programs' as two launches like the
  // interpreter's, or a mix's one launch with k_hot before it where hot zones
  // are prepared
  g.jit_used = jit_ready();
  if(g.jit_used)
  {
    uint32_t a_cur = g.par, a_slot = slot, a_sidx = g.sidx;
    void* args[] = {&a_cur, &a_slot, &a_sidx};
    if(p.jit_kind == 2 && g.hot_on)
      hipLaunchKernelGGL(k_hot, dim3(kHotBlocks), dim3(kHotThreads), hot_lds, g.stream, g.par, g.sidx);
    HIPCK(hipModuleLaunchKernel(g.jit.plan, g.n_zones, 1, 1, se.threads, 1, 1, (unsigned)p.dyn, g.stream,
      args, nullptr));
    if(p.jit_kind == 1)
      HIPCK(hipModuleLaunchKernel(g.jit.rest, g.n_zones, 1, 1, se.threads, 1, 1, (unsigned)p.dyn, g.stream,
        args, nullptr));
  }
  else
  {
    if(g.hot_on)
      hipLaunchKernelGGL(k_hot, dim3(kHotBlocks), dim3(kHotThreads), hot_lds, g.stream, g.par, g.sidx);
    hipLaunchKernelGGL(p.first, dim3(g.n_zones), dim3(se.threads), p.dyn, g.stream, g.par, slot, g.sidx);
    if(p.second)
      hipLaunchKernelGGL(p.second, dim3(g.n_zones), dim3(se.threads), p.dyn, g.stream, g.par, slot, g.sidx);
  }
  if(g.defer_big)
    hipLaunchKernelGGL(k_carry_big, dim3(kBigCopyBlocks), dim3(kBlock), 0, g.stream, g.par);
  HIPCK(hipGetLastError());
  const int grc = gups_apply_launch();
  if(grc) return grc;
  return step_after_launch(slot);
}

// n_ranks > 1, behind a step that ran: every rank's packed GUPS chunks
// (k_gups_pack; the counts are on the host since exchange_step's readback)
// gathered in rank order — one 8-byte PolyRand state per chunk, through the
// grouped send/recv that gathers spawn records — and applied by
// k_gups_apply_ranks. A rank that owns no updater takes part in the gather
// and launches nothing.
int gups_gather_apply()
{
  const uint32_t n = R();
  const unsigned long long* cnt = g.h_xc + 2 * n + 3;
  std::vector<uint64_t> off(n);
  uint64_t total = 0;
  for(uint32_t p = 0; p < n; ++p)
  {
    off[p] = total;
    total += cnt[p];
  }
  const uint64_t mine = cnt[rank()];
  g.gups_out_total += mine;
  g.gups_in_total += total - mine;
  if(total > g.d_gups_all.size())
  {
    const uint64_t cap = std::max<uint64_t>({2ull * g.d_gups_all.size(), total + total / 2, 1ull << 16});
    HIPCK(hipStreamSynchronize(g.stream));      // no k_gups_apply_ranks still reads the old one
    HIPCK(g.d_gups_all.alloc(cap));
  }
  if(total)
  {
    if(mine)
      HIPCK(hipMemcpyAsync(g.d_gups_all + off[rank()], g.d_gups_send, mine * sizeof(uint64_t),
        hipMemcpyDeviceToDevice, g.stream));
    std::vector<XcPeer> pp(n);
    for(uint32_t p = 0; p < n; ++p)
    {
      if(p == rank()) continue;
      pp[p].d_send = g.d_gups_send;
      pp[p].send = mine * sizeof(uint64_t);
      pp[p].d_recv = g.d_gups_all + off[p];
      pp[p].recv = cnt[p] * sizeof(uint64_t);
    }
    const int rc = xc_sendrecv(pp);
    if(rc) return rc;
    // the updaters the streamers write: ids ubase .. ubase + mask
    const HostType& h = g.types[g.gups_type];
    const uint64_t u0 = h.params[3], u1 = u0 + h.params[2] + 1;
    if(owned_below(u1) > owned_below(u0))
    {
      const uint64_t per_block = 4ull * (64u / g.gups_parts);
      const uint32_t blocks = (uint32_t)std::min<uint64_t>((total + per_block - 1) / per_block, kGupsBlocks);
      hipLaunchKernelGGL(k_gups_apply_ranks, dim3(blocks), dim3(256), 0, g.stream,
        (const uint64_t*)g.d_gups_all, total, off[rank()], mine);
      HIPCK(hipGetLastError());
    }
  }
  return 0;
}

// After a step's launches: the parity and step index advance; the exchange
// (n_ranks > 1), the halted step's rerun, the GUPS chunks' gather and apply
// (n_ranks > 1), spawned actors.
int step_after_launch(uint32_t slot)
{
  HIPCK(hipGetLastError());
  const uint32_t step_sidx = g.sidx;
  g.par ^= 1u;
  g.sidx++;
  if(R() > 1)
  {
    int rc = exchange_step(step_sidx);
    if(rc) return rc;
    if(g.h_sstat->halt)
    {
      // this step did not run on any rank (a zone overflowed on some rank the
      // step before): grow, then run it again from the same parity and index
      rc = fixup_spill();
      if(rc) return rc;
      g.par ^= 1u;
      g.sidx--;
      rc = pend_clear(slot, 1);
      if(rc) return rc;
      return launch_step(slot);
    }
    if(g.gups_type >= 0)
    {
      rc = gups_gather_apply();
      if(rc) return rc;
    }
  }
  if(g.spawn_cap)
  {
    int rc = spawn_process(g.par);
    if(rc) return rc;
  }
  // the messages this step sent to host ports (gpu_actor_run_fixed leaves
  // them to the next call that observes the engine)
  if(g.host_ports && !g.host_defer)
  {
    int rc = host_collect();
    if(rc) return rc;
  }
  return 0;
}

int launch_pending(uint32_t slot)
{
  if(g.n_zones == 0) return 0;
  hipLaunchKernelGGL(k_pending, dim3(blocks_for(g.n_zones)), dim3(kBlock), 0, g.stream,
    g.par, slot);
  HIPCK(hipGetLastError());
  return 0;
}

// Sum over ranks of pend[first .. first+n) (host side, after sync).
int pend_read(uint32_t first, uint32_t n, std::vector<unsigned long long>& out)
{
  out.resize(n);
  {
    const int rc = fold_counters(first, n);
    if(rc) return rc;
  }
  if(R() > 1)
  {
    const int rc = xc_allreduce_sum(g.d_pend + first, g.d_pend + first, n, XC_U64);
    if(rc) return rc;
  }
  HIPCK(hipMemcpyAsync(out.data(), g.d_pend + first, n * sizeof(unsigned long long),
    hipMemcpyDeviceToHost, g.stream));
  HIPCK(hipStreamSynchronize(g.stream));
  return 0;
}

// k_gups_apply's (n_ranks > 1: k_gups_apply_ranks') per-workgroup counts
// summed: updates made, atomics issued, updates of peers' chunks.
int gups_stat_read(uint64_t out[3])
{
  out[0] = out[1] = out[2] = 0;
  if(!g.d_gups_stat) return 0;
  std::vector<unsigned long long> st(3 * kGupsBlocks);
  HIPCK(hipMemcpyAsync(st.data(), g.d_gups_stat, st.size() * sizeof(unsigned long long),
    hipMemcpyDeviceToHost, g.stream));
  HIPCK(hipStreamSynchronize(g.stream));
  for(uint32_t b = 0; b < kGupsBlocks; ++b)
    for(int k = 0; k < 3; ++k) out[k] += st[(size_t)k * kGupsBlocks + b];
  return 0;
}

int ensure_events(size_t n)
{
  while(g.ev.size() < n)
  {
    hipEvent_t e;
    HIPCK(hipEventCreate(&e));
    g.ev.push_back(e);
  }
  return 0;
}

// The end of a session (gpu_actor_shutdown, a failed gpu_actor_init): the
// run-time compiled module, the peers' mapped inboxes, then the session's
// value — every buffer frees itself — replaced by a fresh one; the events, the
// communicator and the stream go last.
void session_end()
{
  if(g.stream) (void)hipStreamSynchronize(g.stream);
  jit::unload(g.jit);
  peer_close();
  const std::vector<hipEvent_t> ev = std::move(g.ev);
  const ncclComm_t comm = g.comm;
  const hipStream_t stream = g.stream;
  g.~Session();
  new(&g) Session;
  for(hipEvent_t e : ev) (void)hipEventDestroy(e);
  if(comm) (void)ncclCommDestroy(comm);
  if(stream) (void)hipStreamDestroy(stream);
}

// A host send must name an actor of this rank (each rank injects its own
// share; k_inject lands only local mail).
inline bool host_msg_ok(const gpu_msg_t& m)
{
  // (a host port has no mailbox: only programs address it, gpu_actor_host.h)
  // (the ranges upload_types worked out: one test for every other target)
  if(m.to - g.eng_host.host_first < g.eng_host.host_span)
    for(uint32_t k = 0; k < g.eng_host.host_nrng; ++k)
      if(m.to - g.eng_host.host_rng[k].first < g.eng_host.host_rng[k].count) return false;
  return m.to < g.n_actors && m.behaviour <= 0xF && (R() == 1 || place_owner(R(), g.block_bits, m.to) == rank());
}

int inject_locked(const gpu_msg_t* first, uint64_t n)
{
  if(g.host_seq + n >= (1ull << 40)) return GPU_ACTOR_ERANGE;
  g.dev_epoch++;
  if(n > g.d_msgs.size()) HIPCK(g.d_msgs.alloc(n));
  HIPCK(hipMemcpyAsync(g.d_msgs, first, n * sizeof(gpu_msg_t), hipMemcpyHostToDevice, g.stream));
  if(g.n_zones)
  {
    hipLaunchKernelGGL(k_inject, dim3(blocks_for(n, kLandRecs)), dim3(kLandThreads), 0, g.stream,
      (const gpu_msg_t*)g.d_msgs, n, g.host_seq, g.par);
    HIPCK(hipGetLastError());
  }
  g.host_seq += n;
  // the caller may reuse its buffer: this synchronises the stream
  int rc = read_sstat();
  if(rc) return rc;
  return spill_pending() ? fixup_spill() : 0;
}

// gpu_actor_send's deferred messages, injected in call order.
int flush_sends()
{
  if(g.deferred.empty()) return 0;
  const int rc = inject_locked(g.deferred.data(), g.deferred.size());
  g.deferred.clear();
  return rc;
}

int sendv_locked(const gpu_msg_t* first, uint64_t n)
{
  if(n == 0) return 0;
  if(!first) return GPU_ACTOR_EINVAL;
  for(uint64_t i = 0; i < n; ++i)
    if(!host_msg_ok(first[i])) return GPU_ACTOR_EINVAL;
  int rc = flush_sends();                   // earlier single sends go first
  if(rc) return rc;
  return inject_locked(first, n);
}

// Ahead of a call that observes the engine: staged host sends go in, and the
// messages to host ports a gpu_actor_run_fixed left listed on the device come
// out (nothing to do, and no wait, in an engine without ports).
int observe()
{
  const int rc = flush_sends();
  return rc ? rc : host_collect();
}

} // namespace

// ===========================================================================
// C-ABI
// ===========================================================================
extern "C" {

GPU_ACTOR_API const char* gpu_actor_strerror(int code)
{
  switch(code)
  {
    case GPU_ACTOR_OK: return "ok";
    case GPU_ACTOR_EINVAL: return "invalid argument";
    case GPU_ACTOR_ENOMEM: return "out of memory";
    case GPU_ACTOR_ENODEV: return "no usable GPU";
    case GPU_ACTOR_EMAILBOX: return "mailbox overflow (messages dropped)";
    case GPU_ACTOR_EHIP: return "HIP runtime error";
    case GPU_ACTOR_ESTATE: return "engine not initialised or already initialised";
    case GPU_ACTOR_ERANGE: return "sequence or id space exhausted";
    case GPU_ACTOR_ECOMM: return "RCCL exchange failure";
    case GPU_ACTOR_EBUSY: return "an asynchronous run is in flight";
    default: return "unknown error";
  }
}

GPU_ACTOR_API int gpu_actor_comm_id(void* out128)
{
  if(!out128) return GPU_ACTOR_EINVAL;
  ncclUniqueId id;
  NCCLCK(ncclGetUniqueId(&id));
  static_assert(sizeof(id) == 128, "ncclUniqueId is 128 bytes");
  memcpy(out128, &id, sizeof(id));
  return 0;
}

} // extern "C"

namespace {

// gpu_actor_init's work on a fresh session; a failure leaves what it has
// made so far to the caller's session_end().
int session_begin(const gpu_actor_config_t* cfg)
{
  g.cfg = *cfg;
  if(g.cfg.n_ranks == 0) g.cfg.n_ranks = 1;
  if(g.cfg.rank >= g.cfg.n_ranks || g.cfg.n_ranks > kMaxRanks) return GPU_ACTOR_EINVAL;
  if(g.cfg.batch == 0) g.cfg.batch = 100;                 // PONY_SCHED_BATCH
  if(g.cfg.mailbox_cap == 0) g.cfg.mailbox_cap = 16;
  if(g.cfg.max_actors == 0) g.cfg.max_actors = 1ull << 26;
  if(g.cfg.max_actors > 0xFF000000ull) return GPU_ACTOR_EINVAL;
  if(gp.place_bits >= 0)
    g.block_bits = (uint32_t)gp.place_bits;
  else if(const char* f = getenv("PONYC_AMD_BLOCK_BITS"))   // test hook: the default placement
  {
    const int b = atoi(f);
    if(b < 0 || b > (int)GPU_ACTOR_PLACE_MAX_BITS) return GPU_ACTOR_EINVAL;
    g.block_bits = (uint32_t)b;
  }

  int ndev = 0;
  if(hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return GPU_ACTOR_ENODEV;
  g.device = cfg->device >= 0 ? cfg->device : 0;
  if(cfg->device < 0) (void)hipGetDevice(&g.device);
  if(g.device >= ndev) return GPU_ACTOR_ENODEV;
  HIPCK(hipSetDevice(g.device));
  HIPCK(hipStreamCreateWithFlags(&g.stream, hipStreamNonBlocking));

  HIPCK(g.d_stats.alloc(ST_COUNT));
  HIPCK(hipMemsetAsync(g.d_stats, 0, ST_COUNT * sizeof(unsigned long long), g.stream));
  HIPCK(g.d_pend.alloc(kPendSlots));
  HIPCK(g.d_pend_sh.alloc((size_t)kPendSlots * kShards));
  HIPCK(hipMemsetAsync(g.d_pend_sh, 0, (size_t)kPendSlots * kShards * sizeof(unsigned long long),
    g.stream));
  {
    // hot-zone scratch (hot_dev.h): prep, slot, counts, key ranges (fmin
    // starts at ~0), bins, bin counts, cursors, barrier
    HIPCK(g.d_hot.alloc(kHotLayout.words));
    HIPCK(hipMemsetAsync(g.d_hot, 0, kHotLayout.words * sizeof(uint32_t), g.stream));
    uint32_t* aux = g.d_hot + kHotLayout.aux;
    for(uint32_t h = 0; h < kMaxHot; ++h)
      HIPCK(hipMemsetAsync(aux + (size_t)h * 3 * kHotActors, 0xFF, kHotActors * sizeof(uint32_t),
        g.stream));
  }
  HIPCK(g.d_stats_sh.alloc((size_t)ST_COUNT * kShards));
  HIPCK(hipMemsetAsync(g.d_stats_sh, 0, (size_t)ST_COUNT * kShards * sizeof(unsigned long long),
    g.stream));
  HIPCK(g.d_dbg.alloc(kMaxZones * kDbgSlots));
  HIPCK(hipMemsetAsync(g.d_dbg, 0, kMaxZones * kDbgSlots * sizeof(unsigned long long), g.stream));
  HIPCK(g.d_spawn_n.alloc(1));
  HIPCK(hipMemsetAsync(g.d_spawn_n, 0, sizeof(unsigned int), g.stream));
  HIPCK(g.d_tstart.alloc(GPU_ACTOR_MAX_TYPES));
  HIPCK(g.d_tcnt.alloc(GPU_ACTOR_MAX_TYPES));
  HIPCK(g.d_live.alloc(GPU_ACTOR_MAX_TYPES));
  HIPCK(g.d_ctl.alloc(1));
  HIPCK(g.d_sstat.alloc(1));
  HIPCK(hipMemsetAsync(g.d_sstat, 0, sizeof(SpillStat), g.stream));
  HIPCK(g.h_sstat.alloc(1));
  memset(g.h_sstat, 0, sizeof(SpillStat));
  HIPCK(g.d_need.alloc(kMaxZones));
  HIPCK(g.d_zplan.alloc(kMaxZones));
  HIPCK(hipMemsetAsync(g.d_zplan, 0, kMaxZones * sizeof(uint32_t), g.stream));
  g.trig_bytes = (g.cfg.max_actors + 2 * 4096 + 7) & ~7ull;   // room for either zone size
  for(int p = 0; p < 2; ++p)
  {
    HIPCK(g.d_trig[p].alloc(g.trig_bytes));
    HIPCK(hipMemsetAsync(g.d_trig[p], 0, g.trig_bytes, g.stream));
    HIPCK(g.d_ztrig[p].alloc(kMaxZones));
    HIPCK(hipMemsetAsync(g.d_ztrig[p], 0, kMaxZones * sizeof(uint32_t), g.stream));
    if(R() > 1)
    {
      HIPCK(g.d_trig_own[p].alloc(g.trig_bytes));
      HIPCK(hipMemsetAsync(g.d_trig_own[p], 0, g.trig_bytes, g.stream));
    }
  }
  HIPCK(g.d_spill_flag.alloc(1));
  HIPCK(hipMemsetAsync(g.d_spill_flag, 0, sizeof(unsigned int), g.stream));
  HIPCK(g.d_trig_n.alloc(4));
  HIPCK(hipMemsetAsync(g.d_trig_n, 0, 4 * sizeof(unsigned int), g.stream));
  HIPCK(g.d_bigc.alloc(kBigCopyCap));
  HIPCK(g.d_bigc_n.alloc(2));
  HIPCK(hipMemsetAsync(g.d_bigc_n, 0, 2 * sizeof(unsigned long long), g.stream));
  HIPCK(g.h_ctl.alloc(1));
  HIPCK(hipMemsetAsync(g.d_live, 0, GPU_ACTOR_MAX_TYPES * sizeof(unsigned long long), g.stream));

  if(R() > 1)
  {
    g.xcap = g.cfg.max_exchange ? g.cfg.max_exchange : (1u << 22);
    if(cfg->comm_id)
    {
      ncclUniqueId id;
      memcpy(&id, cfg->comm_id, sizeof(id));
      NCCLCK(ncclCommInitRank(&g.comm, (int)R(), id, (int)rank()));
      gp.xp_a2a = nullptr;
      gp.xp_ar = nullptr;
    }
    else
    {
      // host transport (callbacks registered with gpu_actor_set_transport);
      // its staging grows on demand (stage_room)
      if(!gp.xp_a2a || !gp.xp_ar) return GPU_ACTOR_EINVAL;
    }
    {
      const char* pw = getenv("PONYC_AMD_PEER_WRITE");
      g.peer_write = pw && atoi(pw) != 0;
    }
    if(g.peer_write)
    {
      HIPCK(g.d_pin.alloc((size_t)R() * g.xcap));
      HIPCK(g.d_hx.alloc(1 + R()));
    }
    else
    {
      HIPCK(g.d_xout.alloc((size_t)R() * g.xcap));
      HIPCK(g.d_xin.alloc((size_t)R() * g.xcap));
    }
    HIPCK(g.d_xspill_n.alloc(1));
    HIPCK(hipMemsetAsync(g.d_xspill_n, 0, sizeof(unsigned int), g.stream));
    {
      const int xrc = alloc_xspill(std::max<uint32_t>(1u << 18, g.xcap / 2));
      if(xrc) return xrc;
    }
    HIPCK(g.d_xc.alloc(3 * R() + 3));
    HIPCK(hipMemsetAsync(g.d_xc, 0, (3 * R() + 3) * sizeof(unsigned long long), g.stream));
    HIPCK(g.h_xc.alloc(3 * R() + 3));
    g.d_xcount = g.d_xc;
    g.d_xrecv = g.d_xc + R();
    g.h_xcount.assign(R(), 0);
    g.h_xrecv.assign(R(), 0);
    {
      // one placement on every rank: with b and b^2 summed over ranks, all
      // b are equal iff (sum b)^2 == R * sum b^2 (Cauchy-Schwarz); every rank
      // sees the same sums, so all fail or none
      unsigned long long v[2] = {g.block_bits, (unsigned long long)g.block_bits * g.block_bits};
      unsigned long long* dc = g.d_xc + 2 * R();         // scratch words of the counts block
      HIPCK(hipMemcpyAsync(dc, v, sizeof(v), hipMemcpyHostToDevice, g.stream));
      const int prc = xc_allreduce_sum(dc, dc, 2, XC_U64);
      if(prc) return prc;
      HIPCK(hipMemcpyAsync(v, dc, sizeof(v), hipMemcpyDeviceToHost, g.stream));
      HIPCK(hipStreamSynchronize(g.stream));
      const bool same = v[0] * v[0] == (unsigned long long)R() * v[1];
      HIPCK(hipMemsetAsync(dc, 0, sizeof(v), g.stream));
      if(!same) return GPU_ACTOR_EINVAL;
    }
    if(g.peer_write)
    {
      HIPCK(hipStreamSynchronize(g.stream));
      const int prc = peer_open();
      if(prc) return prc;
    }
  }
  g.init = true;
  int rc = upload_types();
  if(rc) return rc;
  HIPCK(hipStreamSynchronize(g.stream));
  return 0;
}

} // namespace

extern "C" {

// All or nothing: a failure ends the session as gpu_actor_shutdown does, so
// the engine is not initialised, holds nothing, and can be initialised again.
GPU_ACTOR_API int gpu_actor_init(const gpu_actor_config_t* cfg)
{
  std::lock_guard<std::mutex> lk(gp.mu);
  if(g.init) return GPU_ACTOR_ESTATE;
  if(!cfg) return GPU_ACTOR_EINVAL;
  const int rc = session_begin(cfg);
  if(rc) session_end();
  return rc;
}

// Joins a finished (or running) asynchronous run; caller must NOT hold gp.mu.
// Called on the progress thread itself (the completion callback chaining a
// run_async, wait or shutdown), it detaches instead: the thread ends right
// after its callback returns.
void join_worker()
{
  std::thread t;
  {
    std::lock_guard<std::mutex> wl(gp.wmu);
    if(!gp.worker.joinable()) return;
    if(gp.worker.get_id() == std::this_thread::get_id())
    {
      // it cannot join itself: gpu_actor_shutdown joins it later, so its
      // completion callback has returned before anything it runs is freed
      gp.detached.push_back(std::move(gp.worker));
      return;
    }
    t = std::move(gp.worker);
  }
  t.join();
}

// Joins the progress threads that chained runs from their callbacks (all
// but the calling thread itself); caller must NOT hold gp.mu.
void join_detached()
{
  std::vector<std::thread> ts;
  {
    std::lock_guard<std::mutex> wl(gp.wmu);
    for(auto& t : gp.detached)
    {
      if(t.get_id() == std::this_thread::get_id()) t.detach();   // returns after this call
      else ts.push_back(std::move(t));
    }
    gp.detached.clear();
  }
  for(auto& t : ts)
    if(t.joinable()) t.join();
}

GPU_ACTOR_API int gpu_actor_shutdown(void)
{
  join_worker();                      // an async run finishes first
  join_detached();
  std::lock_guard<std::mutex> lk(gp.mu);
  if(!g.init) return GPU_ACTOR_ESTATE;
  session_end();
  return 0;
}

GPU_ACTOR_API int gpu_actor_set_transport(gpu_actor_alltoallv_fn alltoallv,
  gpu_actor_allreduce_fn allreduce, void* ctx)
{
  std::lock_guard<std::mutex> lk(gp.mu);
  if(g.init) return GPU_ACTOR_ESTATE;
  if((alltoallv == nullptr) != (allreduce == nullptr)) return GPU_ACTOR_EINVAL;
  gp.xp_a2a = alltoallv;
  gp.xp_ar = allreduce;
  gp.xp_ctx = ctx;
  return 0;
}

GPU_ACTOR_API int gpu_actor_type_register(uint32_t type_id, uint32_t state_words,
  uint32_t handler_table)
{
  std::lock_guard<std::mutex> lk(gp.mu);
  if(!g.init) return GPU_ACTOR_ESTATE;
  if(type_id >= GPU_ACTOR_MAX_TYPES) return GPU_ACTOR_EINVAL;
  const uint32_t need = required_words(handler_table);
  if(need == 0 || state_words < need) return GPU_ACTOR_EINVAL;
  HostType& t = g.types[type_id];
  if(t.registered) return GPU_ACTOR_EINVAL;
  t.registered = true;
  t.words = state_words;
  t.ht = handler_table;
  t.batch = g.cfg.batch;
  t.cap = g.cfg.mailbox_cap;
  return 0;
}

GPU_ACTOR_API int gpu_actor_type_config(uint32_t type_id, uint32_t batch, uint32_t mailbox_cap)
{
  std::lock_guard<std::mutex> lk(gp.mu);
  if(!g.init) return GPU_ACTOR_ESTATE;
  if(type_id >= GPU_ACTOR_MAX_TYPES || !g.types[type_id].registered) return GPU_ACTOR_EINVAL;
  HostType& t = g.types[type_id];
  if(mailbox_cap & (mailbox_cap - 1)) return GPU_ACTOR_EINVAL;
  if(t.created && mailbox_cap && mailbox_cap != t.cap) return GPU_ACTOR_EINVAL;
  if(batch) t.batch = batch;
  if(mailbox_cap) t.cap = mailbox_cap;
  return t.created ? upload_types() : 0;
}

GPU_ACTOR_API int gpu_actor_type_priority(uint32_t type_id, int32_t priority)
{
  std::lock_guard<std::mutex> lk(gp.mu);
  if(!g.init) return GPU_ACTOR_ESTATE;
  if(type_id >= GPU_ACTOR_MAX_TYPES || !g.types[type_id].registered) return GPU_ACTOR_EINVAL;
  if(gp.async_busy) return GPU_ACTOR_EBUSY;
  g.types[type_id].priority = priority;
  return g.types[type_id].created ? upload_types() : 0;
}

GPU_ACTOR_API int gpu_actor_type_param(uint32_t type_id, uint32_t idx, uint64_t value)
{
  std::lock_guard<std::mutex> lk(gp.mu);
  if(!g.init) return GPU_ACTOR_ESTATE;
  if(type_id >= GPU_ACTOR_MAX_TYPES || idx >= GPU_ACTOR_MAX_PARAMS ||
    !g.types[type_id].registered) return GPU_ACTOR_EINVAL;
  g.types[type_id].params[idx] = value;
  return g.types[type_id].created ? upload_types() : 0;
}

GPU_ACTOR_API int gpu_actor_type_program(uint32_t type_id, const uint64_t* code, uint32_t n)
{
  std::lock_guard<std::mutex> lk(gp.mu);
  if(!g.init) return GPU_ACTOR_ESTATE;
  if(type_id >= GPU_ACTOR_MAX_TYPES || !g.types[type_id].registered ||
     g.types[type_id].ht != GPU_ACTOR_HT_PROGRAM || !code || n <= GPU_ACTOR_PROG_ENTRIES ||
     n > (1u << 20)) return GPU_ACTOR_EINVAL;
  if(gp.async_busy) return GPU_ACTOR_EBUSY;
  HostType& t = g.types[type_id];
  DevBuf<uint64_t> d;
  HIPCK(d.alloc(n));
  // on the engine's stream like every other upload; the new buffer is freed
  // if the copy fails
  if(hipMemcpyAsync(d, code, (size_t)n * sizeof(uint64_t), hipMemcpyHostToDevice, g.stream) !=
       hipSuccess || hipStreamSynchronize(g.stream) != hipSuccess)
  {
    (void)hipGetLastError();
    return GPU_ACTOR_EHIP;
  }
  if(t.d_prog) HIPCK(hipStreamSynchronize(g.stream));   // no launch still reads the old one
  t.d_prog = std::move(d);
  t.prog_n = n;
  t.prog_host.assign(code, code + n);
  t.prog_yields = false;
  for(uint32_t k = 0; k < n; ++k)                   // (a jump may run the entry words too)
    t.prog_yields |= (code[k] & 0xFFu) == GPU_ACTOR_OP_YIELD || (code[k] & 0xFFu) == GPU_ACTOR_OP_SPAWN;
  return t.created ? upload_types() : 0;
}

GPU_ACTOR_API int gpu_actor_create(uint32_t type_id, uint64_t count, uint64_t* first_id)
{
  std::lock_guard<std::mutex> lk(gp.mu);
  if(!g.init) return GPU_ACTOR_ESTATE;
  if(type_id >= GPU_ACTOR_MAX_TYPES) return GPU_ACTOR_EINVAL;
  HostType& t = g.types[type_id];
  if(!t.registered || t.created || count == 0) return GPU_ACTOR_EINVAL;
  const uint64_t live = count;
  count += t.reserve;                    // ids for the type's spawned actors
  if(g.n_actors + count > g.cfg.max_actors) return GPU_ACTOR_ERANGE;
  if(g.spawn_cap + t.reserve > 0xFFFFFFFFull) return GPU_ACTOR_ERANGE;
  if(t.ht == GPU_ACTOR_HT_GUPS_UPDATER)
  {
    const uint64_t size = t.params[0];
    if(size == 0 || (size & (size - 1)) || size > t.words) return GPU_ACTOR_EINVAL;
  }
  const uint64_t lo = owned_below(g.n_actors), hi = owned_below(g.n_actors + count);
  const uint32_t n_local = (uint32_t)hi;
  if((n_local + kZone - 1) / kZone > kMaxZones) return GPU_ACTOR_ERANGE;
  if(t.ht == GPU_ACTOR_HT_HOST_PORT && !g.host_ports)
  {
    // the first port type: room for the messages programs send out (before
    // anything of the type exists: a failure leaves it uncreated)
    const int hrc = host_alloc();
    if(hrc) return hrc;
    g.host_ports = true;
  }
  t.first = g.n_actors;
  t.count = count;
  t.lfirst = (uint32_t)lo;
  t.lcount = (uint32_t)(hi - lo);
  const size_t lc = std::max<size_t>(t.lcount, 1);
  HIPCK(t.d_state.alloc((size_t)t.words * lc));
  HIPCK(hipMemsetAsync(t.d_state, 0, (size_t)t.words * lc * sizeof(uint64_t), g.stream));
  t.created = true;
  g.n_actors += count;
  g.n_local = n_local;
  g.n_types = std::max(g.n_types, type_id + 1);
  int rc = relayout_zones(true);
  if(rc) return rc;
  rc = ensure_spill(spill_cap_for_zones());     // empty between calls: nothing to keep
  if(rc) return rc;
  rc = upload_types();
  if(rc) return rc;
  hipLaunchKernelGGL(k_construct, dim3(blocks_for(std::max<uint64_t>(t.lcount, 1))), dim3(kBlock), 0,
    g.stream, type_id, (uint32_t)live);
  if(t.ht == GPU_ACTOR_HT_GUPS_UPDATER)
    hipLaunchKernelGGL(k_construct_table, dim3(4096), dim3(kBlock), 0, g.stream,
      type_id, (uint32_t)live);
  HIPCK(hipGetLastError());
  const unsigned long long live_ull = live;
  HIPCK(hipMemcpyAsync(g.d_live + type_id, &live_ull, sizeof(live_ull), hipMemcpyHostToDevice,
    g.stream));
  if(t.reserve)
  {
    // the spawn buffers hold one record per reserved id; nothing is in them
    // between steps, so growing them drops nothing
    HIPCK(hipStreamSynchronize(g.stream));
    // the gathered list of n_ranks > 1 holds every rank's records
    const uint32_t cap = g.spawn_cap + (uint32_t)t.reserve;
    for(int p = 0; p < 2; ++p)
    {
      HIPCK(g.d_skey[p].alloc((size_t)cap * R()));
      HIPCK(g.d_sarg[p].alloc((size_t)cap * R()));
    }
    g.spawn_cap = cap;
    rc = upload_types();
    if(rc) return rc;
  }
  HIPCK(hipStreamSynchronize(g.stream));
  if(first_id) *first_id = t.first;
  return 0;
}

GPU_ACTOR_API int gpu_actor_type_reserve(uint32_t type_id, uint64_t n)
{
  std::lock_guard<std::mutex> lk(gp.mu);
  if(!g.init) return GPU_ACTOR_ESTATE;
  if(type_id >= GPU_ACTOR_MAX_TYPES || !g.types[type_id].registered ||
    g.types[type_id].created) return GPU_ACTOR_EINVAL;
  if(n > g.cfg.max_actors) return GPU_ACTOR_ERANGE;
  g.types[type_id].reserve = n;
  return 0;
}

GPU_ACTOR_API int gpu_actor_type_live(uint32_t type_id, uint64_t* live)
{
  std::lock_guard<std::mutex> lk(gp.mu);
  if(!g.init) return GPU_ACTOR_ESTATE;
  if(type_id >= GPU_ACTOR_MAX_TYPES || !live || !g.types[type_id].created)
    return GPU_ACTOR_EINVAL;
  unsigned long long v = 0;
  HIPCK(hipMemcpyAsync(&v, g.d_live + type_id, sizeof(v), hipMemcpyDeviceToHost, g.stream));
  HIPCK(hipStreamSynchronize(g.stream));
  *live = v;
  return 0;
}

GPU_ACTOR_API int gpu_actor_alloc_msgs(uint64_t n, gpu_msg_t** buf)
{
  std::lock_guard<std::mutex> lk(gp.mu);
  if(!g.init) return GPU_ACTOR_ESTATE;
  if(!buf) return GPU_ACTOR_EINVAL;
  if(n > g.h_msgs.size()) HIPCK(g.h_msgs.alloc(n));
  *buf = g.h_msgs;
  return 0;
}

GPU_ACTOR_API int gpu_actor_sendv(const gpu_msg_t* first, uint64_t n)
{
  std::lock_guard<std::mutex> lk(gp.mu);
  if(!g.init) return GPU_ACTOR_ESTATE;
  return sendv_locked(first, n);
}

GPU_ACTOR_API int gpu_actor_send(uint64_t to, uint32_t behaviour, uint64_t arg)
{
  std::lock_guard<std::mutex> lk(gp.mu);
  if(!g.init) return GPU_ACTOR_ESTATE;
  gpu_msg_t m;
  m.to = (uint32_t)to; m.behaviour = behaviour; m.arg = arg;
  if(to >= g.n_actors || !host_msg_ok(m)) return GPU_ACTOR_EINVAL;
  if(g.host_seq + g.deferred.size() + 1 >= (1ull << 40)) return GPU_ACTOR_ERANGE;
  try { g.deferred.push_back(m); } catch(...) { return GPU_ACTOR_ENOMEM; }
  return 0;
}

// The small-step path applies to one rank without spawning types (spawned
// ids are numbered by the host after each dense step). GPA_NO_SPARSE=1 turns
// it off (A/B runs).
bool sparse_ok()
{
  const char* e = getenv("GPA_NO_SPARSE");
  // (nor with host ports: their messages are keyed and collected per k_step)
  return !(e && atoi(e) != 0) && R() == 1 && g.spawn_cap == 0 && g.n_zones > 0 && !g.host_ports;
}

// One k_sparse launch from parity g.par: up to max_steps supersteps (0: no
// limit). Returns its control block after the launch completes.
int run_sparse(uint64_t max_steps, SparseCtl& out)
{
  g.dev_epoch++;
  {
    const int rc = land8_flush();          // k_sparse reads 16-byte landing records only
    if(rc) return rc;
  }
  bool prog = false, gups = false;
  for(const HostType& t : g.types)
  {
    prog |= t.created && t.ht == GPU_ACTOR_HT_PROGRAM;
    gups |= t.created && t.ht == GPU_ACTOR_HT_GUPS_STREAMER;
  }
#define GPA_SPARSE_LAUNCH(P, G)                                                         \
  hipLaunchKernelGGL((k_sparse<P, G>), dim3(1), dim3(kSpThreads), 0, g.stream, g.par,   \
    (unsigned long long)max_steps, g.d_ctl, g.sidx)
  if(prog && gups) GPA_SPARSE_LAUNCH(true, true);
  else if(prog) GPA_SPARSE_LAUNCH(true, false);
  else if(gups) GPA_SPARSE_LAUNCH(false, true);
  else GPA_SPARSE_LAUNCH(false, false);
#undef GPA_SPARSE_LAUNCH
  HIPCK(hipGetLastError());
  {
    // the chunks its supersteps listed (2^16 or more per segment)
    const int rc = gups_apply_launch();
    if(rc) return rc;
  }
  HIPCK(hipMemcpyAsync(g.h_ctl, g.d_ctl, sizeof(SparseCtl), hipMemcpyDeviceToHost, g.stream));
  HIPCK(hipMemcpyAsync(g.h_sstat, g.d_sstat, sizeof(SpillStat), hipMemcpyDeviceToHost,
    g.stream));
  HIPCK(hipStreamSynchronize(g.stream));
  out = *g.h_ctl;
  g.par = out.par;
  g.sidx += (uint32_t)out.steps;
  g.sparse_launches++;
  g.sparse_steps += out.steps;
  return 0;
}

// Pending mail now (all ranks).
int pending_now(unsigned long long& out)
{
  int rc = pend_clear(kPendPre, 1);
  if(rc) return rc;
  rc = launch_pending(kPendPre);
  if(rc) return rc;
  std::vector<unsigned long long> pv;
  rc = pend_read(kPendPre, 1, pv);
  if(rc) return rc;
  out = pv[0];
  return 0;
}

// Zone overflow left by the last operation: grow the zones and land the
// spilled records. One rank decides from its own status. With n_ranks > 1 the
// decision is this status summed over ranks (k_spill_local + pend_read, a
// collective every rank makes at the same point), so all ranks run
// fixup_spill — and clear their spill flags — together or none does.
// This rank's spill status into pend[first + n - 1] (k_spill_local) and its
// SpillStat into h_sstat, then pend[first .. first + n) summed over ranks
// (pend_read: the collective, which also synchronises the stream).
int spill_sum_read(uint32_t first, uint32_t n, std::vector<unsigned long long>& pv)
{
  hipLaunchKernelGGL(k_spill_local, dim3(1), dim3(1), 0, g.stream, g.d_pend + first + n - 1);
  HIPCK(hipGetLastError());
  HIPCK(hipMemcpyAsync(g.h_sstat, g.d_sstat, sizeof(SpillStat), hipMemcpyDeviceToHost,
    g.stream));
  return pend_read(first, n, pv);
}

int settle_spills()
{
  if(R() == 1)
  {
    // (nothing ran since the last read: it stands)
    if(g.sstat_epoch == g.dev_epoch) return spill_pending() ? fixup_spill() : 0;
    const int rc = read_sstat();
    if(rc) return rc;
    return spill_pending() ? fixup_spill() : 0;
  }
  std::vector<unsigned long long> pv;
  const int rc = spill_sum_read(kPendPre, 1, pv);
  if(rc) return rc;
  return pv[0] ? fixup_spill() : 0;
}

// The scheduler loop to quiescence (or max_steps); caller holds gp.mu.
// One rank: chunks of kChunk k_step launches with one readback each, or
// k_sparse launches while few records are pending. A zone that overflowed
// halts the steps after it on the device; the host then grows the zones
// (fixup_spill) and resumes from the first step that did not run.
int run_locked(uint64_t max_steps, uint64_t* steps_done)
{
  if(!g.init) return GPU_ACTOR_ESTATE;
  if(rank_without_actors()) return GPU_ACTOR_EINVAL;
  {
    const int frc = observe();
    if(frc) return frc;
  }
  uint64_t done = 0;
  if(g.n_zones)
  {
    int rc = settle_spills();
    if(rc) return rc;
    unsigned long long before = 0;
    rc = pending_now(before);
    if(rc) return rc;
    std::vector<unsigned long long> pv;
    std::vector<uint32_t> par_at(kChunk + 1), sidx_at(kChunk + 1);
    const bool sp = sparse_ok();
    while(before > 0 && (max_steps == 0 || done < max_steps))
    {
      if(sp && before <= kSpCap)
      {
        // few messages in flight: whole supersteps in one workgroup until the
        // world is quiet, max_steps, or a step needs the zone path
        SparseCtl c;
        rc = run_sparse(max_steps ? max_steps - done : 0, c);
        if(rc) return rc;
        done += c.steps;
        if(spill_pending())
        {
          rc = fixup_spill();
          if(rc) return rc;
          rc = pending_now(before);
          if(rc) return rc;
          continue;
        }
        if(c.reason == SP_QUIESCENT) { before = 0; break; }
        if(c.reason == SP_MAX_STEPS) break;
        if(c.steps && c.pending == 0xFFFFFFFFFFFFFFFFull)
        {
          // the last step overflowed the list: count what is pending
          rc = pending_now(before);
          if(rc) return rc;
          if(before == 0) break;
        }
        if(max_steps && done >= max_steps) break;
        // SP_DENSE: the next steps go through k_step (at least one chunk)
      }
      uint32_t k = kChunk;
      if(max_steps) k = (uint32_t)std::min<uint64_t>(k, max_steps - done);
      // pend[j] = pending at the start of step j (k_step), pend[k] = after the
      // chunk, pend[k + 1] the spill status below (its shards cleared too: a
      // run_fixed before may have added to them)
      rc = pend_clear(0, k + 2);
      if(rc) return rc;
      for(uint32_t j = 0; j < k; ++j)
      {
        par_at[j] = g.par;
        sidx_at[j] = g.sidx;
        rc = launch_step(j);
        if(rc) return rc;
      }
      par_at[k] = g.par;
      rc = launch_pending(k);
      if(rc) return rc;
      // pend[k + 1]: the spill status, summed over ranks with the counts, so
      // every rank takes the same branch below (one rank: its own status)
      rc = spill_sum_read(0, k + 2, pv);
      if(rc) return rc;
      uint32_t j = 0;
      bool halted = false;
      for(; j < k && before > 0; ++j)
      {
        // one rank: a step the overflow halted; n_ranks > 1 re-runs halted
        // steps inside launch_step, so no summed slot reads as skipped
        if(R() == 1 && pv[j] == kPendSkipped) { halted = true; break; }
        ++done;
        before = pv[j + 1];
      }
      if(halted || pv[k + 1] != 0)
      {
        // steps from j on did not run: resume at the parity step j would have read
        if(halted) { g.par = par_at[j]; g.sidx = sidx_at[j]; }
        rc = fixup_spill();
        if(rc) return rc;
        rc = pending_now(before);
        if(rc) return rc;
      }
    }
  }
  g.steps_total += done;
  if(steps_done) *steps_done = done;
  g.host_seq = 0;     // a new host window starts after each run
  return check_sticky();
}

GPU_ACTOR_API int gpu_actor_run(uint64_t max_steps, uint64_t* steps_done)
{
  if(gp.async_busy) return GPU_ACTOR_EBUSY;     // without waiting for the lock it holds
  std::lock_guard<std::mutex> lk(gp.mu);
  if(gp.async_busy) return GPU_ACTOR_EBUSY;
  return run_locked(max_steps, steps_done);
}

GPU_ACTOR_API int gpu_actor_run_async(uint64_t max_steps, gpu_actor_done_fn done, void* ctx)
{
  if(gp.async_busy) return GPU_ACTOR_EBUSY;
  {
    std::lock_guard<std::mutex> lk(gp.mu);
    if(!g.init) return GPU_ACTOR_ESTATE;
    if(gp.async_busy) return GPU_ACTOR_EBUSY;
  }
  join_worker();                      // reap the previous, finished run
  {
  std::lock_guard<std::mutex> lk(gp.mu);
  if(gp.async_busy) return GPU_ACTOR_EBUSY;
  gp.async_busy = true;
  gp.async_started = false;
  gp.async_rc = 0;
  gp.async_steps = 0;
  const int dev = g.device;
  try
  {
    std::lock_guard<std::mutex> wl(gp.wmu);
    gp.worker = std::thread([max_steps, done, ctx, dev]() {
      int rc;
      uint64_t steps = 0;
      {
        std::lock_guard<std::mutex> wl(gp.mu);
        gp.async_started = true;
        rc = hipSetDevice(dev) == hipSuccess ? run_locked(max_steps, &steps) : GPU_ACTOR_EHIP;
        gp.async_rc = rc;
        gp.async_steps = steps;
        gp.async_busy = false;
      }
      // outside the lock: the callback may call back into the library
      if(done) done(ctx, rc, steps);
    });
  }
  catch(...)
  {
    gp.async_busy = false;
    return GPU_ACTOR_ENOMEM;
  }
  }
  // return only once the progress thread holds the lock, so every later call
  // on this library is serialised behind the run it started
  while(!gp.async_started) std::this_thread::yield();
  return 0;
}

GPU_ACTOR_API int gpu_actor_wait(uint64_t* steps_done)
{
  join_worker();
  std::lock_guard<std::mutex> lk(gp.mu);
  if(steps_done) *steps_done = gp.async_steps;
  const int rc = gp.async_rc;
  gp.async_rc = 0;
  return rc;
}

GPU_ACTOR_API int gpu_actor_busy(void)
{
  return gp.async_busy ? 1 : 0;
}

GPU_ACTOR_API int gpu_actor_run_fixed(uint64_t n)
{
  std::lock_guard<std::mutex> lk(gp.mu);
  if(!g.init) return GPU_ACTOR_ESTATE;
  if(n && rank_without_actors()) return GPU_ACTOR_EINVAL;
  {
    const int frc = flush_sends();
    if(frc) return frc;
  }
  if(g.n_zones == 0 || n == 0) return 0;
  // Two events on the engine's stream bracket the n launches: the average
  // step time they give includes each boundary between launches, so it can
  // only overstate the kernel's own duration (events bound to single
  // dispatches slowed those dispatches: r01 measured 94.8 us against a 93.5 us
  // wall step).
  int rc = ensure_events(2);
  if(rc) return rc;
  rc = settle_spills();
  if(rc) return rc;
  // host ports: these steps' messages stay listed on the device until the
  // next call that observes the engine (no wait is added here); their keys
  // tell host_step_room() steps apart, so a list that would span more is
  // collected first
  struct HostDefer {
    HostDefer() { g.host_defer = true; }
    ~HostDefer() { g.host_defer = false; }
  };
  if(g.host_ports)
  {
    if(n > host_step_room()) return GPU_ACTOR_ERANGE;
    if(g.host_dirty && (uint64_t)(g.sidx - g.host_base) + n > host_step_room())
    {
      rc = host_collect();
      if(rc) return rc;
    }
  }
  HostDefer defer;
  uint64_t left = n;
  double ms_total = 0.0;
  while(left)
  {
    // only the slots these launches add to (slot kPendPre is written whole);
    // one rank reads none of them here (its spill status decides), and every
    // reader of a slot clears it first (run, pending_now), so none at all
    if(R() > 1)
    {
      rc = pend_clear(0, (uint32_t)std::min<uint64_t>(left, kPendPre));
      if(rc) return rc;
    }
    const uint32_t par0 = g.par, sidx0 = g.sidx;
    HIPCK(hipEventRecord(g.ev[0], g.stream));
    for(uint64_t j = 0; j < left; ++j)
    {
      rc = launch_step((uint32_t)(j % kPendPre));
      if(rc) return rc;
    }
    HIPCK(hipEventRecord(g.ev[1], g.stream));
    bool any;
    if(R() == 1)
    {
      // the spill status and the counters (for the sticky errors) in one
      // host round trip
      unsigned long long st[ST_COUNT];
      rc = fold_counters(0, 0);
      if(rc) return rc;
      HIPCK(hipMemcpyAsync(st, g.d_stats, sizeof(st), hipMemcpyDeviceToHost, g.stream));
      rc = read_sstat();                    // synchronises the stream
      if(rc) return rc;
      g.sticky_epoch = g.dev_epoch;
      sticky_from(st);
      any = spill_pending();
    }
    else
    {
      // the same decision on every rank (see settle_spills)
      std::vector<unsigned long long> pv;
      rc = spill_sum_read(kPendPre, 1, pv);  // synchronises the stream
      if(rc) return rc;
      any = pv[0] != 0;
    }
    float ms = 0.f;
    HIPCK(hipEventElapsedTime(&ms, g.ev[0], g.ev[1]));
    ms_total += ms;
    if(!any) break;
    // steps after an overflow did not run (one rank): grow, then run them
    const uint64_t skipped = std::min<uint64_t>(g.h_sstat->skipped, left);
    const uint64_t ran = left - skipped;
    if(R() == 1 && skipped)
    {
      g.par = par0 ^ (uint32_t)(ran & 1u);
      g.sidx = sidx0 + (uint32_t)ran;
    }
    rc = fixup_spill();
    if(rc) return rc;
    left = skipped;
  }
  g.last_drain_ms = ms_total / (double)n;
  g.steps_total += n;
  g.host_seq = 0;
  return check_sticky();
}

GPU_ACTOR_API int gpu_actor_sync(void)
{
  std::lock_guard<std::mutex> lk(gp.mu);
  if(!g.init) return GPU_ACTOR_ESTATE;
  {
    const int frc = observe();
    if(frc) return frc;
  }
  HIPCK(hipStreamSynchronize(g.stream));
  return check_sticky();
}

GPU_ACTOR_API int gpu_actor_state_read(uint32_t type_id, uint64_t first, uint64_t n,
  uint64_t* out)
{
  std::lock_guard<std::mutex> lk(gp.mu);
  if(!g.init) return GPU_ACTOR_ESTATE;
  {
    const int frc = observe();
    if(frc) return frc;
  }
  if(type_id >= GPU_ACTOR_MAX_TYPES || !out) return GPU_ACTOR_EINVAL;
  HostType& t = g.types[type_id];
  if(!t.created || first + n > t.lcount) return GPU_ACTOR_EINVAL;
  if(n == 0) return 0;
  // field-major [words][lcount] to [words][n]: one copy (a table type has
  // millions of words and few actors; a copy per word would take minutes)
  if(n == t.lcount)
    HIPCK(hipMemcpyAsync(out, t.d_state, (size_t)t.words * n * sizeof(uint64_t),
      hipMemcpyDeviceToHost, g.stream));
  else
    HIPCK(hipMemcpy2DAsync(out, n * sizeof(uint64_t), t.d_state + first,
      (size_t)t.lcount * sizeof(uint64_t), n * sizeof(uint64_t), t.words, hipMemcpyDeviceToHost,
      g.stream));
  HIPCK(hipStreamSynchronize(g.stream));
  return 0;
}

GPU_ACTOR_API int gpu_actor_state_write(uint32_t type_id, uint64_t first, uint64_t n,
  const uint64_t* in)
{
  std::lock_guard<std::mutex> lk(gp.mu);
  if(!g.init) return GPU_ACTOR_ESTATE;
  {
    const int frc = flush_sends();
    if(frc) return frc;
  }
  if(type_id >= GPU_ACTOR_MAX_TYPES || !in) return GPU_ACTOR_EINVAL;
  HostType& t = g.types[type_id];
  if(!t.created || first + n > t.lcount) return GPU_ACTOR_EINVAL;
  if(n == 0) return 0;
  if(n == t.lcount)
    HIPCK(hipMemcpyAsync(t.d_state, in, (size_t)t.words * n * sizeof(uint64_t),
      hipMemcpyHostToDevice, g.stream));
  else
    HIPCK(hipMemcpy2DAsync(t.d_state + first, (size_t)t.lcount * sizeof(uint64_t), in,
      n * sizeof(uint64_t), n * sizeof(uint64_t), t.words, hipMemcpyHostToDevice, g.stream));
  HIPCK(hipStreamSynchronize(g.stream));
  return 0;
}

GPU_ACTOR_API int gpu_actor_counts(gpu_actor_counts_t* out)
{
  std::lock_guard<std::mutex> lk(gp.mu);
  if(!g.init) return GPU_ACTOR_ESTATE;
  {
    const int frc = observe();
    if(frc) return frc;
  }
  if(!out) return GPU_ACTOR_EINVAL;
  unsigned long long st[ST_COUNT];
  uint64_t gu[3] = {0, 0, 0};
  int rc = R() > 1 ? gups_stat_read(gu) : 0;
  if(rc) return rc;
  rc = pend_clear(kPendPre, 1);
  if(rc) return rc;
  rc = fold_counters(0, 0);
  if(rc) return rc;
  rc = launch_pending(kPendPre);
  if(rc) return rc;
  const unsigned long long* src_stats = g.d_stats;
  if(R() > 1)
  {
    // sum counters and pending over ranks into scratch (pend[0 .. ST_COUNT))
    rc = xc_allreduce_sum(g.d_stats, g.d_pend, ST_COUNT, XC_U64);
    if(rc) return rc;
    rc = xc_allreduce_sum(g.d_pend + kPendPre, g.d_pend + kPendPre, 1, XC_U64);
    if(rc) return rc;
    src_stats = g.d_pend;
  }
  HIPCK(hipMemcpyAsync(st, src_stats, sizeof(st), hipMemcpyDeviceToHost, g.stream));
  unsigned long long pend = 0;
  HIPCK(hipMemcpyAsync(&pend, g.d_pend + kPendPre, sizeof(pend), hipMemcpyDeviceToHost,
    g.stream));
  HIPCK(hipStreamSynchronize(g.stream));
  memset(out, 0, sizeof(*out));
  out->steps = g.steps_total;
  out->delivered = st[ST_DELIVERED];
  out->sent = st[ST_SENT];
  out->pending = pend;
  out->dropped = st[ST_DROPPED] + st[ST_XCHG_OVERFLOW];
  // + the updates k_gups_apply_ranks applied here from peers' chunks
  out->remote = g.remote_total + gu[2];
  out->active = st[ST_ACTIVE];
  for(int t = 0; t < GPU_ACTOR_MAX_TYPES; ++t) out->delivered_by_type[t] = st[ST_BY_TYPE + t];
  out->atomics = st[ST_ATOMICS];
  return 0;
}

GPU_ACTOR_API uint32_t gpu_actor_owner(uint64_t id)
{
  const uint32_t r = g.cfg.n_ranks ? g.cfg.n_ranks : 1;
  return place_owner(r, g.block_bits, id);
}

// ---- placement (include/gpu_actor_place.h) -----------------------------------
GPU_ACTOR_API int gpu_actor_place_blocks(uint32_t block_bits)
{
  std::lock_guard<std::mutex> lk(gp.mu);
  if(block_bits > GPU_ACTOR_PLACE_MAX_BITS) return GPU_ACTOR_EINVAL;
  if(g.init) return GPU_ACTOR_ESTATE;
  gp.place_bits = (int)block_bits;
  return 0;
}

GPU_ACTOR_API int gpu_actor_place_map(uint32_t n_ranks, uint32_t block_bits, uint64_t id,
  uint32_t* rank, uint64_t* slot)
{
  if(n_ranks == 0 || block_bits > GPU_ACTOR_PLACE_MAX_BITS) return GPU_ACTOR_EINVAL;
  if(rank) *rank = place_owner(n_ranks, block_bits, id);
  if(slot) *slot = place_slot(n_ranks, block_bits, id);
  return 0;
}

GPU_ACTOR_API int gpu_actor_place_global(uint32_t n_ranks, uint32_t block_bits, uint32_t rank,
  uint64_t slot, uint64_t* id)
{
  if(n_ranks == 0 || rank >= n_ranks || block_bits > GPU_ACTOR_PLACE_MAX_BITS || !id)
    return GPU_ACTOR_EINVAL;
  *id = place_global(n_ranks, block_bits, rank, slot);
  return 0;
}

GPU_ACTOR_API int gpu_actor_place_below(uint32_t n_ranks, uint32_t block_bits, uint32_t rank,
  uint64_t id, uint64_t* n)
{
  if(n_ranks == 0 || rank >= n_ranks || block_bits > GPU_ACTOR_PLACE_MAX_BITS || !n)
    return GPU_ACTOR_EINVAL;
  *n = place_below(n_ranks, block_bits, rank, id);
  return 0;
}

GPU_ACTOR_API void* gpu_actor_stream(void) { return (void*)g.stream; }

GPU_ACTOR_API double gpu_actor_last_drain_ms(void) { return g.last_drain_ms; }

// ---- messages to the host (include/gpu_actor_host.h) -------------------------
GPU_ACTOR_API int gpu_actor_host_reserve(uint64_t n)
{
  if(gp.async_busy) return GPU_ACTOR_EBUSY;
  std::lock_guard<std::mutex> lk(gp.mu);
  if(!g.init) return GPU_ACTOR_ESTATE;
  if(gp.async_busy) return GPU_ACTOR_EBUSY;
  // (the segments' room, reserve rounded up to kHostShards, is sorted with an int count)
  if(n == 0 || n > (1ull << 30)) return GPU_ACTOR_EINVAL;
  if(n == g.host_reserve && (!g.host_ports || g.host_seg)) return 0;
  int rc = observe();                       // what the old room still holds
  if(rc) return rc;
  const uint64_t old = g.host_reserve;
  g.host_reserve = n;
  if(!g.host_ports) return 0;               // allocated with the first port type
  rc = host_alloc();
  if(rc)
  {
    g.host_reserve = old;
    if(host_alloc() != 0)
    {
      // no room at either size: the device constants must not keep the freed
      // lists (uploaded without ports: span 0), and no step runs until a
      // later gpu_actor_host_reserve succeeds (launch_step)
      (void)upload_types();
      return GPU_ACTOR_ENOMEM;
    }
  }
  const int urc = upload_types();
  return rc ? rc : urc;
}

GPU_ACTOR_API int gpu_actor_recv(gpu_host_msg_t* out, uint64_t cap, uint64_t* n)
{
  std::lock_guard<std::mutex> lk(gp.mu);
  if(!g.init) return GPU_ACTOR_ESTATE;
  if(!n || (cap && !out)) return GPU_ACTOR_EINVAL;
  *n = 0;
  const int rc = observe();
  if(rc) return rc;
  const uint64_t k = std::min<uint64_t>(cap, g.hostq.size() - g.hostq_head);
  if(k) memcpy(out, g.hostq.data() + g.hostq_head, k * sizeof(gpu_host_msg_t));
  g.hostq_head += k;
  if(g.hostq_head == g.hostq.size())
  {
    g.hostq.clear();
    g.hostq_head = 0;
  }
  *n = k;
  return 0;
}

GPU_ACTOR_API int gpu_actor_recv_pending(uint64_t* n)
{
  std::lock_guard<std::mutex> lk(gp.mu);
  if(!g.init) return GPU_ACTOR_ESTATE;
  if(!n) return GPU_ACTOR_EINVAL;
  *n = 0;
  const int rc = observe();
  if(rc) return rc;
  *n = g.hostq.size() - g.hostq_head;
  return 0;
}

GPU_ACTOR_API int gpu_actor_host_notify(gpu_actor_host_fn fn, void* ctx)
{
  std::lock_guard<std::mutex> lk(gp.mu);
  if(!g.init) return GPU_ACTOR_ESTATE;
  g.host_fn = fn;
  g.host_ctx = fn ? ctx : nullptr;
  return 0;
}

// Diagnostic (not in the public header): engine internals for tests.
// out[0] spill fixups, [1] k_sparse launches, [2] supersteps run by k_sparse,
// [3] zone buffer records, [4] spill list capacity, [5] zones.
GPU_ACTOR_API int gpu_actor_debug_info(uint64_t* out, uint64_t n)
{
  std::lock_guard<std::mutex> lk(gp.mu);
  if(!g.init || !out) return GPU_ACTOR_ESTATE;
  // + the trigger counts by step index mod 3 (zone_dev.h: read this step's,
  // add to the next's, clear the one after) and the zone geometry
  unsigned int tn[3] = {0, 0, 0};
  if(g.d_trig_n)
  {
    HIPCK(hipMemcpyAsync(tn, g.d_trig_n, sizeof(tn), hipMemcpyDeviceToHost, g.stream));
    HIPCK(hipStreamSynchronize(g.stream));
  }
  // + [10] hot zones k_hot gave back to k_step after a missed phase, [11]
  // whether k_hot runs in this engine
  uint32_t hb[4] = {0, 0, 0, 0};
  if(g.d_hot)
  {
    HIPCK(hipMemcpyAsync(hb, hot_bar_words(), sizeof(hb), hipMemcpyDeviceToHost, g.stream));
    HIPCK(hipStreamSynchronize(g.stream));
  }
  // + [12] whether the last step ran the module compiled from the programs
  // (jit_host.h), [13] modules built or loaded by this engine
  // + [14] updates k_gups_apply made, [15] the atomics it issued for them
  // (n_ranks > 1: k_gups_apply_ranks', for the updaters this rank owns)
  uint64_t gu[3] = {0, 0, 0};
  {
    const int rc = gups_stat_read(gu);
    if(rc) return rc;
  }
  // + [16] whether cross-rank records go straight into the peers' inboxes
  // + [17] GUPS chunk descriptors received from peers, [18] listed by this
  // rank (n_ranks > 1), [19] this rank's share of gpu_actor_counts' remote
  // from k_gups_apply_ranks: the updates of peers' chunks it applied
  // + [20] zone steps that took the two-pass plan path (zone_dev.h two_pass)
  unsigned long long st[ST_COUNT];
  {
    const int rc = fold_counters(0, 0);
    if(rc) return rc;
  }
  HIPCK(hipMemcpyAsync(st, g.d_stats, sizeof(st), hipMemcpyDeviceToHost, g.stream));
  HIPCK(hipStreamSynchronize(g.stream));
  // + [21] landing records taken from the compact lane (EngDev::landc)
  // + [22] the session's placement (gpu_actor_place_blocks)
  const uint64_t v[23] = {g.fixups, g.sparse_launches, g.sparse_steps, g.zone_records, g.spill_cap,
                          g.n_zones, tn[0], tn[1], tn[2], g.zbits, hb[3], g.hot_on ? 1u : 0u,
                          g.jit_used ? 1u : 0u, g.jit_builds, gu[0], gu[1], g.peer_write ? 1u : 0u,
                          g.gups_in_total, g.gups_out_total, gu[2], st[ST_PLAN_ZONES],
                          st[ST_LAND8], g.block_bits};
  for(uint64_t i = 0; i < n && i < 23; ++i) out[i] = v[i];
  return 0;
}

// Diagnostic (not in the public header): out[0] the buffers of dev_buf.h that
// hold memory in this process, out[1] their bytes. Callable in any state.
GPU_ACTOR_API void gpu_actor_debug_live_buffers(uint64_t out[2])
{
  if(!out) return;
  out[0] = buf_live.count.load();
  out[1] = buf_live.bytes.load();
}

// Diagnostic (not in the public header): compile the step for a program set
// into the code-object cache (jit_host.h) without a device — `nprog` programs,
// types[k] running words[off_k, off_k + lens[k]) (concatenated), at the
// 4096-actor geometry when z12 — so that a later run loads it at once.
// Returns 0, or GPU_ACTOR_EINVAL with hiprtc's log on stderr.
GPU_ACTOR_API int gpu_actor_debug_jit_compile(const uint32_t* types, const uint64_t* words,
  const uint32_t* lens, uint32_t nprog, int z12, const char* arch)
{
  if(!types || !words || !lens || nprog == 0 || nprog > GPU_ACTOR_MAX_TYPES) return GPU_ACTOR_EINVAL;
  std::vector<jit::Prog> progs;
  uint64_t off = 0;
  for(uint32_t k = 0; k < nprog; ++k)
  {
    if(lens[k] <= GPU_ACTOR_PROG_ENTRIES || lens[k] > jit::kMaxWords) return GPU_ACTOR_EINVAL;
    progs.push_back({types[k], std::vector<uint64_t>(words + off, words + off + lens[k])});
    off += lens[k];
  }
  const std::string src = jit::unit_source(progs, z12 != 0);
  const std::string a = arch && *arch ? arch : "gfx950";
  std::string log;
  const std::string co = jit::code_object(src, a, jit::key_of(src, a), log);
  if(co.empty())
  {
    fprintf(stderr, "gpu_actor jit: %s\n", log.c_str());
    return GPU_ACTOR_EINVAL;
  }
  return 0;
}

// Diagnostic (not in the public header): the translation unit jit_host.h
// generates for that program set (jit::unit_source, what hiprtc would
// compile), NUL-terminated into buf[0, cap). Returns the text's length without
// the NUL — when that is >= cap nothing is written: call again with more
// room — or GPU_ACTOR_EINVAL. Needs no device.
GPU_ACTOR_API int64_t gpu_actor_debug_jit_source(const uint32_t* types, const uint64_t* words,
  const uint32_t* lens, uint32_t nprog, int z12, char* buf, uint64_t cap)
{
  if(!types || !words || !lens || nprog == 0 || nprog > GPU_ACTOR_MAX_TYPES) return GPU_ACTOR_EINVAL;
  std::vector<jit::Prog> progs;
  uint64_t off = 0;
  for(uint32_t k = 0; k < nprog; ++k)
  {
    if(lens[k] <= GPU_ACTOR_PROG_ENTRIES || lens[k] > jit::kMaxWords) return GPU_ACTOR_EINVAL;
    progs.push_back({types[k], std::vector<uint64_t>(words + off, words + off + lens[k])});
    off += lens[k];
  }
  const std::string src = jit::unit_source(progs, z12 != 0);
  if(buf && src.size() < cap) memcpy(buf, src.c_str(), src.size() + 1);
  return (int64_t)src.size();
}

// Diagnostic (not in the public header): gpu_actor_debug_jit_compile for the
// any-mix step of a mix of compiled tables (bit per table id, jit_host.h build_mix).
GPU_ACTOR_API int gpu_actor_debug_jit_compile_mix(uint32_t mask, int z12, const char* arch)
{
  if(mask == 0) return GPU_ACTOR_EINVAL;
  const std::string src = jit::mix_source(mask, z12 != 0);
  const std::string a = arch && *arch ? arch : "gfx950";
  std::string log;
  if(jit::code_object(src, a, jit::key_of(src, a), log).empty())
  {
    fprintf(stderr, "gpu_actor jit: %s\n", log.c_str());
    return GPU_ACTOR_EINVAL;
  }
  return 0;
}

// Diagnostic (not in the public header): phase stamps of the last k_step of
// a -DGPA_STAMPS build, [n_zones][kDbgSlots] shader-clock values.
GPU_ACTOR_API int gpu_actor_debug_stamps(uint64_t* out, uint64_t n)
{
  std::lock_guard<std::mutex> lk(gp.mu);
  if(!g.init || !out) return GPU_ACTOR_ESTATE;
  n = std::min<uint64_t>(n, (uint64_t)kMaxZones * kDbgSlots);
  HIPCK(hipMemcpyAsync(out, g.d_dbg, n * sizeof(uint64_t), hipMemcpyDeviceToHost, g.stream));
  HIPCK(hipStreamSynchronize(g.stream));
  return 0;
}

// Diagnostic (not in the public header): the RCCL bodies of the four
// cross-rank collectives (xc_allreduce_sum for u8/u32/u64, xc_alltoall_u64,
// xc_allgather_u64) and a grouped ncclSend/ncclRecv — the calls
// xc_sendrecv makes — run once on a one-rank communicator over this engine's
// device (ncclCommInitAll: no bootstrap), on device buffers in the engine's
// stream, exactly as exchange_step calls them. One rank sums to itself, so
// out[] reads back what went in: out[0..4) the u64 sum, [4..8) u32,
// [8..16) u8, [16] all-to-all, [17] all-gather, [18..22) the self
// send/recv's received words; out[22] = the RCCL version. A one-rank engine
// only (the comm is swapped in for the call); returns GPU_ACTOR_ECOMM with the
// failing call on stderr if RCCL refuses.
GPU_ACTOR_API int gpu_actor_debug_rccl_selftest(uint64_t* out, uint64_t n)
{
  std::lock_guard<std::mutex> lk(gp.mu);
  if(!g.init || !out || n < 23) return GPU_ACTOR_EINVAL;
  if(R() != 1 || g.comm || gp.xp_ar || gp.xp_a2a) return GPU_ACTOR_ESTATE;
  ncclComm_t comm = nullptr;
  int dev = g.device;
  NCCLCK(ncclCommInitAll(&comm, 1, &dev));
  g.comm = comm;
  DevBuf<unsigned long long> d;
  int rc = 0;
  auto run = [&]() -> int {
    HIPCK(d.alloc(64));
    unsigned long long h[64] = {};
    for(int i = 0; i < 4; ++i) h[i] = 0x1000000000ull * (i + 1) + i;           // u64
    uint32_t* h32 = reinterpret_cast<uint32_t*>(h + 4);
    for(int i = 0; i < 4; ++i) h32[i] = 0x10000u * (i + 1) + 7u;               // u32
    uint8_t* h8 = reinterpret_cast<uint8_t*>(h + 8);
    for(int i = 0; i < 64; ++i) h8[i] = (uint8_t)(3 * i + 1);                  // u8
    h[16] = 0xA2A0000000000001ull;                                               // all-to-all
    h[17] = 0xA770000000000002ull;                                               // all-gather
    for(int i = 0; i < 4; ++i) h[24 + i] = 0x5E4D000000000000ull + i;           // send source
    HIPCK(hipMemcpyAsync(d, h, sizeof(h), hipMemcpyHostToDevice, g.stream));
    int r = xc_allreduce_sum(d, d, 4, XC_U64);
    if(!r) r = xc_allreduce_sum(d + 4, d + 4, 8, XC_U32);
    if(!r) r = xc_allreduce_sum(d + 8, d + 8, 64, XC_U8);
    if(!r) r = xc_alltoall_u64(d + 16, d + 32);
    if(!r) r = xc_allgather_u64(d + 17, d + 33);
    if(r) return r;
    NCCLCK(ncclGroupStart());
    NCCLCK(ncclSend(d + 24, 4 * sizeof(unsigned long long), ncclUint8, 0, g.comm, g.stream));
    NCCLCK(ncclRecv(d + 40, 4 * sizeof(unsigned long long), ncclUint8, 0, g.comm, g.stream));
    NCCLCK(ncclGroupEnd());
    HIPCK(hipMemcpyAsync(h, d, sizeof(h), hipMemcpyDeviceToHost, g.stream));
    HIPCK(hipStreamSynchronize(g.stream));
    for(int i = 0; i < 16; ++i) out[i] = h[i];
    out[16] = h[32];
    out[17] = h[33];
    for(int i = 0; i < 4; ++i) out[18 + i] = h[40 + i];
    int ver = 0;
    NCCLCK(ncclGetVersion(&ver));
    out[22] = (uint64_t)ver;
    return 0;
  };
  rc = run();
  d.reset();
  g.comm = nullptr;
  (void)ncclCommDestroy(comm);
  return rc;
}

} // extern "C"
