"""The run-time compiled step's generated C++ (csrc/jit_host.h prog_function),
run on the host: the `jit_prog_<type>` functions are cut out of the
translation unit that ponyc_amd.engine.jit_source returns and compiled with the
host C++ compiler against the shim below, which stands in for the device side
they call into. The executable handles one superstep's jobs per call (the
interface of prog_model.ModelExec), so prog_model.World can drive it in the
model's place: labels, jump targets, entry dispatch and step counting are then
checked with no GPU. A plain executable: no sanitizer, nothing preloaded."""
from __future__ import annotations

import os
import re
import shutil
import struct
import subprocess

SHIM = r"""
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>
#define __device__
#define __forceinline__ inline
enum { ST_DROPPED = 0 };
struct TypeDev { uint64_t params[8]; };
struct Eng { uint64_t n_ids; unsigned long long stats[1]; };
static Eng c_eng;
struct Msg { uint64_t to, beh, arg; };
struct Ctx {
  uint64_t self; uint32_t type;
  std::vector<Msg> sends, spawns;
  int yields;
};
static inline unsigned long long atomicAdd(unsigned long long* p, unsigned long long v)
{ const unsigned long long o = *p; *p += v; return o; }
static inline uint64_t __umul64hi(uint64_t a, uint64_t b)
{ return (uint64_t)(((unsigned __int128)a * b) >> 64); }
// GPU_ACTOR_OP_MIX as include/gpu_actor.h states it
static inline uint64_t splitmix_mix(uint64_t x)
{
  uint64_t z = x + 0x9e3779b97f4a7c15ull;
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}
template <class A> void send_serial(A& a, uint32_t to, uint32_t beh, uint64_t arg)
{ a.sends.push_back({to, beh, arg}); }
template <class A> void spawn_actor(A& a, uint32_t type, uint32_t beh, uint64_t arg)
{ a.spawns.push_back({type, beh, arg}); }
template <class A> void actor_yield(A& a) { a.yields++; }

//@FUNCTIONS@

static uint64_t rd(FILE* f)
{
  uint64_t v;
  if(fread(&v, 8, 1, f) != 1) { fprintf(stderr, "short input\n"); exit(2); }
  return v;
}
static void wr(FILE* f, uint64_t v) { fwrite(&v, 8, 1, f); }

// in:  n_ids, 16 x 8 params, n_jobs, per job: type, self, state[8], n_msgs, (beh, arg)...
// out: per job: state[8], handled, dropped, n_sends, (to, beh, arg)..., n_spawns, (type, beh, arg)...
int main(int argc, char** argv)
{
  if(argc != 3) return 2;
  FILE* in = fopen(argv[1], "rb");
  FILE* out = fopen(argv[2], "wb");
  if(!in || !out) return 2;
  c_eng.n_ids = rd(in);
  static TypeDev types[16];
  for(int t = 0; t < 16; ++t) for(int k = 0; k < 8; ++k) types[t].params[k] = rd(in);
  const uint64_t jobs = rd(in);
  for(uint64_t j = 0; j < jobs; ++j)
  {
    Ctx a;
    a.type = (uint32_t)rd(in);
    a.self = rd(in);
    a.yields = 0;
    uint64_t s[8];
    for(int k = 0; k < 8; ++k) s[k] = rd(in);
    const uint64_t n = rd(in);
    uint64_t handled = 0;
    c_eng.stats[ST_DROPPED] = 0;
    for(uint64_t m = 0; m < n; ++m)
    {
      const uint32_t beh = (uint32_t)rd(in);
      const uint64_t arg = rd(in);
      if(a.yields) continue;            // (the rest of the input is still consumed)
      ++handled;
      const TypeDev& T = types[a.type & 15];
      switch(a.type)
      {
//@DISPATCH@
        default: fprintf(stderr, "no program for type %u\n", a.type); return 2;
      }
    }
    for(int k = 0; k < 8; ++k) wr(out, s[k]);
    wr(out, handled);
    wr(out, c_eng.stats[ST_DROPPED]);
    wr(out, a.sends.size());
    for(const Msg& m : a.sends) { wr(out, m.to); wr(out, m.beh); wr(out, m.arg); }
    wr(out, a.spawns.size());
    for(const Msg& m : a.spawns) { wr(out, m.to); wr(out, m.beh); wr(out, m.arg); }
  }
  fclose(out);
  return 0;
}
"""


def compiler():
    for c in (os.environ.get("CXX"), "c++", "g++", "clang++",
              os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "clang++")):
        if c and shutil.which(c):
            return shutil.which(c)
    return None


def extract_functions(src: str) -> dict:
    """{type id: text} of the jit_prog_<type> functions in a generated unit."""
    out = {}
    for m in re.finditer(r"template <class A>\n__device__ __forceinline__ void jit_prog_(\d+)\(.*?\n}\n",
                         src, re.S):
        out[int(m.group(1))] = m.group(0)
    return out


def build(progs, workdir: str, name: str) -> str:
    """Compile the generated functions of `progs` ([(type id, words)]) with
    the shim; returns the executable's path."""
    from ponyc_amd.engine import jit_source
    fns = extract_functions(jit_source(progs, False))
    assert sorted(fns) == sorted(t for t, _ in progs), (sorted(fns), [t for t, _ in progs])
    dispatch = "".join(f"        case {t}: jit_prog_{t}(T, a, s, beh, arg); break;\n" for t in sorted(fns))
    text = SHIM.replace("//@FUNCTIONS@", "\n".join(fns[t] for t in sorted(fns))).replace("//@DISPATCH@", dispatch)
    cpp, exe = os.path.join(workdir, name + ".cpp"), os.path.join(workdir, name)
    with open(cpp, "w") as f:
        f.write(text)
    subprocess.run([compiler(), "-std=c++17", "-O0", "-w", "-o", exe, cpp], check=True)
    return exe


class HostJitExec:
    """prog_model.ModelExec's interface over the host-compiled functions.
    Types without a program (a compiled table the model restates) stay on
    the model."""

    def __init__(self, exe: str, workdir: str):
        self.exe, self.workdir = exe, workdir

    def step(self, world, jobs):
        import prog_model as M
        mine = [j for j in jobs if world.types[j[0]].table is None]
        other = [j for j in jobs if world.types[j[0]].table is not None]
        buf = [struct.pack("<Q", world.n_ids)]
        for t in range(16):
            params = world.types[t].params if t < len(world.types) else [0] * 8
            buf.append(struct.pack("<8Q", *params))
        buf.append(struct.pack("<Q", len(mine)))
        for ti, a, st, msgs in mine:
            buf.append(struct.pack("<11Q", ti, a, *st, len(msgs)))
            for beh, arg in msgs:
                buf.append(struct.pack("<2Q", beh, arg))
        fin, fout = os.path.join(self.workdir, "jobs.in"), os.path.join(self.workdir, "jobs.out")
        with open(fin, "wb") as f:
            f.write(b"".join(buf))
        subprocess.run([self.exe, fin, fout], check=True)
        with open(fout, "rb") as f:
            raw = f.read()
        words = struct.unpack(f"<{len(raw) // 8}Q", raw)
        res, p = {}, 0
        for ti, a, _, msgs in mine:
            st = list(words[p:p + 8])
            handled, dropped, ns = words[p + 8:p + 11]
            p += 11
            sends = [tuple(words[p + 3 * k:p + 3 * k + 3]) for k in range(ns)]
            p += 3 * ns
            nsp = words[p]
            p += 1
            if nsp:
                raise NotImplementedError("the driver places no spawned actors")
            res[a] = (st, sends, dropped, handled, [0] * len(msgs))
        assert p == len(words)
        for j, r in zip(other, M.ModelExec().step(world, other)):
            res[j[1]] = r
        return [res[j[1]] for j in jobs]
