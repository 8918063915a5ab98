"""
Messages from GPU actors to CPU actors (include/gpu_actor_host.h): the part
of the gpu_actor package a program uses when its GPU actors report to
`env.out`, a collector or `Main`. A host port is an actor id of the engine
that stands for a CPU actor; a program's SEND to it is the pony_sendv towards
that actor (actor.c:773-817). The engine hands the messages over in one
canonical order, (superstep, sender, sender sequence).

Declared with exact prototypes like gpu_actor.pony's entry points (gencall.c:
1196-1198); every call returns an I32 error code, never a Pony error. Message
arrays cross the FFI as U64 words, four per gpu_host_msg_t (as GpuMsgs packs
gpu_msg_t): step, from | seq << 32, to | behaviour << 32, arg.
"""
use @gpu_actor_host_reserve[I32](n: U64)
use @gpu_actor_recv[I32](out: Pointer[U64] tag, cap: U64, n: Pointer[U64])
use @gpu_actor_recv_pending[I32](n: Pointer[U64])
use @gpu_actor_host_notify[I32](fn: @{(GpuHostNotify, Pointer[U64], U64)},
  ctx: GpuHostNotify)

primitive HtHostPort fun apply(): U32 => 14       // GPU_ACTOR_HT_HOST_PORT

struct GpuHostMsg
  """gpu_host_msg_t: one host-bound message, 32 bytes."""
  var step: U64 = 0
  var from: U32 = 0
  var seq: U32 = 0
  var to: U32 = 0
  var behaviour: U32 = 0
  var arg: U64 = 0

  new create() => None

  new from_words(w0: U64, w1: U64, w2: U64, w3: U64) =>
    step = w0
    from = (w1 and 0xFFFF_FFFF).u32()
    seq = (w1 >> 32).u32()
    to = (w2 and 0xFFFF_FFFF).u32()
    behaviour = (w2 >> 32).u32()
    arg = w3

primitive GpuProgram
  """
  gpu_actor_type_program for callers outside this package (FFI declarations
  are per package; gpu_actor.pony declares the entry point): the behaviours of
  a GPU_ACTOR_HT_PROGRAM type, the only kind of actor that can address ports.
  """
  fun table(): U32 => 12            // GPU_ACTOR_HT_PROGRAM

  fun apply(type_id: U32, code: Array[U64] box): I32 =>
    @gpu_actor_type_program(type_id, code.cpointer(), code.size().u32())

interface tag GpuHostNotify
  """The CPU actor behind the ports: one behaviour call per message."""
  be gpu_host_msg(step: U64, from: U32, seq: U32, to: U32, behaviour: U32, arg: U64)

primitive GpuHostForward
  """
  The callback handed to gpu_actor_host_notify. The library calls it on the
  thread that runs the steps (the progress thread of gpu_actor_run_async),
  with its lock held: it must not call back into gpu_actor_*. Registered with
  the runtime (pony.h:520-528), that thread's behaviour calls below are plain
  pony_sendv from an external thread — the way ASIO delivers its events
  (asio/event.c:116-135). The messages arrive in canonical order, and the
  notify actor's queue keeps it.
  """
  fun apply(): @{(GpuHostNotify, Pointer[U64], U64)} =>
    @{(notify: GpuHostNotify, words: Pointer[U64], n: U64) =>
      @pony_register_thread()
      let a = Array[U64].from_cpointer(words, n.usize() * 4)
      var i: USize = 0
      while i < n.usize() do
        try
          let m = GpuHostMsg.from_words(a(i * 4)?, a((i * 4) + 1)?, a((i * 4) + 2)?,
            a((i * 4) + 3)?)
          notify.gpu_host_msg(m.step, m.from, m.seq, m.to, m.behaviour, m.arg)
        end
        i = i + 1
      end
    }

class GpuHostPorts
  """
  Ports of one type, and the two ways to take their messages: `notify` (each
  message becomes a behaviour call on a CPU actor, from the thread that runs
  the steps) or `recv` (polled from the queue after a run).
  """
  let first: U64
  let count: U64

  new create(type_id: U32, ports: U64) =>
    var f: U64 = 0
    @gpu_actor_type_register(type_id, 1, HtHostPort())
    @gpu_actor_create(type_id, ports, addressof f)
    first = f
    count = ports

  fun port(i: U64): U64 => first + (i % count)

  fun reserve(n: U64): I32 => @gpu_actor_host_reserve(n)

  fun notify(target: GpuHostNotify): I32 =>
    @gpu_actor_host_notify(GpuHostForward(), target)

  fun pending(): U64 =>
    var n: U64 = 0
    @gpu_actor_recv_pending(addressof n)
    n

  fun recv(cap: U64): Array[GpuHostMsg] =>
    """Up to `cap` of the oldest messages, in canonical order."""
    let words = Array[U64].init(0, cap.usize() * 4)
    var n: U64 = 0
    @gpu_actor_recv(words.cpointer(), cap, addressof n)
    let out = Array[GpuHostMsg](n.usize())
    var i: USize = 0
    while i < n.usize() do
      try
        out.push(GpuHostMsg.from_words(words(i * 4)?, words((i * 4) + 1)?,
          words((i * 4) + 2)?, words((i * 4) + 3)?))
      end
      i = i + 1
    end
    out
