"""
GPU actors that report to a CPU actor (include/gpu_actor_host.h). Every
reference example ends this way — a Pinger tells Main, a Spreader prints
through env.out; here 1,024 program actors each send the number they were
given to a host port, and the engine forwards the messages to the Collector
below in canonical order (superstep, sender, sequence). The run is
asynchronous (gpu_actor_run_async): the library's progress thread runs the
steps, and after each one makes a behaviour call per message — the way the
ASIO thread delivers its events (asio/event.c:116-135) — while Main's
scheduler thread stays free; Main hears of the end through gpu_run_done.
"""
use "gpu_actor"

actor Collector is GpuHostNotify
  let _env: Env
  let _expect: U64
  var _n: U64 = 0
  var _sum: U64 = 0

  new create(env: Env, expect: U64) =>
    _env = env
    _expect = expect

  be gpu_host_msg(step: U64, from: U32, seq: U32, to: U32, behaviour: U32, arg: U64) =>
    _n = _n + 1
    _sum = _sum + arg
    if _n == _expect then
      _env.out.print(_n.string() + " reports, sum " + _sum.string())
    end

actor Main is GpuRunNotify
  let _gpu: GpuActors

  new create(env: Env) =>
    let n: U64 = 1024
    _gpu = GpuActors
    // behaviour 0 REPORT(x): SEND port (param 0), behaviour 0, x
    let code = Array[U64].init(0, 16)
    try code(0)? = 16 end
    code.push(0x0B02)              // ldp  r11, param 0
    code.push(0x8B013)             // send r11, 0, r8
    code.push(0)                   // halt
    _gpu.register(0, 8, GpuProgram.table())
    GpuProgram(0, code)
    let first = _gpu.create_actors(0, n)
    let ports = GpuHostPorts(1, 1)
    _gpu.param(0, 0, ports.port(0))
    ports.notify(Collector(env, n))
    let msgs = GpuMsgs(n.usize())
    var i: U64 = 0
    while i < n do
      msgs.push(first + i, 0, i)
      i = i + 1
    end
    _gpu.sendv(msgs)
    _gpu.run_async(this)

  be gpu_run_done(rc: I32, steps: U64) =>
    _gpu.dispose()
