/*
 * gpu_actor_host.h — messages from GPU actors to the host (libgpuactor.so).
 *
 * The other half of the boundary in gpu_actor.h: there the host injects
 * messages into the engine; here behaviours send messages out of it. A host
 * port is an actor id that stands for something on the CPU (env.out, a
 * collector, Main): a program's SEND to a port id is a host-bound message,
 * the analogue of pony_sendv towards a CPU actor (actor.c:773-817). The
 * engine collects those messages after the superstep that sent them and
 * hands them to the host in one canonical total order,
 *
 *     (superstep index, sender id, sender sequence number),
 *
 * from which per-pair FIFO and causal order follow; two runs of the same
 * inputs return byte-identical lists. A progress thread forwards them into
 * the CPU runtime the way the ASIO thread delivers its events
 * (asio/event.c:116-135): see gpu_actor_host_notify and INTEGRATION.md.
 *
 * Only GPU_ACTOR_HT_PROGRAM behaviours can address ports; the compiled handler
 * tables cannot. With n_ranks > 1 a host-bound message is collected by the
 * rank whose actor sent it, whatever the port's id: each rank's host receives
 * its own senders' messages, nothing crosses ranks, and the (step, from, seq)
 * key merges the ranks' lists into the single-rank order.
 *
 * Conventions are those of gpu_actor.h: 0 ok, < 0 a GPU_ACTOR_E* code, every
 * entry point returns GPU_ACTOR_ESTATE before gpu_actor_init.
 */
#ifndef GPU_ACTOR_HOST_H
#define GPU_ACTOR_HOST_H

#include "gpu_actor.h"

#if defined(__cplusplus)
extern "C" {
#endif

/* Handler table of a port type: gpu_actor_type_register(type, words >= 1,
 * GPU_ACTOR_HT_HOST_PORT), then gpu_actor_create(type, P, &first) gives P
 * port ids in the ordinary global id space. Ports have no mailbox and never
 * run; their state words are never touched. A SEND to a port counts as sent
 * and, at once, as delivered (and delivered_by_type of the port's type); it
 * is never pending, never mutes its sender, and takes the sender's next
 * sequence number like any other send. gpu_actor_send / gpu_actor_sendv to a
 * port id fail with GPU_ACTOR_EINVAL. */
#define GPU_ACTOR_HT_HOST_PORT  14

/* One host-bound message. */
typedef struct gpu_host_msg_t   /* 32 bytes */
{
  uint64_t step;       /* superstep index (as the step kernels count it: a 32-bit
                          counter since init, so it wraps after 2^32 steps) in
                          which it was sent                               */
  uint32_t from;       /* sender's global actor id                       */
  uint32_t seq;        /* sender's sequence number within that step      */
  uint32_t to;         /* port id                                        */
  uint32_t behaviour;  /* behaviour index of the SEND                    */
  uint64_t arg;        /* its argument                                   */
} gpu_host_msg_t;

/* Device room for n host-bound messages per collection (default
 * GPU_ACTOR_HOST_RESERVE_DEFAULT; 1 <= n <= 2^30). gpu_actor_run and
 * gpu_actor_run_async collect after every superstep, so there n bounds one
 * superstep; gpu_actor_run_fixed(k) adds no host synchronisation and collects
 * at the next call that observes the engine, so its k steps together must
 * fit. Past the room a message is lost: counted in `dropped`, and the run
 * returns GPU_ACTOR_EMAILBOX (the contract of gpu_actor_type_reserve for
 * spawns; compare the unbounded messageq.c:31-59 a CPU actor has). A lost
 * message was sent: it stays counted in `sent`, `delivered` and
 * `delivered_by_type` as well as in `dropped`, so after an overflow
 * `delivered` includes the lost host-bound messages. Which
 * messages of an overfull collection survive is not defined. Anything still
 * on the device is collected first. GPU_ACTOR_EBUSY while an asynchronous run
 * is in flight. */
#define GPU_ACTOR_HOST_RESERVE_DEFAULT (1ull << 20)
GPU_ACTOR_API int gpu_actor_host_reserve(uint64_t n);

/* Collected messages wait in an unbounded host-side queue (the CPU actor's
 * message queue, actor.c:773-817 pony_sendv -> messageq). gpu_actor_recv
 * removes up to `cap` of the oldest into out[], in canonical order, and sets
 * *n; like the other observing calls it first flushes staged host sends and
 * collects what is still on the device. */
GPU_ACTOR_API int gpu_actor_recv(gpu_host_msg_t* out, uint64_t cap, uint64_t* n);

/* Messages gpu_actor_recv would return now, with room for all of them. */
GPU_ACTOR_API int gpu_actor_recv_pending(uint64_t* n);

/* Delivery by callback instead of the queue (the ASIO pattern,
 * asio/event.c:116-135: the runtime's own thread sends the message on): when
 * fn is set, every collection hands its messages to fn, in canonical order,
 * on the thread that runs the steps — the caller's for gpu_actor_run, the
 * progress thread for gpu_actor_run_async — and nothing enters the queue.
 * msgs is valid only during the call. fn runs while the library's lock is
 * held: it MUST NOT call any gpu_actor_* entry point (forward with
 * pony_sendv, or copy, and return). NULL restores the queue. */
typedef void (*gpu_actor_host_fn)(void* ctx, const gpu_host_msg_t* msgs, uint64_t n);
GPU_ACTOR_API int gpu_actor_host_notify(gpu_actor_host_fn fn, void* ctx);

#if defined(__cplusplus)
}
#endif

#endif /* GPU_ACTOR_HOST_H */
