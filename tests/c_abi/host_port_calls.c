/*
 * host_port_calls.c — calls the entry points of include/gpu_actor_host.h the
 * way a compiled Pony program does (test infrastructure, beside
 * pony_ffi_calls.c).
 *
 * The prototypes below are NOT taken from the header: they are the C
 * restatement of pony/gpu_actor/host_port.pony's `use @...` declarations,
 * i.e. what gencall.c emits for a declared FFI call (gencall.c:1179-1198:
 * I32/U64 -> i32/i64 by value, Pointer[A]/struct/tag -> an opaque pointer, a
 * bare lambda -> a C function pointer). tests/test_host_port_abi.py checks
 * them against both the Pony file and the header.
 *
 *   host_port_calls cpu     every entry point before init (no GPU needed)
 */
#include <stdint.h>
#include <stdio.h>
#include <string.h>

/* ---- host_port.pony's declarations, as gencall.c lowers them ---- */
int32_t gpu_actor_host_reserve(uint64_t n);
int32_t gpu_actor_recv(void* out, uint64_t cap, void* n);
int32_t gpu_actor_recv_pending(void* n);
int32_t gpu_actor_host_notify(void (*fn)(void*, void*, uint64_t), void* ctx);

/* GpuHostMsg (host_port.pony) as Pony lays a struct out: its fields in order */
typedef struct pony_gpu_host_msg
{
  uint64_t step;
  uint32_t from;
  uint32_t seq;
  uint32_t to;
  uint32_t behaviour;
  uint64_t arg;
} pony_gpu_host_msg;

#define ESTATE (-6)
static int fails = 0;
#define EXPECT(expr, want) do { long long _v = (long long)(expr); \
  if(_v != (long long)(want)) { fprintf(stderr, "FAIL %s:%d %s = %lld, want %lld\n", \
    __FILE__, __LINE__, #expr, _v, (long long)(want)); ++fails; } } while(0)

/* GpuHostPorts' bare lambda: ctx is the notify actor */
static void on_msgs(void* ctx, void* msgs, uint64_t n)
{
  (void)ctx; (void)msgs; (void)n;
}

static int cpu_mode(void)
{
  uint64_t u = 7;
  pony_gpu_host_msg m[2];
  memset(m, 0, sizeof m);
  EXPECT(sizeof(pony_gpu_host_msg), 32);
  EXPECT(gpu_actor_host_reserve(1024), ESTATE);
  EXPECT(gpu_actor_recv(m, 2, &u), ESTATE);
  EXPECT(gpu_actor_recv_pending(&u), ESTATE);
  EXPECT(gpu_actor_host_notify(on_msgs, NULL), ESTATE);
  EXPECT(gpu_actor_host_notify(NULL, NULL), ESTATE);
  printf("cpu: %s\n", fails ? "FAILED" : "ok");
  return fails ? 1 : 0;
}

int main(int argc, char** argv)
{
  if(argc >= 2 && !strcmp(argv[1], "cpu")) return cpu_mode();
  fprintf(stderr, "usage: %s cpu\n", argv[0]);
  return 64;
}
