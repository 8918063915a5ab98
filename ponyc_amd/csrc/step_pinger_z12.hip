// k_step<GPU_ACTOR_HT_PINGER> at 4096-actor zones, 1024-thread workgroups (step_tu.h).
#define GPA_STEP_Z12 1
#define GPA_STEP_NAME pinger
#define GPA_STEP_HT GPU_ACTOR_HT_PINGER
#include "step_tu.h"
