// k_step<GPU_ACTOR_HT_FANIN_SENDER> at 4096-actor zones, 1024-thread workgroups (step_tu.h).
#define GPA_STEP_Z12 1
#define GPA_STEP_NAME fanin_sender
#define GPA_STEP_HT GPU_ACTOR_HT_FANIN_SENDER
#include "step_tu.h"
