// k_step<GPU_ACTOR_HT_PROGRAM> at 4096-actor zones, 1024-thread workgroups (step_tu.h).
#define GPA_STEP_Z12 1
#define GPA_STEP_NAME program
#define GPA_STEP_HT GPU_ACTOR_HT_PROGRAM
#include "step_tu.h"
