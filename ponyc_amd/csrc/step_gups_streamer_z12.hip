// k_step<GPU_ACTOR_HT_GUPS_STREAMER> at 4096-actor zones, 1024-thread workgroups (step_tu.h).
#define GPA_STEP_Z12 1
#define GPA_STEP_NAME gups_streamer
#define GPA_STEP_HT GPU_ACTOR_HT_GUPS_STREAMER
#include "step_tu.h"
