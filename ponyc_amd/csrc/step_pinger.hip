// k_step for engines whose serial actors all run GPU_ACTOR_HT_PINGER (step_tu.h).
#define GPA_STEP_NAME pinger
#define GPA_STEP_HT GPU_ACTOR_HT_PINGER
#include "step_tu.h"
