// k_step for engines whose serial actors all run GPU_ACTOR_HT_STORM (step_tu.h).
#define GPA_STEP_NAME storm
#define GPA_STEP_HT GPU_ACTOR_HT_STORM
#include "step_tu.h"
