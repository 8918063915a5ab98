// k_step for engines whose serial actors all run GPU_ACTOR_HT_PROGRAM (step_tu.h).
#define GPA_STEP_NAME program
#define GPA_STEP_HT GPU_ACTOR_HT_PROGRAM
#include "step_tu.h"
