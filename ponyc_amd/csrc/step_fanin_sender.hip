// k_step for engines whose serial actors all run GPU_ACTOR_HT_FANIN_SENDER (step_tu.h).
#define GPA_STEP_NAME fanin_sender
#define GPA_STEP_HT GPU_ACTOR_HT_FANIN_SENDER
#include "step_tu.h"
