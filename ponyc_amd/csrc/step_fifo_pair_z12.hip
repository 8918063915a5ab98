// k_step<kHtFifoPair> at 4096-actor zones, 1024-thread workgroups (step_tu.h).
#define GPA_STEP_Z12 1
#define GPA_STEP_NAME fifo_pair
#define GPA_STEP_HT 64
#include "step_tu.h"
