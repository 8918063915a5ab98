// k_step<-1> at 4096-actor zones, 1024-thread workgroups (step_tu.h).
#define GPA_STEP_Z12 1
#define GPA_STEP_NAME any
#define GPA_STEP_HT -1
#include "step_tu.h"
