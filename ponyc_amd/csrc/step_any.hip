// k_step for any mix of handler tables (a switch over the actor's table) (step_tu.h).
#define GPA_STEP_NAME any
#define GPA_STEP_HT -1
#include "step_tu.h"
