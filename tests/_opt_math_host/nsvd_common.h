// Host stand-in for csrc/nsvd_common.h: lets g++ compile csrc/opt_math.h (copied beside this file by
// tests/test_optim_host.py) so that the optimiser rules' float32 arithmetic and the double-precision schedule run on
// the CPU. Only what opt_math.h uses.
#pragma once
#include <math.h>
#include <stdint.h>
#include <stddef.h>
#include "nsvd.h"
#define __device__
#define __forceinline__ inline
