// stairh_deg.hip -- stairh_decode instantiated for ONE check degree
// (SH_X = info edges per check, set by the Makefile: one object per degree,
// compiled in parallel)
#include "stairh_kernel.h"

#ifndef SH_X
#error "SH_X (info edges per check: 5, 8, 12, 20, 25 or 28) must be defined"
#endif
#define SH_CAT2(a, b) a##b
#define SH_CAT(a, b) SH_CAT2(a, b)

int SH_CAT(stairh_launch_x, SH_X)(const stairh::StairhArgs &a, int S, int blocks, int algo, hipStream_t s)
{
    return stairh::launch_x<SH_X>(a, S, blocks, algo, s);
}
