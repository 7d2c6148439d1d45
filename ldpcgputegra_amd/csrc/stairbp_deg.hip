// stairbp_deg.hip -- stairbp_decode instantiated for ONE check degree
// (SB_X = info edges per check, set by the Makefile: one object per degree,
// compiled in parallel)
#include "stairbp_kernel.h"

#ifndef SB_X
#error "SB_X (info edges per check: 5, 8, 12, 20, 25 or 28) must be defined"
#endif
#define SB_CAT2(a, b) a##b
#define SB_CAT(a, b) SB_CAT2(a, b)

int SB_CAT(stairbp_launch_x, SB_X)(const stairf_dev::StairfArgs &a, int S, int blocks, hipStream_t s)
{
    return stairbp::launch_x<SB_X>(a, S, blocks, s);
}
