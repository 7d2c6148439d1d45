// ldsh_deg.hip -- ldsh_decode (ldsh_kernel.h) instantiated for ONE variant:
// LH_V = algorithm (0 OMS, 1 NMS, 2 plain min-sum) + 3 * (two lanes per check),
// set by the Makefile.  Each variant carries the 31 check degrees; one object
// per variant, compiled in parallel.
#include "ldsh_kernel.h"

#ifndef LH_V
#error "LH_V (0 .. 5: algorithm + 3 * split) must be defined"
#endif
#define LH_CAT2(a, b) a##b
#define LH_CAT(a, b) LH_CAT2(a, b)

int LH_CAT(ldsh_launch_v, LH_V)(const ldsh::LdshArgs &a, int blocks, size_t shm, hipStream_t s)
{
    return ldsh::launch_as<LH_V % 3, (LH_V >= 3)>(a, blocks, shm, s);
}
