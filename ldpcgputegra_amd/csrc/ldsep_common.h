// ldsep_common.h -- what the edge-parallel kernels of family 9 share: the
// float one (ldsep.hip), its binary16 form (ldseph.hip) and its int8 form
// (ldsepi.hip).  The lane mapping
// (8 lanes per check, 8 checks per pass), the compiled (layers, passes) shapes
// that LdsCode::ep_shape indexes, and the lane permutations of the 8-lane
// butterflies.  The per-slot lane table (LdsCode::d_ep_tab) is built by
// ldsep_upload and serves both.
#pragma once
#include <cstdint>

#include "kernels_common.h"

namespace ldsep {

constexpr int EP_G = 8;                 // lanes per check
constexpr int EP_CPP = 64 / EP_G;       // checks per pass
constexpr int EP_WAVES = 4;             // waves per workgroup

// (NL, NP) shapes compiled: layers x passes of 8 checks
struct EpShape {
    int nl, np;
};
constexpr EpShape kEpShapes[] = {{12, 4}, {11, 6}};   // 648x324 (Z = 27), 576x288 (Z = 24)

// lane permutations inside each group of 8 (every lane written: no old value)
LDPC_DEV uint32_t dpp_xor1(uint32_t x) { return __builtin_amdgcn_mov_dpp((int)x, 0xB1, 0xF, 0xF, true); }
LDPC_DEV uint32_t dpp_xor2(uint32_t x) { return __builtin_amdgcn_mov_dpp((int)x, 0x4E, 0xF, 0xF, true); }
LDPC_DEV uint32_t dpp_hmirror(uint32_t x) { return __builtin_amdgcn_mov_dpp((int)x, 0x141, 0xF, 0xF, true); }

}  // namespace ldsep
