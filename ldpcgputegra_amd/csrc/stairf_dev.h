// stairf_dev.h -- what the two staircase float kernels share on the device
// side: the launch arguments, the per-(X, S) constants and the DPP chain move.
// Included by stairf.hip (min-sum) and the stairbp translation units (belief
// propagation); internal to them.  stairf_et.h has the launch sequence.
#pragma once

#include "stairf.h"

namespace stairf_dev {

struct StairfArgs {
    float *V;
    float *msg;
    const uint32_t *tab;
    int G, T, stride, iters, x0;
    float beta;
    const uint8_t *live;   // early termination: codewords still decoding (stores of the others are off)
};

template <int X, int S>
struct SF {
    static constexpr int W = (X + 3) / 2;   // u32 words of packed u16 node ids per check
    static constexpr int E = X + 2;         // messages per check
    // groups in flight: ring registers 2P * W + P * (2X + 3) stay <= ~180, and
    // S * P <= 48 checks (every DVB-S2 code's hazard distance is >= 51)
    static constexpr int PR = X <= 5 ? 8 : X <= 8 ? 6 : X <= 12 ? 4 : 2;
    static constexpr int P = PR < 48 / S ? PR : 48 / S;
};

inline int s_index(int S) { return S == 2 ? 3 : S == 4 ? 0 : S == 8 ? 1 : 2; }

// chain step `step`: slot `step` reads slot step - 1 of its codeword (row_shr:1),
// slot 0 reads slot S - 1 (row_shl:S-1; the previous group's last check)
template <int S>
LDPC_DEV float rot_chain(float t, int step)
{
    // bound_ctrl: lanes whose source is outside the row read 0 (none of them is
    // the step's valid slot), which lets the move fold into the subtract that
    // consumes it (v_sub_f32_dpp): one dependent instruction less per step
    const int v = __float_as_int(t);
    return __int_as_float(step == 0 ? __builtin_amdgcn_update_dpp(0, v, 0x100 + S - 1, 0xF, 0xF, true)
                                    : __builtin_amdgcn_update_dpp(0, v, 0x111, 0xF, 0xF, true));
}

}  // namespace stairf_dev
