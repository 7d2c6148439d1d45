// stairbp.hip -- belief propagation on the float staircase kernel: the launch
// of stairbp_decode (stairbp_kernel.h, one object per degree from
// stairbp_deg.hip) and its group-width rule.  Host code only.
#include <cmath>

#include "stairbp_kernel.h"
#include "stairf_et.h"

// Group width of a BP launch.  Min-sum picks S by HBM behaviour; BP is
// VALU-bound and every lane executes the S chain steps of its group, so an
// iteration costs (M / S) groups x (3X - 1 + S) box-plus x f(w), where f says
// what sharing a CU costs a wave: w = stride * S / 64 / 256 waves per CU,
// f = 1 up to two waves and (w / 2)^(5/8) beyond.  Measured (DVB-S2 r1/2, 20
// iterations, tools/bp_stair_rate.py), S = 2 / 4 / 8 / 16, to three digits: a
// lone wave runs a box-plus in about 480 cycles, latency-bound, and
//   batch  1024 (w = S / 16): 997 / 557 / 376 / 251 ms    f = 1 throughout
//   batch  4096 (w = S / 4):  996 / 561 / 384 / 392       f(4) = 1.56
//   batch 16384 (w = S):      1020 / 860 / 841 / 950      f(4), f(8), f(16) = 1.54, 2.24, 3.78
// against (w / 2)^(5/8) = 1.54, 2.38, 3.67.  (A model of whole rounds of the
// chip's 1024 SIMDs at one wave each picks 16 and 4 at the two larger batches
// and loses to 8 by 2 % each time.)  f is fitted to r1/2 alone; the other codes
// take it unmeasured.  The width with the least cost wins, the wider one on a
// tie.  widths: bit S set = the code has that table.
int stairbp_model_width(int X, int m, int stride, unsigned widths)
{
    int best = 0;
    double best_cost = 0.0;
    for (int S : {16, 8, 4, 2}) {
        if (!(widths & (unsigned)S) || m % S) continue;
        const double w = (double)stride * S / 64.0 / 256.0;
        const double cost = (double)(m / S) * (3 * X - 1 + S) * (w > 2.0 ? std::pow(w / 2.0, 0.625) : 1.0);
        if (!best || cost < best_cost) {
            best = S;
            best_cost = cost;
        }
    }
    return best;
}

extern "C" int ldpc_bp_staircase_width_model(int x, int m, int stride, unsigned widths)
{
    return stairbp_model_width(x, m, stride, widths);
}

int launch_stairbp(const DecodeLaunch &L, const StairfCode &sc, hipStream_t s)
{
    using namespace stairf_dev;
    if (!stairf_stride_ok(sc, L.n, L.stride) || L.vpitch != L.stride) return -1;
    if (L.early && (!L.live || !L.bad || !L.iters_used || !L.d_edge_var)) return -1;
    const int S = stairf_width(sc, L.stride, true);
    if (!S) return -1;
    const int blocks = L.stride / (64 / S);
    auto run = [&](const StairfArgs &a) {
        switch (sc.X) {
        case 5: return stairbp_launch_x5(a, S, blocks, s);
        case 8: return stairbp_launch_x8(a, S, blocks, s);
        case 12: return stairbp_launch_x12(a, S, blocks, s);
        case 20: return stairbp_launch_x20(a, S, blocks, s);
        case 25: return stairbp_launch_x25(a, S, blocks, s);
        case 28: return stairbp_launch_x28(a, S, blocks, s);
        }
        return -1;
    };
    return run_decode(L, sc, make_args(L, sc, S), s, run);
}
