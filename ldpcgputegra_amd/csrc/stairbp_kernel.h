// stairbp_kernel.h -- layered belief propagation (LDPC_ALGO_BP) for staircase
// (DVB-S2 IRA) codes in the shape of stairf.hip: the same V layout, message
// layout [wave][group][edge][slot][cw], u16-pair tables (StairfCode::d_tab),
// XCD placement and DPP chain; the check update is bp_math.h's box-plus, in the
// order of bp_check, so the results equal the host decoder's bit for bit.
//
// A check of degree X + 2 has its edges in table order: X info edges, the x
// edge (the o node of the check before), the o edge.  With t_j = V[v_j] - m_j
// the recursion of bp_check splits along the staircase as min-sum's does:
//   before the chain (one lane per check, independent):
//     F_0 = t_0, F_j = F_{j-1} [+] t_j (j < X);  co = V[o] - m_o
//   the chain, S steps, step s valid in slot s:
//     cs = rot(t) - m_x;  mo = F_{X-1} [+] cs  (= F_X = m'_o);  t = co + mo
//     (t is the new V of the o node: the next check's x input)
//   after the chain (per lane):
//     m'_x = F_{X-1} [+] co;  B = cx [+] co
//     j = X-1 .. 1: m'_j = F_{j-1} [+] B;  B = t_j [+] B;   m'_0 = B
//   the tail check has no x edge: m'_o = F_{X-1} and B starts at co, by
//   selects (an infinite t_x through [+] would turn -0.0 into +0.0).
// Per check 3X - 1 box-plus spread over the S lanes of a group plus the S of
// the chain, which every lane executes.
//
// The kernel is VALU-bound (a box-plus is about 75 instructions, 480 cycles
// for a wave alone on its SIMD), so one group of read-ahead covers HBM
// latency: the loop holds ONE copy of the check body and a plain double buffer
// -- group g + 1's V and messages are in flight while group g is decoded, and
// are turned into t on arrival (the subtract is the buffer rotation).
// The loads of group g + 1 are issued BEFORE group g's V stores (min-sum
// issues those of g + P after them), so groups g and g + 1 -- checks up to
// 2S - 1 apart -- must share no info node: hazard >= 2S.  stairf_upload builds
// a width's table only where min_hazard >= S * SF<X, S>::P, so P >= 2 (asserted
// below) makes every table that is valid for min-sum valid here.
#pragma once
#include "bp_math.h"
#include "stairf_dev.h"

namespace stairbp {

using namespace stairf_dev;

template <int X, int S, bool ET>
__global__ void __launch_bounds__(64) stairbp_decode(StairfArgs a)
{
    constexpr int W = SF<X, S>::W, E = SF<X, S>::E, C = 64 / S;
    // group g + 1 is loaded before group g is stored: needs min_hazard >= 2S, which the tables give for P >= 2
    static_assert(SF<X, S>::P >= 2, "stairbp loads group g + 1 before storing group g: tables must have hazard >= 2S");
    const int lane = threadIdx.x, slot = lane % S, cwl = lane / S;
    // XCD-aware: the 128 / (4 C) waves whose V pieces share a 128-B line run on one XCD
    const int nb = gridDim.x;
    const int wv = (nb % 8 == 0) ? (int)(blockIdx.x % 8) * (nb / 8) + (int)(blockIdx.x / 8) : (int)blockIdx.x;
    // addressing as stairf_decode: V wave base + u32 byte offset node * stride * 4
    // + lane; messages wave base + group + lane + edge * 256
    const uint32_t pitch = (uint32_t)a.stride * 4, lv = (uint32_t)cwl * 4, lm = (uint32_t)(slot * C + cwl) * 4;
    char *Vw = (char *)(a.V + (size_t)wv * C);
    char *Mw = (char *)(a.msg + (size_t)wv * a.G * E * 64);
    const uint32_t *tl = a.tab + slot;
    // early termination: a converged codeword's lanes still execute (they share
    // the wave with live codewords) but store nothing; a wave whose codewords
    // have all converged leaves at once
    const bool alive = !ET || a.live[(size_t)wv * C + cwl];
    if (ET && !__any(alive)) return;
    const int G = a.G;
    const long total = (long)a.iters * G;

    uint32_t idc[W], idn[W], idf[W];   // node ids: the group decoded, the next (its data in flight), the one after
    float nv[X + 1], nm[E];            // in flight: info V, o V; info messages, x message, o message
    float tj[X], F[X];

    auto node = [&](const uint32_t (&ids)[W], int j) -> uint32_t {
        const uint32_t w = ids[j >> 1];
        return (j & 1) ? (w >> 16) : (w & 0xFFFFu);
    };
    auto load_ids = [&](uint32_t (&ids)[W], int gg) {
#pragma unroll
        for (int i = 0; i < W; i++) ids[i] = tl[((size_t)gg * W + i) * S];
    };
    auto vref = [&](uint32_t nd) -> float & { return *(float *)(Vw + (__umul24(nd, pitch) + lv)); };
    auto load_vm = [&](const uint32_t (&ids)[W], int gg) {
#pragma unroll
        for (int j = 0; j < X; j++) nv[j] = vref(node(ids, j));
        nv[X] = vref(node(ids, X + 1));
        const char *mg = Mw + (size_t)gg * E * 256 + lm;
#pragma unroll
        for (int j = 0; j < E; j++) nm[j] = *(const float *)(mg + j * 256);
    };

    float t = vref((uint32_t)a.x0);   // check 0's first chain input: its x node's LLR
    int g_p = 0, g_v = 1 % G, g_i = 2 % G;   // group (mod G) being decoded / loaded / id-loaded
    load_ids(idc, 0);
    load_ids(idn, g_v);
    load_vm(idc, 0);
    for (long i = 0; i < total; i++) {
        // group g_p's data has arrived: t_j, and the buffer is free for group g_v
#pragma unroll
        for (int j = 0; j < X; j++) tj[j] = nv[j] - nm[j];
        const float co = nv[X] - nm[X + 1], mx = nm[X];
        load_vm(idn, g_v);
        load_ids(idf, g_i);

        const int c = g_p * S + slot;
        const bool hasx = c != a.T;      // the tail check has no x edge
        const bool sto = c >= a.T - 1;   // o edge not read by the next check (or wraps): store it
        F[0] = tj[0];
#pragma unroll
        for (int j = 1; j < X; j++) F[j] = bp_boxplus(F[j - 1], tj[j]);
        const float FX = F[X - 1];
        // the chain: S steps, slot s valid at step s
        float cx = 0.0f, mo = 0.0f;
#pragma unroll
        for (int s = 0; s < S; s++) {
            const float cs = rot_chain<S>(t, s) - mx;
            const float bx = bp_boxplus(FX, cs);
            const float ms = hasx ? bx : FX;
            t = co + ms;
            if (slot == s) {
                cx = cs;
                mo = ms;
            }
        }
        const float mxn = bp_boxplus(FX, co);
        const float bxo = bp_boxplus(cx, co);
        float B = hasx ? bxo : co;
        char *mg = Mw + (size_t)g_p * E * 256 + lm;
        if (alive) {
            *(float *)(mg + X * 256) = mxn;
            *(float *)(mg + (X + 1) * 256) = mo;
            if (hasx) vref(node(idc, X)) = cx + mxn;
            if (sto) vref(node(idc, X + 1)) = co + mo;
        }
#pragma unroll
        for (int j = X - 1; j >= 0; j--) {
            float mj = B;
            if (j > 0) {
                mj = bp_boxplus(F[j - 1], B);
                B = bp_boxplus(tj[j], B);
            }
            if (alive) {
                *(float *)(mg + j * 256) = mj;
                vref(node(idc, j)) = tj[j] + mj;
            }
        }
#pragma unroll
        for (int k = 0; k < W; k++) {
            idc[k] = idn[k];
            idn[k] = idf[k];
        }
        g_p = g_v;
        g_v = g_i;
        g_i = g_i + 1 == G ? 0 : g_i + 1;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the prefetch past the end
}

template <int X, int S>
int launch_xs(const StairfArgs &a, int blocks, hipStream_t s)
{
    if (a.live)
        hipLaunchKernelGGL((stairbp_decode<X, S, true>), dim3(blocks), dim3(64), 0, s, a);
    else
        hipLaunchKernelGGL((stairbp_decode<X, S, false>), dim3(blocks), dim3(64), 0, s, a);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

template <int X>
int launch_x(const StairfArgs &a, int S, int blocks, hipStream_t s)
{
    return S == 2 ? launch_xs<X, 2>(a, blocks, s)
         : S == 4 ? launch_xs<X, 4>(a, blocks, s)
         : S == 8 ? launch_xs<X, 8>(a, blocks, s)
                  : launch_xs<X, 16>(a, blocks, s);
}

}  // namespace stairbp

// one object per X (stairbp_deg.hip)
int stairbp_launch_x5(const stairf_dev::StairfArgs &a, int S, int blocks, hipStream_t s);
int stairbp_launch_x8(const stairf_dev::StairfArgs &a, int S, int blocks, hipStream_t s);
int stairbp_launch_x12(const stairf_dev::StairfArgs &a, int S, int blocks, hipStream_t s);
int stairbp_launch_x20(const stairf_dev::StairfArgs &a, int S, int blocks, hipStream_t s);
int stairbp_launch_x25(const stairf_dev::StairfArgs &a, int S, int blocks, hipStream_t s);
int stairbp_launch_x28(const stairf_dev::StairfArgs &a, int S, int blocks, hipStream_t s);
