// stairh_kernel.h -- binary16 layered min-sum for staircase (DVB-S2 IRA) codes:
// stairf.hip's kernel with two codewords per lane.  Another element type of
// kernel family 11 (as family 7 serves int8 and float), with the half contract
// of DESIGN.md §3 as its arithmetic.
//
// What is stairf's: the schedule and its tables (StairfCode::d_tab: S
// consecutive checks per group, u16 node-id pairs), the XCD placement, the ring
// of P groups in flight, the DPP chain that passes the intermediate parity value
// from slot to slot.
//
// What is new: a lane holds codewords 2k and 2k + 1 of its wave as ONE 32-bit
// pair (low half: the even codeword), so a wave covers 128 / S codewords x S
// checks and at S = 2 a V piece is again a whole 128-B line.  V is
// V[node][stride] binary16, read and written as those pairs; the messages keep
// the layout [wave][group][edge][slot][pair], one 256-B run per instruction.
// All arithmetic is packed (pk_f16.h): no per-half compare anywhere.
// With early termination the two halves of a lane can differ in being alive:
// then every store is two 16-bit stores, each under its own codeword's flag.
#pragma once
#include "pk_f16.h"
#include "stairf_dev.h"

namespace stairh {

using namespace stairf_dev;
using namespace pkf16;   // the packed helpers of the half contract

struct StairhArgs {
    uint32_t *V;           // V[node][stride] binary16, addressed as pairs
    uint32_t *msg;
    const uint32_t *tab;
    int G, T, stride, iters, x0;
    uint32_t beta2;        // RNE16(beta) in both halves
    const uint8_t *live;   // early termination: codewords still decoding
};

template <int S>
LDPC_DEV uint32_t rot_chain_u(uint32_t t, int step)
{
    // stairf_dev::rot_chain on the pair (lanes outside the row read 0; none is the step's valid slot)
    return (uint32_t)(step == 0 ? __builtin_amdgcn_update_dpp(0, (int)t, 0x100 + S - 1, 0xF, 0xF, true)
                                : __builtin_amdgcn_update_dpp(0, (int)t, 0x111, 0xF, 0xF, true));
}

template <int X, int A, int S, bool ET>
__global__ void __launch_bounds__(64) stairh_decode(StairhArgs a)
{
    constexpr int W = SF<X, S>::W, E = SF<X, S>::E, P = SF<X, S>::P, C = 64 / S;   // C pairs = 2 C codewords
    const int lane = threadIdx.x, slot = lane % S, cwl = lane / S;
    // XCD-aware: the 128 / (4 C) waves whose V pieces (4 C bytes) share a 128-B line run on one XCD
    const int nb = gridDim.x;
    const int wv = (nb % 8 == 0) ? (int)(blockIdx.x % 8) * (nb / 8) + (int)(blockIdx.x / 8) : (int)blockIdx.x;
    // V: wave base (uniform) + u32 byte offset node * stride * 2 + pair (the host
    // keeps (n + 1) * stride * 2 < 2^32); messages: wave base + group (uniform)
    // + lane + edge * 256 (immediate)
    const uint32_t pitch = (uint32_t)a.stride * 2, lv = (uint32_t)cwl * 4, lm = (uint32_t)(slot * C + cwl) * 4;
    char *Vw = (char *)(a.V + (size_t)wv * C);
    char *Mw = (char *)(a.msg + (size_t)wv * a.G * E * 64);
    const uint32_t *tl = a.tab + slot;
    // early termination: a converged codeword's half keeps computing but is not
    // stored; a wave whose codewords have all converged leaves at once
    bool al0 = true, al1 = true;
    if constexpr (ET) {
        const uint8_t *lp = a.live + ((size_t)wv * C + cwl) * 2;
        al0 = lp[0] != 0;
        al1 = lp[1] != 0;
        if (!__any(al0 || al1)) return;
    }
    const int G = a.G;
    const long total = (long)a.iters * G;

    uint32_t id[2 * P][W];
    uint32_t vv[P][X + 1];   // info V, o V
    uint32_t mm[P][E];       // info messages, x message, o message

    auto node = [&](const uint32_t (&ids)[W], int j) -> uint32_t {
        const uint32_t w = ids[j >> 1];
        return (j & 1) ? (w >> 16) : (w & 0xFFFFu);
    };
    auto load_ids = [&](uint32_t (&ids)[W], int gg) {
#pragma unroll
        for (int i = 0; i < W; i++) ids[i] = tl[((size_t)gg * W + i) * S];
    };
    auto vptr = [&](uint32_t nd) -> char * { return Vw + (__umul24(nd, pitch) + lv); };
    auto put = [&](char *p, uint32_t x) {
        if constexpr (ET) {
            if (al0) *(uint16_t *)p = (uint16_t)x;
            if (al1) *(uint16_t *)(p + 2) = (uint16_t)(x >> 16);
        } else {
            *(uint32_t *)p = x;
        }
    };
    auto load_vm = [&](uint32_t (&v)[X + 1], uint32_t (&m)[E], const uint32_t (&ids)[W], int gg) {
#pragma unroll
        for (int j = 0; j < X; j++) v[j] = *(const uint32_t *)vptr(node(ids, j));
        v[X] = *(const uint32_t *)vptr(node(ids, X + 1));
        const char *mg = Mw + (size_t)gg * E * 256 + lm;
#pragma unroll
        for (int j = 0; j < E; j++) m[j] = *(const uint32_t *)(mg + j * 256);
    };

    uint32_t t = *(const uint32_t *)vptr((uint32_t)a.x0);   // check 0's first chain input: its x node's LLR
    auto process = [&](const uint32_t (&v)[X + 1], const uint32_t (&m)[E], const uint32_t (&ids)[W], int gg) {
        const int c = gg * S + slot;
        const bool hasx = c != a.T;                  // the tail check has no x edge
        const bool sto = c >= a.T - 1;               // o edge not read by the next check (or wraps): store it
        uint32_t cv[X], av[X];
        uint32_t m1 = INF2, m2 = INF2;
        // the check's sign starts at D & 1; only bits 15 and 31 of sI are ever used
        uint32_t sI = ((X + 1 + (hasx ? 1 : 0)) & 1) ? SGN2 : 0u;
#pragma unroll
        for (int j = 0; j < X; j++) {
            cv[j] = pk_sub(v[j], m[j]);
            av[j] = pk_abs(cv[j]);
            sI ^= cv[j];
            const uint32_t tt = m1;
            m1 = pk_min(av[j], m1);
            m2 = pk_min(m2, pk_max(av[j], tt));
        }
        const uint32_t co = pk_sub(v[X], m[X + 1]), ao = pk_abs(co);
        const uint32_t mx = hasx ? m[X] : NINF2;     // tail: |c_x| = +inf, sign +
        // the chain: S steps, slot s valid at step s
        uint32_t cx = 0;
#pragma unroll
        for (int s = 0; s < S; s++) {
            const uint32_t cs = pk_sub(rot_chain_u<S>(t, s), mx);
            if (slot == s) cx = cs;
            const uint32_t r = cst<A>(pk_min(m1, pk_abs(cs)), a.beta2);
            t = clamp_v(pk_add(co, with_sign(r, sI ^ cs)));
        }
        const uint32_t ax = pk_abs(cx);
        const uint32_t mo = with_sign(cst<A>(pk_min(m1, ax), a.beta2), sI ^ cx);
        const uint32_t mxn = with_sign(cst<A>(pk_min(m1, ao), a.beta2), sI ^ co);
        // the two smallest magnitudes of the whole check
        uint32_t M1 = pk_min(m1, ax), M2 = pk_min(m2, pk_max(m1, ax));
        {
            const uint32_t tt = M1;
            M1 = pk_min(ao, M1);
            M2 = pk_min(M2, pk_max(ao, tt));
        }
        const uint32_t sum = pk_addu(M1, M2), sx = sI ^ cx ^ co;
        char *mg = Mw + (size_t)gg * E * 256 + lm;
#pragma unroll
        for (int j = 0; j < X; j++) {
            const uint32_t r = cst<A>(pk_subu(sum, pk_minu(av[j], M2)), a.beta2);
            const uint32_t mj = with_sign(r, sx ^ cv[j]);
            put(mg + j * 256, mj);
            put(vptr(node(ids, j)), clamp_v(pk_add(cv[j], mj)));
        }
        put(mg + X * 256, mxn);
        put(mg + (X + 1) * 256, mo);
        if (hasx) put(vptr(node(ids, X)), clamp_v(pk_add(cx, mxn)));
        if (sto) put(vptr(node(ids, X + 1)), clamp_v(pk_add(co, mo)));
    };

    // prologue: ids of groups 0 .. 2P-1, data of groups 0 .. P-1
    int g_p = 0, g_v = P % G, g_i = (2 * P) % G;   // group (mod G) being decoded / loaded / id-loaded
#pragma unroll
    for (int s = 0; s < 2 * P; s++) load_ids(id[s], s % G);
#pragma unroll
    for (int s = 0; s < P; s++) load_vm(vv[s], mm[s], id[s], s % G);
    for (long base = 0; base < total; base += 2 * P) {
#pragma unroll
        for (int s = 0; s < 2 * P; s++) {
            const int k = s % P;
            if (base + s < total) process(vv[k], mm[k], id[s], g_p);
            load_vm(vv[k], mm[k], id[(s + P) % (2 * P)], g_v);
            load_ids(id[s], g_i);
            g_p = g_p + 1 == G ? 0 : g_p + 1;
            g_v = g_v + 1 == G ? 0 : g_v + 1;
            g_i = g_i + 1 == G ? 0 : g_i + 1;
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the prefetches past the end
}

template <int X, int S, bool ET>
int launch_xse(const StairhArgs &a, int blocks, int algo, hipStream_t s)
{
    if (algo == 1)
        hipLaunchKernelGGL((stairh_decode<X, 1, S, ET>), dim3(blocks), dim3(64), 0, s, a);
    else if (algo == 2)
        hipLaunchKernelGGL((stairh_decode<X, 2, S, ET>), dim3(blocks), dim3(64), 0, s, a);
    else
        hipLaunchKernelGGL((stairh_decode<X, 0, S, ET>), dim3(blocks), dim3(64), 0, s, a);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

template <int X, int S>
int launch_xs(const StairhArgs &a, int blocks, int algo, hipStream_t s)
{
    return a.live ? launch_xse<X, S, true>(a, blocks, algo, s) : launch_xse<X, S, false>(a, blocks, algo, s);
}

template <int X>
int launch_x(const StairhArgs &a, int S, int blocks, int algo, hipStream_t s)
{
    return S == 2 ? launch_xs<X, 2>(a, blocks, algo, s)
         : S == 4 ? launch_xs<X, 4>(a, blocks, algo, s)
         : S == 8 ? launch_xs<X, 8>(a, blocks, algo, s)
                  : launch_xs<X, 16>(a, blocks, algo, s);
}

}  // namespace stairh

// stairh_deg.hip, one object per X
int stairh_launch_x5(const stairh::StairhArgs &a, int S, int blocks, int algo, hipStream_t s);
int stairh_launch_x8(const stairh::StairhArgs &a, int S, int blocks, int algo, hipStream_t s);
int stairh_launch_x12(const stairh::StairhArgs &a, int S, int blocks, int algo, hipStream_t s);
int stairh_launch_x20(const stairh::StairhArgs &a, int S, int blocks, int algo, hipStream_t s);
int stairh_launch_x25(const stairh::StairhArgs &a, int S, int blocks, int algo, hipStream_t s);
int stairh_launch_x28(const stairh::StairhArgs &a, int S, int blocks, int algo, hipStream_t s);
