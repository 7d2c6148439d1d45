// ldsh_kernel.h -- binary16 LDS-resident layered min-sum for short codes:
// lds.hip's lds_decode with two codewords per lane.  Another element type of
// kernel family 7 (as it serves int8 and float), with the half contract of
// DESIGN.md §3 as its arithmetic (pk_f16.h).
//
// What is lds.hip's: the plan and its tables (LdsCode: layers of checks that
// share no variable, the layer-major u16 edge table), the wave-per-workgroup
// launch, one __syncthreads per layer, frame-major input and output.
//
// What is new: codewords 2p (low half) and 2p + 1 (high half) of the batch are
// ONE 32-bit pair.  One wave = PPW pairs, LPP = 64 / PPW lanes per pair; LDS per
// wave is the table, then V[PPW][N] and msg[PPW][E] as uint32_t -- the bytes of
// the float kernel for twice the codewords.  The two halves of a pair can stop
// apart (early termination runs per codeword inside the wave): a stopped half
// is frozen by storing under a per-half mask (pk_f16.h put2; while no pair of
// the wave is half stopped, every store is a plain one), and a pair whose
// halves have both stopped skips the layers.  With an odd batch the last pair's
// high half is loaded as +0, computes, and is never written to global memory.
#pragma once
#include "pk_f16.h"

namespace ldsh {

using namespace pkf16;

struct LdshArgs {
    const uint16_t *llr;      // frame-major [batch][N] binary16
    uint8_t *hard;            // frame-major [batch][N] 0/1, may be null
    uint16_t *soft;           // frame-major [batch][N] binary16, may be null
    const uint16_t *tab;      // [E] layer-major edge -> variable
    const int4 *layers;       // [nl] (edge base, checks, degree, -)
    int nl, n, e, batch, iters;
    int lpp_log2;             // lanes per pair = 1 << lpp_log2
    int early;
    uint32_t beta2;           // RNE16(beta) in both halves
    int32_t *iters_used;
    int tab_bytes;            // LDS bytes of the table, 16-B aligned
};

// one lane per check
template <int D, int A, bool WHOLE>
LDPC_DEV void check(uint32_t *V, uint32_t *msg, const uint16_t *tab, int cnt, uint32_t beta2, uint32_t mask)
{
    uint32_t c[D], av[D];
    int idx[D];
    uint32_t sign = (D & 1) ? SGN2 : 0u;   // only bits 15 and 31 are ever used
    uint32_t m1 = INF2, m2 = INF2;
#pragma unroll
    for (int j = 0; j < D; j++) {
        idx[j] = tab[j * cnt];
        c[j] = pk_sub(V[idx[j]], msg[j * cnt]);
        av[j] = c[j] & ABS2;
        sign ^= c[j];
        const uint32_t t = m1;
        m1 = pk_min(av[j], m1);
        m2 = pk_min(m2, pk_max(av[j], t));
    }
    const uint32_t sum = pk_addu(m1, m2);
#pragma unroll
    for (int j = 0; j < D; j++) {
        const uint32_t r = cst<A>(pk_subu(sum, pk_minu(av[j], m2)), beta2);
        const uint32_t m = with_sign(r, sign ^ c[j]);
        put2<WHOLE>(msg + j * cnt, m, mask);
        put2<WHOLE>(V + idx[j], clamp_v(pk_add(c[j], m)), mask);
    }
}

LDPC_DEV uint32_t swap_pair(uint32_t x)   // quad_perm [1,0,3,2]
{
    return (uint32_t)__builtin_amdgcn_mov_dpp((int)x, 0xB1, 0xF, 0xF, false);
}

// Two lanes per check (SPLIT): lane half h takes edges h, h + 2, ...; the
// partial (min1, min2, sign) of the two lanes are exchanged with one DPP swap
// of neighbouring lanes and merged: min1 = min(a1, b1), min2 = min(a2, b2,
// max(a1, b1)), the sign the XOR of the pairs.  The padding lane of an odd
// degree contributes magnitude +inf (0x7C00) and sign +, and is never stored.
template <int D, int A, bool WHOLE>
LDPC_DEV void check_split(uint32_t *V, uint32_t *msg, const uint16_t *tab, int cnt, int h, uint32_t beta2,
                          uint32_t mask)
{
    constexpr int DH = (D + 1) / 2;
    uint32_t c[DH], av[DH];
    int idx[DH];
    uint32_t sign = 0u;
    uint32_t m1 = INF2, m2 = INF2;
#pragma unroll
    for (int k = 0; k < DH; k++) {
        const int j = 2 * k + h;
        const bool ok = (D % 2 == 0) || k < DH - 1 || h == 0;
        idx[k] = ok ? tab[j * cnt] : 0;
        c[k] = ok ? pk_sub(V[idx[k]], msg[j * cnt]) : 0u;
        av[k] = ok ? (c[k] & ABS2) : INF2;
        sign ^= c[k];
        const uint32_t t = m1;
        m1 = pk_min(av[k], m1);
        m2 = pk_min(m2, pk_max(av[k], t));
    }
    const uint32_t p1 = swap_pair(m1), p2 = swap_pair(m2), ps = swap_pair(sign);
    m2 = pk_min(pk_min(m2, p2), pk_max(m1, p1));
    m1 = pk_min(m1, p1);
    sign ^= ps ^ ((D & 1) ? SGN2 : 0u);
    const uint32_t sum = pk_addu(m1, m2);
#pragma unroll
    for (int k = 0; k < DH; k++) {
        const int j = 2 * k + h;
        const bool ok = (D % 2 == 0) || k < DH - 1 || h == 0;
        const uint32_t r = cst<A>(pk_subu(sum, pk_minu(av[k], m2)), beta2);
        const uint32_t m = with_sign(r, sign ^ c[k]);
        if (ok) {
            put2<WHOLE>(msg + j * cnt, m, mask);
            put2<WHOLE>(V + idx[k], clamp_v(pk_add(c[k], m)), mask);
        }
    }
}

// the checks li, li + LPP, ... of one layer (lane li of its pair)
template <int D, int A, bool SPLIT, bool WHOLE>
LDPC_DEV void layer(uint32_t *V, uint32_t *msg, const uint16_t *tab, int base, int cnt, int li, int lpp,
                    uint32_t beta2, uint32_t mask)
{
    if constexpr (SPLIT) {   // lanes 2i, 2i+1: check i (the two stay together through the loop)
        const int h = li & 1;
        for (int i = li >> 1; i < cnt; i += lpp >> 1)
            check_split<D, A, WHOLE>(V, msg + base + i, tab + base + i, cnt, h, beta2, mask);
    } else {
        for (int i = li; i < cnt; i += lpp) check<D, A, WHOLE>(V, msg + base + i, tab + base + i, cnt, beta2, mask);
    }
}

#define LDPC_LDSH_DEG_CASES(X) \
    X(2) X(3) X(4) X(5) X(6) X(7) X(8) X(9) X(10) X(11) X(12) X(13) X(14) X(15) X(16) X(17) X(18) X(19) \
    X(20) X(21) X(22) X(23) X(24) X(25) X(26) X(27) X(28) X(29) X(30) X(31) X(32)

template <int A, bool SPLIT>
__global__ void __launch_bounds__(64) ldsh_decode(LdshArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = threadIdx.x;
    const int lpp = 1 << a.lpp_log2, ppw = 64 >> a.lpp_log2;
    const int pl = lane >> a.lpp_log2, li = lane & (lpp - 1);
    const int b0 = 2 * (blockIdx.x * ppw + pl);           // the pair's codewords: b0 and b0 + 1
    const bool has0 = b0 < a.batch, has1 = b0 + 1 < a.batch;
    const int N = a.n, E = a.e;
    uint16_t *tab = (uint16_t *)smem;
    uint32_t *Vall = (uint32_t *)(smem + a.tab_bytes);
    uint32_t *V = Vall + (size_t)pl * N;
    uint32_t *msg = Vall + (size_t)ppw * N + (size_t)pl * E;

    {   // the table: 16-B chunks (the device table is padded to tab_bytes)
        const uint4 *g = (const uint4 *)a.tab;
        uint4 *l = (uint4 *)smem;
#pragma unroll 8
        for (int i = lane; i < a.tab_bytes / 16; i += 64) l[i] = g[i];
    }
    // rows b0 and b0 + 1 through the clamp into pairs; a missing row is +0
    const uint16_t *r0 = a.llr + (size_t)b0 * N, *r1 = r0 + N;
    if (has0 && N % 8 == 0 && ((uintptr_t)a.llr & 15) == 0) {
        // 16-B loads when every row starts 16-B aligned (wave-uniform: the caller's
        // buffer needs only 2-byte alignment): 8 elements of each row -> 8 pairs
        const uint4 *g0 = (const uint4 *)r0, *g1 = (const uint4 *)r1;
        uint4 *l = (uint4 *)V;   // (tab_bytes and N * 4 are multiples of 16)
#pragma unroll 4
        for (int i = li; i < N / 8; i += lpp) {
            const uint4 x = g0[i];
            const uint4 y = has1 ? g1[i] : make_uint4(0, 0, 0, 0);
            l[2 * i] = make_uint4(clamp_v((x.x & 0xFFFFu) | (y.x << 16)), clamp_v((x.x >> 16) | (y.x & 0xFFFF0000u)),
                                  clamp_v((x.y & 0xFFFFu) | (y.y << 16)), clamp_v((x.y >> 16) | (y.y & 0xFFFF0000u)));
            l[2 * i + 1] = make_uint4(clamp_v((x.z & 0xFFFFu) | (y.z << 16)), clamp_v((x.z >> 16) | (y.z & 0xFFFF0000u)),
                                      clamp_v((x.w & 0xFFFFu) | (y.w << 16)), clamp_v((x.w >> 16) | (y.w & 0xFFFF0000u)));
        }
    } else if (has0) {
#pragma unroll 8
        for (int i = li; i < N; i += lpp) {
            const uint32_t lo = r0[i], hi = has1 ? r1[i] : 0u;
            V[i] = clamp_v(lo | (hi << 16));
        }
    } else {
        for (int i = li; i < N; i += lpp) V[i] = 0u;
    }
#pragma unroll 8
    for (int i = li; i < E; i += lpp) msg[i] = 0u;
    __syncthreads();

    const unsigned long long gmask = (lpp == 64 ? ~0ull : ((1ull << lpp) - 1)) << (pl * lpp);
    // codewords still decoding; without early termination the pair runs whole
    // (a missing high half computes on +0), with it a missing half counts as stopped
    bool al0 = has0, al1 = a.early ? has1 : has0;
    int it = 0;
    for (; it < a.iters; it++) {
        if (!__builtin_amdgcn_ballot_w64(al0 || al1)) break;   // the wave leaves when all its codewords have stopped
        const uint32_t mask = (al0 ? 0xFFFFu : 0u) | (al1 ? 0xFFFF0000u : 0u);
        // wave-uniform: no pair of this wave has one half stopped and one running, so every store is a whole pair
        const bool whole = !a.early || !__builtin_amdgcn_ballot_w64(al0 != al1);
        for (int l = 0; l < a.nl; l++) {
            const int4 L = a.layers[l];   // wave-uniform
            if (mask) {
                if (whole) {
                    switch (L.z) {
#define X(DD) \
    case DD: layer<DD, A, SPLIT, true>(V, msg, tab, L.x, L.y, li, lpp, a.beta2, mask); break;
                        LDPC_LDSH_DEG_CASES(X)
#undef X
                    default: break;
                    }
                } else {
                    switch (L.z) {
#define X(DD) \
    case DD: layer<DD, A, SPLIT, false>(V, msg, tab, L.x, L.y, li, lpp, a.beta2, mask); break;
                        LDPC_LDSH_DEG_CASES(X)
#undef X
                    default: break;
                    }
                }
            }
            __syncthreads();   // one wave: orders the layer's LDS writes before the next layer's reads
        }
        if (a.early && mask) {
            // syndrome of hard(V) per half over this lane's checks of every layer
            uint32_t bad = 0;
            for (int l = 0; l < a.nl; l++) {
                const int4 L = a.layers[l];
                for (int i = li; i < L.y; i += lpp) {
                    uint32_t par = 0;
                    for (int j = 0; j < L.z; j++) par ^= pos2(V[tab[L.x + j * L.y + i]]);
                    bad |= par;
                }
            }
            const bool bad0 = (__builtin_amdgcn_ballot_w64((bad & 1u) != 0) & gmask) != 0;
            const bool bad1 = (__builtin_amdgcn_ballot_w64((bad & 2u) != 0) & gmask) != 0;
            if (al0 && !bad0) {
                al0 = false;
                if (a.iters_used && li == 0) a.iters_used[b0] = it + 1;
            }
            if (al1 && !bad1) {
                al1 = false;
                if (a.iters_used && li == 0) a.iters_used[b0 + 1] = it + 1;
            }
        }
    }
    if (a.iters_used && li == 0) {   // codewords that never stopped (al1 is never set for a missing row when early)
        if (has0 && al0) a.iters_used[b0] = it;
        if (has1 && al1) a.iters_used[b0 + 1] = it;
    }
    __syncthreads();
    if (!has0) return;
    uint8_t *h0 = a.hard ? a.hard + (size_t)b0 * N : nullptr;
    uint16_t *s0 = a.soft ? a.soft + (size_t)b0 * N : nullptr;
    for (int i = li; i < N; i += lpp) {
        const uint32_t v = V[i], pos = pos2(v);
        if (h0) {
            h0[i] = (uint8_t)(pos & 1u);
            if (has1) h0[N + i] = (uint8_t)(pos >> 1);
        }
        if (s0) {
            s0[i] = (uint16_t)v;
            if (has1) s0[N + i] = (uint16_t)(v >> 16);
        }
    }
}

template <int A, bool SPLIT>
int launch_as(const LdshArgs &a, int blocks, size_t shm, hipStream_t s)
{
    hipLaunchKernelGGL((ldsh_decode<A, SPLIT>), dim3(blocks), dim3(64), shm, s, a);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace ldsh

// ldsh_deg.hip, one object per (algorithm, split) variant: LH_V = algorithm (0 OMS, 1 NMS, 2 MS) + 3 * split
int ldsh_launch_v0(const ldsh::LdshArgs &a, int blocks, size_t shm, hipStream_t s);
int ldsh_launch_v1(const ldsh::LdshArgs &a, int blocks, size_t shm, hipStream_t s);
int ldsh_launch_v2(const ldsh::LdshArgs &a, int blocks, size_t shm, hipStream_t s);
int ldsh_launch_v3(const ldsh::LdshArgs &a, int blocks, size_t shm, hipStream_t s);
int ldsh_launch_v4(const ldsh::LdshArgs &a, int blocks, size_t shm, hipStream_t s);
int ldsh_launch_v5(const ldsh::LdshArgs &a, int blocks, size_t shm, hipStream_t s);
