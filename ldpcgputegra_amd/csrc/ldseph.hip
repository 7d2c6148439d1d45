// ldseph.hip -- the binary16 form of ldsep.hip: edge-parallel layered min-sum
// for short quasi-cyclic codes with two codewords per lane.  Another element
// type of kernel family 9, behind ldpc_ctx_set_f16_edge_parallel, with the half
// contract of DESIGN.md §3 as its arithmetic (pk_f16.h).
//
// What is ldsep.hip's (ldsep_common.h): the shape list, the table
// LdsCode::d_ep_tab as ldsep_upload built it (byte offsets of 4-byte elements:
// here a 32-bit pair), 8 lanes per check, 8 checks per pass, the (layer, pass)
// slots unrolled, each lane's messages in VGPRs for the whole decode, the
// exclusive-min and sign butterflies over the 8 lanes.
//
// What is new: codewords 2p (low half) and 2p + 1 (high half) of the batch are
// ONE 32-bit pair and one wave decodes one pair, so a workgroup of EP_WAVES
// waves holds 8 codewords in the LDS bytes the float kernel needs for 4.
// * c = V (-) m per half; the magnitudes c & ABS2 order as packed u16, so the
//   exclusive-min butterfly runs on v_pk_min_u16 (the DPP move is an
//   instruction of its own: VOP3P takes no DPP operand); its result E is
//   exactly a_j == min1 ? min2 : min1 of the serial decode;
// * the sign of a contribution is its sign bit: the parity of a check is the
//   XOR butterfly of the pairs themselves (bits 15 and 31 are the only ones
//   used), the message cst(E) with the bits parity ^ own sign inserted;
// * V = clamp_v(c (+) m').  No "+ 0.0" on load: -0.0 is a negative
//   contribution here as in the host decoder, so the kernel equals the host
//   decoder bit for bit, the sign of a zero soft value included.
//
// The sinks.  A check of degree d < 8 pads its group with lanes that read the
// sink V[N] = -inf in both halves: +inf never wins a minimum and the sign bit
// of each padding lane supplies the contract's D & 1 flip (8 - d and d have the
// same parity); the lanes of an empty check slot read the second sink V[N + 1],
// which no live check reads.  A padding lane's own update is
// clamp_v(-inf (+) m') = -1024, and it stores it like every lane, which would
// leave a finite sink for the next layer.  Chosen here: the sinks are RE-ARMED,
// lanes 0 and 1 store -inf to V[N] and V[N + 1] after the stores of every layer.
// It is exact because (a) all loads of a layer precede all its stores (the
// layer's checks share no variable, the sinks are the only address two lanes
// write), so inside a layer every padding lane has read -inf already; (b) the
// LDS executes one wave's instructions in order, so the re-arming store lands
// after the padding lanes' and before the next layer's loads; (c) a padding
// lane's contribution is then -inf (-) m = -inf for every finite m (|m| <= 256),
// whatever it stored before.  The alternatives cost more: a clamp that spares
// the sinks is a select per edge, a store destination nobody reads a second
// offset table (NS more VGPRs); the re-arm is one masked LDS store per layer.
// An empty slot computes on -inf alone (cst(+inf) = 256, or NaN for NMS with
// beta 0) and touches V[N + 1] only.
//
// Early termination (template parameter ET; without it no mask code exists):
// after every iteration the syndrome of pos2(V) per half by the same 8-lane XOR
// butterfly over all slots (the sinks read -inf: never 1).  A half whose
// syndrome is zero records its iters_used and is frozen: from then on the
// stores keep the old value of that half (one v_bfi with the loaded pair under
// a wave-uniform per-half mask; the lane that loaded a variable is the only one
// that stores it).  The wave leaves when both halves have stopped; the missing
// half of a lone last pair is loaded as +0, counts as stopped, and is never
// written to global memory.
#include "ldsep_common.h"
#include "ldsh.h"
#include "pk_f16.h"

namespace {

using namespace ldsep;
using namespace pkf16;

struct EphArgs {
    const uint16_t *llr;    // frame-major [batch][N] binary16
    uint8_t *hard;          // frame-major [batch][N], may be null
    uint16_t *soft;         // frame-major [batch][N] binary16, may be null
    const uint32_t *tab;    // [NL * NP][64]: LDS byte offset of lane's variable in V (sinks N, N+1)
    int n, vstride, batch, iters;
    uint32_t beta2;         // RNE16(beta) in both halves
    int32_t *iters_used;
};

// A: 0 OMS, 1 NMS, 2 plain min-sum (pk_f16.h cst)
template <int NL, int NP, int A, bool ET>
__global__ void __launch_bounds__(64 * EP_WAVES) ldseph_decode(EphArgs a)
{
    constexpr int NS = NL * NP;
    extern __shared__ __attribute__((aligned(16))) uint32_t eph_smem[];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const int b0 = 2 * ((int)blockIdx.x * EP_WAVES + wave);   // the pair's codewords: b0 and b0 + 1
    if (b0 >= a.batch) return;                                // (no workgroup barrier anywhere)
    const bool has1 = b0 + 1 < a.batch;
    const int N = a.n;
    const uint32_t vbase = (uint32_t)wave * (uint32_t)a.vstride * 4u;
    uint32_t *V = eph_smem + (size_t)wave * a.vstride;
    char *L = (char *)eph_smem;
    uint32_t off[NS];   // LDS byte address of this lane's variable per (layer, pass)
    uint32_t msg[NS];
#pragma unroll
    for (int s = 0; s < NS; s++) {
        off[s] = a.tab[s * 64 + lane] + vbase;
        msg[s] = 0u;
    }
    // rows b0 and b0 + 1 through the clamp into pairs; a missing row is +0
    const uint16_t *r0 = a.llr + (size_t)b0 * N, *r1 = r0 + N;
    for (int i = lane; i < N; i += 64) {
        const uint32_t lo = r0[i], hi = has1 ? r1[i] : 0u;
        V[i] = clamp_v(lo | (hi << 16));
    }
    if (lane < 2) V[N + lane] = NINF2;
    // codewords still decoding (wave-uniform); a missing half counts as stopped
    bool al0 = true, al1 = has1;
    int it = 0;
    for (; it < a.iters; it++) {
        if (ET && !(al0 || al1)) break;
        const uint32_t mask = (al0 ? 0xFFFFu : 0u) | (al1 ? 0xFFFF0000u : 0u);
#pragma unroll
        for (int l = 0; l < NL; l++) {
            uint32_t v[NP];
#pragma unroll
            for (int p = 0; p < NP; p++) v[p] = *(const uint32_t *)(L + off[l * NP + p]);
#pragma unroll
            for (int p = 0; p < NP; p++) {
                const int s = l * NP + p;
                const uint32_t c = pk_sub(v[p], msg[s]);
                const uint32_t aj = c & ABS2;
                // the minimum over the OTHER 7 lanes of the check per half: mm = the
                // min of this lane's group, e = the min of its group without itself
                uint32_t e = dpp_xor1(aj);
                uint32_t mm = pk_minu(aj, e);
                const uint32_t q = dpp_xor2(mm);
                e = pk_minu(e, q);
                mm = pk_minu(mm, q);
                e = pk_minu(e, dpp_hmirror(mm));
                // parity of the 8 lanes' sign bits (the padding lanes' -inf: the D & 1 flip)
                uint32_t sg = c ^ dpp_xor1(c);
                sg ^= dpp_xor2(sg);
                sg ^= dpp_hmirror(sg);
                // cst of the others' minimum.  Plain min-sum: e is a magnitude (sign bits clear,
                // never NaN in a live check), so min(e, 256) as packed u16 is cst<2>'s value and
                // spares the canonicalising v_pk_max_f16 the float min needs on an integer result
                const uint32_t r = A == 2 ? pk_minu(e, MSAT2) : cst<A>(e, a.beta2);
                const uint32_t m = with_sign(r, sg ^ c);
                msg[s] = m;
                const uint32_t x = clamp_v(pk_add(c, m));
                v[p] = ET ? ((x & mask) | (v[p] & ~mask)) : x;
            }
#pragma unroll
            for (int p = 0; p < NP; p++) *(uint32_t *)(L + off[l * NP + p]) = v[p];
            if (lane < 2) V[N + lane] = NINF2;   // re-arm the sinks (header comment)
        }
        if (ET) {
            uint32_t bad = 0;
#pragma unroll
            for (int s = 0; s < NS; s++) {
                uint32_t h = pos2(*(const uint32_t *)(L + off[s]));
                h ^= dpp_xor1(h);
                h ^= dpp_xor2(h);
                h ^= dpp_hmirror(h);
                bad |= h;
            }
            const bool bad0 = __builtin_amdgcn_ballot_w64((bad & 1u) != 0) != 0;
            const bool bad1 = __builtin_amdgcn_ballot_w64((bad & 2u) != 0) != 0;
            if (al0 && !bad0) {
                al0 = false;
                if (a.iters_used && lane == 0) a.iters_used[b0] = it + 1;
            }
            if (al1 && !bad1) {
                al1 = false;
                if (a.iters_used && lane == 0) a.iters_used[b0 + 1] = it + 1;
            }
        }
    }
    if (a.iters_used && lane == 0) {   // codewords that never stopped
        if (al0) a.iters_used[b0] = it;
        if (al1) a.iters_used[b0 + 1] = it;
    }
    uint8_t *h0 = a.hard ? a.hard + (size_t)b0 * N : nullptr;
    uint16_t *s0 = a.soft ? a.soft + (size_t)b0 * N : nullptr;
    for (int i = lane; i < N; i += 64) {
        const uint32_t x = V[i], pos = pos2(x);
        if (h0) {
            h0[i] = (uint8_t)(pos & 1u);
            if (has1) h0[N + i] = (uint8_t)(pos >> 1);
        }
        if (s0) {
            s0[i] = (uint16_t)x;
            if (has1) s0[N + i] = (uint16_t)(x >> 16);
        }
    }
}

uint32_t half_bits(float x)
{
    const _Float16 v = (_Float16)x;   // round to nearest even
    return (uint32_t)__builtin_bit_cast(uint16_t, v);
}

template <int NL, int NP>
void launch_shape(const EphArgs &a, int algo, bool early, dim3 grid, dim3 block, size_t shm, hipStream_t s)
{
    switch (algo * 2 + (early ? 1 : 0)) {
    case 0: hipLaunchKernelGGL((ldseph_decode<NL, NP, 0, false>), grid, block, shm, s, a); break;
    case 1: hipLaunchKernelGGL((ldseph_decode<NL, NP, 0, true>), grid, block, shm, s, a); break;
    case 2: hipLaunchKernelGGL((ldseph_decode<NL, NP, 1, false>), grid, block, shm, s, a); break;
    case 3: hipLaunchKernelGGL((ldseph_decode<NL, NP, 1, true>), grid, block, shm, s, a); break;
    case 4: hipLaunchKernelGGL((ldseph_decode<NL, NP, 2, false>), grid, block, shm, s, a); break;
    default: hipLaunchKernelGGL((ldseph_decode<NL, NP, 2, true>), grid, block, shm, s, a); break;
    }
}

}  // namespace

// V is (n + 2) 32-bit pairs per wave: the bytes of the float kernel's codeword, so its LDS predicate holds as it is
bool ldseph_applicable(const ldpc_code *h, const LdsCode &lc) { return ldsep_applicable(h, lc, true); }

int launch_ldseph(const LdsCode &lc, const ldpc_code *h, const uint16_t *llr, uint8_t *hard, uint16_t *soft,
                  const DecodeLaunch &L, hipStream_t s)
{
    if (!ldseph_applicable(h, lc) || L.batch <= 0) return -1;
    EphArgs a{};
    a.llr = llr;
    a.hard = hard;
    a.soft = soft;
    a.tab = lc.d_ep_tab;
    a.n = h->n;
    a.vstride = (h->n + 2 + 3) / 4 * 4;
    a.batch = L.batch;
    a.iters = L.iters;
    const uint32_t b16 = half_bits(L.beta) & 0x7FFFu;   // (-0.0 is +0)
    a.beta2 = b16 | (b16 << 16);
    a.iters_used = L.iters_used;
    const int algo = L.algo == 1 ? 1 : b16 == 0 ? 2 : 0;
    const int pairs = (L.batch + 1) / 2;
    const size_t shm = (size_t)EP_WAVES * a.vstride * 4;
    const dim3 grid((pairs + EP_WAVES - 1) / EP_WAVES), block(64 * EP_WAVES);
    static_assert(sizeof(kEpShapes) / sizeof(kEpShapes[0]) == 2 && kEpShapes[0].nl == 12 && kEpShapes[0].np == 4 &&
                  kEpShapes[1].nl == 11 && kEpShapes[1].np == 6, "the instantiations below follow the shape list");
    switch (lc.ep_shape) {
    case 0: launch_shape<12, 4>(a, algo, L.early != 0, grid, block, shm, s); break;
    case 1: launch_shape<11, 6>(a, algo, L.early != 0, grid, block, shm, s); break;
    default: return -1;
    }
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
