// ldsepi.hip -- the int8 form of ldsep.hip: edge-parallel layered min-sum for
// short quasi-cyclic codes with two codewords per lane, in the reference's own
// fixed-point arithmetic.  The int8 element type of kernel family 9, behind
// ldpc_ctx_set_i8_edge_parallel, bit for bit lds_check_i8 (lds.hip) and the
// oracle inside the domain ldsepi_params_ok states.
//
// What is ldseph.hip's: codewords 2p (low half) and 2p + 1 (high half) of the
// batch are ONE 32-bit pair and one wave decodes one pair; EP_WAVES waves per
// workgroup and no workgroup barrier; V in LDS as (n + 2) pairs per wave; the
// table LdsCode::d_ep_tab unchanged (byte offsets of 4-byte elements: a pair);
// off[NS] and msg[NS] in VGPRs for the whole decode, the (layer, pass) slots
// unrolled; the exclusive-min and sign butterflies over the 8 lanes of a check;
// the per-half freeze of early termination.
//
// Number form: plain sign-extended i16 halves, not pk16.h's R / C form (value
// in the high byte).  R / C gives the upper int8 saturation for free (one
// v_pk_min_i16 less per contribution and per new V), but (a) the padding lanes
// below are settled by per-lane clamp bounds, which needs that min / max pair
// anyway; (b) NMS's (min * f) >> 5 and the unsigned offset subtraction want the
// magnitude as a plain integer, two conversions per edge in R / C; (c) input,
// hard and soft bytes are a sign extension / a truncation away.  The per-edge
// functions and the argument why i16 is exact are in pk_i8.h.
//
// Per edge, with l the layer (pk_i8.h):
//   c  = contribution(V, m, hi, lo)           max(sat8(V - m), var_min)
//   a  = magnitude(c, x_l, y_l)               first group min(|c|, msg_max), later |min(c, msg_max)|
//   e  = exclusive minimum of a over the check's 8 lanes (v_pk_min_i16 + DPP);
//        it equals a == min1 ? min2 : min1 of the serial decode, ties included
//   r  = cst_oms(e) / cst_nms(e)
//   m' = message(r, parity ^ c)               parity: XOR butterfly of the c pairs (bits 15 / 31)
//   V' = new_v(c, m', lo)                     max(sat8(c + m'), var_min)
// The later-group rule is wave-uniform per layer (a bit mask in the arguments,
// all zero for NMS, which never uses it), so x_l / y_l are scalar selects.
//
// Padding lanes and empty slots.  ldseph pads a check of degree d < 8 with
// lanes that load a -inf sink.  An int8 sink cannot survive the contract's own
// clamps: max(., var_min) would shrink it to |var_min| (below live magnitudes
// for var_min = -64, non-negative for var_min = 0) and the later-group rule
// puts it through min(c, msg_max) as well.  Chosen here: a padding lane does not
// depend on what it loads.  A layer has one check degree d_l (the plan's layers
// are runs of one degree group), so lane j of a group of 8 pads exactly when
// j >= d_l: one compare per layer, and such a lane takes hi = lo = -127 and
// y = 127, which makes its contribution the constant -127 for every accepted
// parameter set and under both rules: magnitude |min(-127, x)| = 127, what
// min1 = min2 = 127 initialises to, and a negative sign, the D & 1 flip (8 - d
// and d have equal parity).  Nothing has to survive the stores of a layer: the
// padding lanes' V' = max(min(-127 + m', 127), -127) <= 0 lands in V[N], which
// only padding lanes load, and no re-arming store is needed.  The lanes of an
// empty check slot all address V[N + 1]: they compute on whatever it holds
// (bounded i16 values, no traps), write only it, and their 8 equal loads give
// the syndrome butterfly parity 0.  V[N] never holds a positive value (start 0,
// then the <= 0 above), so a padding lane never sets a syndrome bit either.
//
// Early termination (template parameter ET), as ldseph: after every iteration
// the syndrome of pos2(V) per half by the XOR butterfly over all slots; a half
// whose syndrome is zero records its iters_used and is frozen by a per-half
// mask on the stores; the wave leaves when both halves have stopped; the
// missing half of a lone last pair is loaded as 0, counts as stopped and is
// never written to global memory.
//
// Buffers: input, hard and soft rows are bytes at any alignment (byte loads and
// stores), rows beyond the batch are never touched, iters_used may be null.  A
// raw LLR of -128 stays in V until the variable's first update (its first
// contribution is max(-128, var_min)); with 0 iterations the input comes back
// unchanged.  The error count of a decode is not fused (dispatch.hip runs the
// separate count for int8): the epilogue has no workgroup barrier to reduce on.
#include "ldsep_common.h"
#include "lds.h"
#include "pk_i8.h"

namespace {

using namespace ldsep;
using namespace pki8;

struct EpiArgs {
    const int8_t *llr;      // frame-major [batch][N]
    uint8_t *hard;          // frame-major [batch][N], may be null
    int8_t *soft;           // frame-major [batch][N], may be null
    const uint32_t *tab;    // [NL * NP][64]: LDS byte offset of lane's variable in V (sinks N, N+1)
    int n, vstride, batch, iters;
    uint32_t vmin2, mmax2;  // var_min / msg_max in both halves
    uint32_t par2;          // OMS / MS: the offset, NMS: the factor mod 2^16, in both halves
    uint32_t later;         // bit l: layer l is of a later degree group (0 for NMS)
    unsigned long long degs;   // 4 bits per layer: its check degree
    int32_t *iters_used;
};

template <int NL, int NP, bool NMS, bool ET>
__global__ void __launch_bounds__(64 * EP_WAVES) ldsepi_decode(EpiArgs a)
{
    constexpr int NS = NL * NP;
    extern __shared__ __attribute__((aligned(16))) uint32_t epi_smem[];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const int b0 = 2 * ((int)blockIdx.x * EP_WAVES + wave);   // the pair's codewords: b0 and b0 + 1
    if (b0 >= a.batch) return;                                // (no workgroup barrier anywhere)
    const bool has1 = b0 + 1 < a.batch;
    const int N = a.n;
    const int j = lane & (EP_G - 1);   // this lane's edge of its check
    const uint32_t vbase = (uint32_t)wave * (uint32_t)a.vstride * 4u;
    uint32_t *V = epi_smem + (size_t)wave * a.vstride;
    char *L = (char *)epi_smem;
    uint32_t off[NS];   // LDS byte address of this lane's variable per (layer, pass)
    uint32_t msg[NS];
#pragma unroll
    for (int s = 0; s < NS; s++) {
        off[s] = a.tab[s * 64 + lane] + vbase;
        msg[s] = 0u;
    }
    // rows b0 and b0 + 1 sign-extended into pairs; a missing row is 0
    const int8_t *r0 = a.llr + (size_t)b0 * N, *r1 = r0 + N;
    for (int i = lane; i < N; i += 64) V[i] = pair(r0[i], has1 ? r1[i] : 0);
    if (lane < 2) V[N + lane] = 0u;
    // codewords still decoding (wave-uniform); a missing half counts as stopped
    bool al0 = true, al1 = has1;
    int it = 0;
    for (; it < a.iters; it++) {
        if (ET && !(al0 || al1)) break;
        const uint32_t mask = (al0 ? 0xFFFFu : 0u) | (al1 ? 0xFFFF0000u : 0u);
#pragma unroll
        for (int l = 0; l < NL; l++) {
            // the layer's rule and this lane's bounds (header comment: padding lanes)
            const bool later = !NMS && ((a.later >> l) & 1u) != 0;
            const bool pad = j >= (int)((a.degs >> (4 * l)) & 15u);
            const uint32_t hi = pad ? KN127 : K127, lo = pad ? KN127 : a.vmin2;
            const uint32_t x = mag_x(later, a.mmax2), y = pad ? K127 : mag_y(later, a.mmax2);
            uint32_t v[NP];
#pragma unroll
            for (int p = 0; p < NP; p++) v[p] = *(const uint32_t *)(L + off[l * NP + p]);
#pragma unroll
            for (int p = 0; p < NP; p++) {
                const int s = l * NP + p;
                const uint32_t c = contribution(v[p], msg[s], hi, lo);
                const uint32_t aj = magnitude(c, x, y);
                // the minimum over the OTHER 7 lanes of the check per half: mm = the
                // min of this lane's group, e = the min of its group without itself
                uint32_t e = dpp_xor1(aj);
                uint32_t mm = pk_min(aj, e);
                const uint32_t q = dpp_xor2(mm);
                e = pk_min(e, q);
                mm = pk_min(mm, q);
                e = pk_min(e, dpp_hmirror(mm));
                // parity of the 8 lanes' sign bits (the padding lanes' -127: the D & 1 flip)
                uint32_t sg = c ^ dpp_xor1(c);
                sg ^= dpp_xor2(sg);
                sg ^= dpp_hmirror(sg);
                const uint32_t r = NMS ? cst_nms(e, a.par2) : cst_oms(e, a.par2, a.mmax2);
                const uint32_t m = message(r, sg ^ c);
                msg[s] = m;
                const uint32_t nv = new_v(c, m, lo);
                v[p] = ET ? ((nv & mask) | (v[p] & ~mask)) : nv;
            }
#pragma unroll
            for (int p = 0; p < NP; p++) *(uint32_t *)(L + off[l * NP + p]) = v[p];
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
    int8_t *s0 = a.soft ? a.soft + (size_t)b0 * N : nullptr;
    for (int i = lane; i < N; i += 64) {
        const uint32_t xv = V[i], pos = pos2(xv);
        if (h0) {
            h0[i] = (uint8_t)(pos & 1u);
            if (has1) h0[N + i] = (uint8_t)(pos >> 1);
        }
        if (s0) {
            s0[i] = (int8_t)half_lo(xv);
            if (has1) s0[N + i] = (int8_t)half_hi(xv);
        }
    }
}

template <int NL, int NP>
void launch_shape(const EpiArgs &a, bool nms, bool early, dim3 grid, dim3 block, size_t shm, hipStream_t s)
{
    switch ((nms ? 2 : 0) + (early ? 1 : 0)) {
    case 0: hipLaunchKernelGGL((ldsepi_decode<NL, NP, false, false>), grid, block, shm, s, a); break;
    case 1: hipLaunchKernelGGL((ldsepi_decode<NL, NP, false, true>), grid, block, shm, s, a); break;
    case 2: hipLaunchKernelGGL((ldsepi_decode<NL, NP, true, false>), grid, block, shm, s, a); break;
    default: hipLaunchKernelGGL((ldsepi_decode<NL, NP, true, true>), grid, block, shm, s, a); break;
    }
}

}  // namespace

// the domain of the kernel: the int8 ranges check_params admits, less var_min = -128
// (abs8(-128) = -128 would turn a magnitude negative)
bool ldsepi_params_ok(const ldpc_params *p)
{
    if (p->algo != LDPC_ALGO_OMS && p->algo != LDPC_ALGO_NMS && p->algo != LDPC_ALGO_MS) return false;
    if (p->var_max != 127 || p->var_min < -127 || p->var_min > 0) return false;
    if (p->msg_max < 0 || p->msg_max > 127) return false;
    return p->algo != LDPC_ALGO_OMS || (p->offset >= 0 && p->offset <= 255);
}

extern "C" int ldpc_ldsepi_params_ok(const ldpc_params *p, int *ok)
{
    if (!p || !ok) return ldpc_set_error(LDPC_EINVAL, "NULL");
    *ok = ldsepi_params_ok(p) ? 1 : 0;
    return LDPC_OK;
}

// V is (n + 2) 32-bit pairs per wave: the bytes of the float kernel's codeword, so its LDS predicate holds as it is
bool ldsepi_applicable(const ldpc_code *h, const LdsCode &lc) { return ldsep_applicable(h, lc, true); }

int launch_ldsepi(const LdsCode &lc, const ldpc_code *h, const int8_t *llr, uint8_t *hard, int8_t *soft,
                  const DecodeLaunch &L, hipStream_t s)
{
    if (!ldsepi_applicable(h, lc) || L.batch <= 0) return -1;
    const bool nms = L.algo == 1;
    EpiArgs a{};
    a.llr = llr;
    a.hard = hard;
    a.soft = soft;
    a.tab = lc.d_ep_tab;
    a.n = h->n;
    a.vstride = (h->n + 2 + 3) / 4 * 4;
    a.batch = L.batch;
    a.iters = L.iters;
    a.vmin2 = splat(L.var_min);
    a.mmax2 = splat(L.msg_max);
    a.par2 = splat(nms ? (L.param & 0xFFFF) : (L.param & 0xFF));
    a.later = nms ? 0u : lc.ep_later;
    a.degs = lc.ep_degs;
    a.iters_used = L.iters_used;
    const int pairs = (L.batch + 1) / 2;
    const size_t shm = (size_t)EP_WAVES * a.vstride * 4;
    const dim3 grid((pairs + EP_WAVES - 1) / EP_WAVES), block(64 * EP_WAVES);
    static_assert(sizeof(kEpShapes) / sizeof(kEpShapes[0]) == 2 && kEpShapes[0].nl == 12 && kEpShapes[0].np == 4 &&
                  kEpShapes[1].nl == 11 && kEpShapes[1].np == 6, "the instantiations below follow the shape list");
    switch (lc.ep_shape) {
    case 0: launch_shape<12, 4>(a, nms, L.early != 0, grid, block, shm, s); break;
    case 1: launch_shape<11, 6>(a, nms, L.early != 0, grid, block, shm, s); break;
    default: return -1;
    }
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
