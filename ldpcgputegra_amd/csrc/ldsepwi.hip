// ldsepwi.hip -- the int8 form of ldsepw.hip: edge-parallel layered min-sum
// with one PAIR of codewords spread over the W = 2 or 4 waves of a workgroup,
// in the reference's own fixed-point arithmetic, for the quasi-cyclic codes
// whose (layer, pass) slots pass what one wave's registers hold: 1944x972,
// 1248x624, 2304x1152 and tables of their shape.  The int8 element type of
// kernel family 9 on those codes, behind ldpc_ctx_set_i8_ep_wide, bit for bit
// lds_check_i8 (lds.hip) and the oracle inside the domain ldsepi_params_ok
// states (tests/test_gpu_i8_ep_wide.py).
//
// What is ldsepw.hip's, unchanged: the plan and the table (LdsCode::epw_*,
// d_epw_tab: byte offsets of 4-byte elements, here a pair); V, N + 2 elements,
// in the workgroup's LDS -- the bytes of ldsepw's float codeword, so its LDS
// predicate holds as it is; wave w takes passes w, w + W, ... of each layer,
// NPW slots per layer and wave, a pass index past the plan's an empty slot on
// V[N + 1]; messages and offsets in VGPRs for the whole decode, the offsets two
// to a register above 72 slots, made opaque by repack(); one __syncthreads()
// after each layer's V writes; amdgpu_waves_per_eu(2); the workgroup-wide
// early-termination word by iteration parity.
//
// What is ldsepi.hip's, unchanged: codewords 2p (low i16 half) and 2p + 1 (high
// half) of the batch are one 32-bit pair, here one workgroup's (grid =
// (batch + 1) / 2); the per-edge functions of pk_i8.h in that kernel's order
// (contribution, magnitude, the pk_min exclusive-minimum butterfly, the XOR sign
// butterfly, cst_oms / cst_nms, message, new_v); the padding-lane rule: lane j
// of a group of 8 pads where j >= the layer's check degree and then takes
// hi = lo = -127, y = 127, a constant contribution of -127 whatever it loads;
// the per-half freeze of early termination; byte rows at any alignment.
//
// Races on the sinks.  Unlike ldsepi, several waves store to V[N] (the padding
// lanes of their checks) and to V[N + 1] (the lanes of their empty check slots)
// inside one layer, unordered.  That is harmless:
// * every store is one aligned 32-bit word, so a load sees some lane's whole
//   value, never a mix of two;
// * every value ever stored to V[N] is <= 0 in both halves: it starts as 0 and
//   a padding lane stores max(min(-127 + m', 127), -127) <= 0, or, for a frozen
//   half, what it loaded from V[N] -- and nothing a padding lane computes
//   depends on what it loads, so the order of those stores changes no result
//   and V[N] never sets a syndrome bit;
// * every value stored to V[N + 1] is a new_v result or a loaded V[N + 1], a
//   clamped i16 (-127 .. 127) per half: the lanes of an empty slot compute on
//   bounded values and write only V[N + 1].  The 8 lanes of an empty check read
//   V[N + 1] in one instruction of one wave, after a barrier that no store
//   follows, so they see one value and their syndrome parity is 0.
//
// Early termination (template parameter ET) is decided per workgroup and frozen
// per half: each wave ORs the pos2 parities of its slots into the LDS word of
// the iteration's parity (bit 0 the low half, bit 1 the high), a barrier, every
// wave reads the same word and derives the same al0 / al1.  A half that stops
// records its iters_used and is masked out of the stores; the workgroup leaves
// when both halves have stopped; the missing half of a lone last pair is loaded
// as 0, counts as stopped and is never written to global memory.
//
// Buffers, as ldsepi: rows beyond the batch are never touched; hard, soft and
// iters_used may be null; a raw LLR of -128 stays in V until the variable's
// first update; 0 iterations return the input unchanged; no fused error count
// (dispatch.hip runs the separate count for int8).
#include <cstdlib>

#include "ldsep_common.h"
#include "lds.h"
#include "pk_i8.h"

namespace {

using namespace ldsep;
using namespace pki8;

// (layers, passes per wave, waves) compiled, the kernel's own list: ldsepw's
// five entries, each at 0 bytes of scratch under the 256-register budget
// (DESIGN.md section 5 has the table)
struct EpwiShape {
    int nl, npw, w;
};
constexpr EpwiShape kEpwiShapes[] = {
    {12, 6, 2}, {12, 3, 4},               // 1944x972 (Z = 81: 11 passes)
    {11, 7, 2}, {11, 4, 4},               // 1248x624 (Z = 104: 13 passes)
    {11, 6, 4},                           // 2304x1152 (Z = 192: 24 passes)
};
constexpr int kEpwiShapeCount = (int)(sizeof(kEpwiShapes) / sizeof(kEpwiShapes[0]));
// the instantiations launch_ldsepwi switches over: kEpwiShapes again, entry by entry
#define EPWI_SHAPES(X) X(0, 12, 6, 2) X(1, 12, 3, 4) X(2, 11, 7, 2) X(3, 11, 4, 4) X(4, 11, 6, 4)
#define EPWI_SAME(i, NL, NPW, W) \
    static_assert(kEpwiShapes[i].nl == NL && kEpwiShapes[i].npw == NPW && kEpwiShapes[i].w == W, "kEpwiShapes vs EPWI_SHAPES");
EPWI_SHAPES(EPWI_SAME)
static_assert(kEpwiShapeCount == 5, "kEpwiShapes vs EPWI_SHAPES");
#undef EPWI_SAME
constexpr int EPWI_MAX_W = 4;

struct EpwiArgs {
    const int8_t *llr;      // frame-major [batch][N]
    uint8_t *hard;          // frame-major [batch][N], may be null
    int8_t *soft;           // frame-major [batch][N], may be null
    const uint32_t *tab;    // [nl * np][64]: LDS byte offset of lane's variable in V (sinks N, N+1)
    int n, np, batch, iters;
    uint32_t vmin2, mmax2;  // var_min / msg_max in both halves
    uint32_t par2;          // OMS / MS: the offset, NMS: the factor mod 2^16, in both halves
    uint32_t later;         // bit l: layer l is of a later degree group (0 for NMS)
    unsigned long long degs;   // 4 bits per layer: its check degree
    int32_t *iters_used;
};

// amdgpu_waves_per_eu(2): a budget of 256 registers, as ldsepw_decode
template <int NL, int NPW, int W, bool NMS, bool ET>
__global__ void __launch_bounds__(64 * W) __attribute__((amdgpu_waves_per_eu(2))) ldsepwi_decode(EpwiArgs a)
{
    constexpr int NS = NL * NPW;
    extern __shared__ __attribute__((aligned(16))) uint32_t epwi_V[];
    __shared__ uint32_t epwi_bad[2];   // early termination: the workgroup's verdict per half (bits 0, 1), by iteration parity
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const int b0 = 2 * (int)blockIdx.x;   // the pair's codewords: b0 (grid = (batch + 1) / 2: always there) and b0 + 1
    const bool has1 = b0 + 1 < a.batch;
    const int N = a.n;
    const int j = lane & (EP_G - 1);   // this lane's edge of its check
    uint32_t *V = epwi_V;
    char *L = (char *)epwi_V;
    // LDS byte address of this lane's variable per (layer, this wave's q-th
    // pass); past 72 slots a wave two offsets share a register as 16-bit halves
    // ((N + 2) * 4 <= 64 KB, ldsepw_plan), as ldsepw.hip
    constexpr bool PACK = NS > 72;
    uint32_t off[PACK ? (NS + 1) / 2 : NS];
    uint32_t msg[NS];
#pragma unroll
    for (int l = 0; l < NL; l++)
#pragma unroll
        for (int q = 0; q < NPW; q++) {
            const int p = q * W + wave;                // wave-uniform
            const int s = l * NPW + q;
            const uint32_t o = p < a.np ? a.tab[(l * a.np + p) * 64 + lane] : (uint32_t)(N + 1) * 4u;
            if (!PACK) off[s] = o;
            else if (s & 1) off[s >> 1] |= o << 16;
            else off[s >> 1] = o;
            msg[s] = 0u;   // CDecoder_OMS_fixed_SSE.cpp:129-131
        }
    auto addr = [&](int s) -> uint32_t {
        return !PACK ? off[s] : (s & 1) ? off[s >> 1] >> 16 : off[s >> 1] & 0xFFFFu;
    };
    // rows b0 and b0 + 1 sign-extended into pairs; a missing row is 0
    const int8_t *r0 = a.llr + (size_t)b0 * N, *r1 = r0 + N;
    for (int i = threadIdx.x; i < N; i += 64 * W) V[i] = pair(r0[i], has1 ? r1[i] : 0);
    if (threadIdx.x < 2) {
        V[N + threadIdx.x] = 0u;
        epwi_bad[threadIdx.x] = 0;
    }
    __syncthreads();
    // codewords still decoding (workgroup-uniform); a missing half counts as stopped
    bool al0 = true, al1 = has1;
    int it = 0;
    // BARRIER INVARIANT: every wave of the workgroup executes the same number
    // of barriers.  The trip count and the break below depend only on kernel
    // arguments, on blockIdx (has1) and on an LDS word all waves read after a
    // barrier (al0 / al1), so they are workgroup-uniform; a wave whose passes
    // are all empty slots still runs every layer and arrives at every barrier;
    // no wave returns before the loop ends.  A wave that left early would leave
    // the others waiting at s_barrier for ever.
    // packed offsets: made opaque before the layers and again before the
    // syndrome pass, else the compiler unpacks every slot once, outside the loop
    // or at the top of an iteration, and keeps all NS unpacked offsets alive
    auto repack = [&]() {
        if (PACK) {
#pragma unroll
            for (int k = 0; k < (NS + 1) / 2; k++) asm volatile("" : "+v"(off[k]));
        }
    };
    while (it < a.iters) {
        if (ET && !(al0 || al1)) break;
        const uint32_t mask = (al0 ? 0xFFFFu : 0u) | (al1 ? 0xFFFF0000u : 0u);
        repack();
#pragma unroll
        for (int l = 0; l < NL; l++) {
            // the layer's rule and this lane's bounds (ldsepi.hip: padding lanes)
            const bool later = !NMS && ((a.later >> l) & 1u) != 0;
            const bool pad = j >= (int)((a.degs >> (4 * l)) & 15u);
            const uint32_t hi = pad ? KN127 : K127, lo = pad ? KN127 : a.vmin2;
            const uint32_t x = mag_x(later, a.mmax2), y = pad ? K127 : mag_y(later, a.mmax2);
            uint32_t v[NPW];
#pragma unroll
            for (int q = 0; q < NPW; q++) v[q] = *(const uint32_t *)(L + addr(l * NPW + q));
#pragma unroll
            for (int q = 0; q < NPW; q++) {
                const int s = l * NPW + q;
                const uint32_t c = contribution(v[q], msg[s], hi, lo);
                const uint32_t aj = magnitude(c, x, y);
                // the minimum over the OTHER 7 lanes of the check per half: ldsepi.hip's exclusive-min butterfly
                uint32_t e = dpp_xor1(aj);
                uint32_t mm = pk_min(aj, e);
                const uint32_t t = dpp_xor2(mm);
                e = pk_min(e, t);
                mm = pk_min(mm, t);
                e = pk_min(e, dpp_hmirror(mm));
                // parity of the 8 lanes' sign bits (the padding lanes' -127: the D & 1 flip)
                uint32_t sg = c ^ dpp_xor1(c);
                sg ^= dpp_xor2(sg);
                sg ^= dpp_hmirror(sg);
                const uint32_t r = NMS ? cst_nms(e, a.par2) : cst_oms(e, a.par2, a.mmax2);
                const uint32_t m = message(r, sg ^ c);
                msg[s] = m;
                const uint32_t nv = new_v(c, m, lo);
                v[q] = ET ? ((nv & mask) | (v[q] & ~mask)) : nv;
            }
#pragma unroll
            for (int q = 0; q < NPW; q++) *(uint32_t *)(L + addr(l * NPW + q)) = v[q];
            // this layer's V writes, of every wave, before the next layer's
            // reads (after the last layer: before the syndrome and the epilogue)
            __syncthreads();
        }
        it++;
        if (ET) {   // syndrome of pos2(V) per half over every check (sinks: header comment)
            uint32_t bad = 0;
            repack();
#pragma unroll
            for (int s = 0; s < NS; s++) {
                uint32_t h = pos2(*(const uint32_t *)(L + addr(s)));
                h ^= dpp_xor1(h);
                h ^= dpp_xor2(h);
                h ^= dpp_hmirror(h);
                bad |= h;
            }
            const uint32_t bits = (__builtin_amdgcn_ballot_w64((bad & 1u) != 0) != 0 ? 1u : 0u) |
                                  (__builtin_amdgcn_ballot_w64((bad & 2u) != 0) != 0 ? 2u : 0u);
            const int par = it & 1;
            if (bits && lane == 0) atomicOr(&epwi_bad[par], bits);
            // the other word is next iteration's: nobody reads it before the
            // barrier below, and its writers come after that barrier
            if (threadIdx.x == 0) epwi_bad[par ^ 1] = 0;
            __syncthreads();
            const uint32_t word = epwi_bad[par];   // the same word for every wave
            if (al0 && !(word & 1u)) {
                al0 = false;
                if (a.iters_used && threadIdx.x == 0) a.iters_used[b0] = it;
            }
            if (al1 && !(word & 2u)) {
                al1 = false;
                if (a.iters_used && threadIdx.x == 0) a.iters_used[b0 + 1] = it;
            }
        }
    }
    if (a.iters_used && threadIdx.x == 0) {   // codewords that never stopped
        if (al0) a.iters_used[b0] = it;
        if (al1) a.iters_used[b0 + 1] = it;
    }
    uint8_t *h0 = a.hard ? a.hard + (size_t)b0 * N : nullptr;
    int8_t *s0 = a.soft ? a.soft + (size_t)b0 * N : nullptr;
    for (int i = threadIdx.x; i < N; i += 64 * W) {
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

// index into kEpwiShapes of the entry that runs (nl, np) on w waves, -1 if none
int shape_of(int nl, int np, int w)
{
    int best = -1;
    for (int i = 0; i < kEpwiShapeCount; i++) {
        const EpwiShape &s = kEpwiShapes[i];
        if (s.nl == nl && s.w == w && s.w * s.npw >= np && (best < 0 || s.npw < kEpwiShapes[best].npw)) best = i;
    }
    return best;
}

template <int NL, int NPW, int W>
void launch_shape(const EpwiArgs &a, bool nms, bool early, dim3 grid, dim3 block, size_t shm, hipStream_t s)
{
    switch ((nms ? 2 : 0) + (early ? 1 : 0)) {
    case 0: hipLaunchKernelGGL((ldsepwi_decode<NL, NPW, W, false, false>), grid, block, shm, s, a); break;
    case 1: hipLaunchKernelGGL((ldsepwi_decode<NL, NPW, W, false, true>), grid, block, shm, s, a); break;
    case 2: hipLaunchKernelGGL((ldsepwi_decode<NL, NPW, W, true, false>), grid, block, shm, s, a); break;
    default: hipLaunchKernelGGL((ldsepwi_decode<NL, NPW, W, true, true>), grid, block, shm, s, a); break;
    }
}

}  // namespace

int ldsepwi_mask(int nl, int np)
{
    int mask = 0;
    for (int w = 2; w <= EPWI_MAX_W; w += 2)
        if (shape_of(nl, np, w) >= 0) mask |= 1 << w;
    return mask;
}

bool ldsepwi_applicable(const ldpc_code *h, const LdsCode &lc)
{
    return lc.epw_valid && ((size_t)h->n + 2) * 4 <= kLdsMaxBytes && ldsepwi_mask(lc.epw_nl, lc.epw_np) != 0;
}

// The automatic W by plan shape and batch, fitted to
// profiles/i8_ep_wide_rate.json (tools/i8_ep_wide_rate.py; DESIGN.md section 7;
// tests/test_i8_ep_wide_cpu.py restates it).  Not the float rule: in int8 a
// workgroup decodes two codewords, so a batch fills the machine with half the
// workgroups and the four-wave shapes (121 .. 138 VGPRs, 3 or 4 waves per SIMD)
// stay ahead for longer.  The 12-layer shape (1944x972) runs four waves at every
// batch: about 1.15 .. 1.6x faster than two at all four measured batches.  The
// 11-layer shape of up to 14 passes (1248x624) runs four waves up to 8192
// codewords (about 1.1 .. 1.6x faster at 1024 and 4096) and two beyond (faster
// by a few per cent at 16384 and 65536; the threshold is the geometric mean of
// 4096 and 16384).  More than 14 passes (2304x1152) are compiled for four waves
// only.  At every measured point the faster W was ahead of the LDS-resident
// family 7 by far more than the spread of the steps (about 0.2 .. 0.7 of its
// time, spread below 0.1; the table is in DESIGN.md section 5), so the rule
// never hands a qualifying table back: *beats_old is always true.
int ldsepwi_rule(int nl, int np, int mask, int batch, bool *beats_old)
{
    (void)np;
    if (beats_old) *beats_old = mask != 0;
    if (!mask) return 0;
    if (!(mask & (1 << 2))) return 4;
    if (!(mask & (1 << 4))) return 2;
    return nl == 12 || batch <= 8192 ? 4 : 2;
}

int ldsepwi_waves(const LdsCode &lc, int batch)
{
    const int mask = ldsepwi_mask(lc.epw_nl, lc.epw_np);
    const char *e = getenv("LDPC_EPW_WAVES");   // shared with ldsepw
    if (e && *e) {
        const int w = atoi(e);
        return (w == 2 || w == 4) && (mask & (1 << w)) ? w : 0;
    }
    return ldsepwi_rule(lc.epw_nl, lc.epw_np, mask, batch, nullptr);
}

int launch_ldsepwi(const LdsCode &lc, const ldpc_code *h, const int8_t *llr, uint8_t *hard, int8_t *soft, int waves,
                   const DecodeLaunch &L, hipStream_t s)
{
    if (!ldsepwi_applicable(h, lc) || L.batch <= 0) return -1;
    const int shape = shape_of(lc.epw_nl, lc.epw_np, waves);
    if (shape < 0) return -1;
    const bool nms = L.algo == 1;
    EpwiArgs a{};
    a.llr = llr;
    a.hard = hard;
    a.soft = soft;
    a.tab = lc.d_epw_tab;
    a.n = h->n;
    a.np = lc.epw_np;
    a.batch = L.batch;
    a.iters = L.iters;
    a.vmin2 = splat(L.var_min);
    a.mmax2 = splat(L.msg_max);
    a.par2 = splat(nms ? (L.param & 0xFFFF) : (L.param & 0xFF));
    a.later = nms ? 0u : lc.epw_later;
    a.degs = lc.epw_degs;
    a.iters_used = L.iters_used;
    const size_t shm = ((size_t)h->n + 2) * 4;
    const dim3 grid((L.batch + 1) / 2), block(64 * waves);
#define EPWI_CASE(i, NL, NPW, W) \
    case i: launch_shape<NL, NPW, W>(a, nms, L.early != 0, grid, block, shm, s); break;
    switch (shape) {
        EPWI_SHAPES(EPWI_CASE)
    default: return -1;
    }
#undef EPWI_CASE
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
