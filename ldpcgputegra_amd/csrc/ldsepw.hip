// ldsepw.hip -- ldsep.hip's edge-parallel float layered min-sum with one
// codeword spread over the W = 2 or 4 waves of a workgroup, for the
// quasi-cyclic codes whose (layer, pass) slots pass what one wave's registers
// hold (about 77): 1944x972 (12 layers x 11 passes of 8 checks), 1248x624
// (11 x 13), 2304x1152 (11 x 24) and tables of their shape.  Family 9, float32,
// behind ldpc_ctx_set_ep_wide.
//
// What is ldsep.hip's, unchanged: 8 lanes per check and 8 checks per pass; each
// lane keeps the messages of its edges in VGPRs for the whole decode and the
// LDS byte offset of its edge's variable per slot; the exclusive-minimum and
// the sign-parity butterflies of ldsep_common.h on the magnitudes as integers;
// the sink variables V[N] = -inf (padding lanes of a check) and V[N + 1] (the
// lanes of an empty check slot); x + 0.0f on load.  Every per-edge operation
// is that kernel's, so the float contract is too: bit for bit the oracle's
// decode of the LLRs with every zero made +0.0, and equal to its decode of the
// LLRs as given except in the sign of a zero; subnormals kept
// (tests/test_gpu_ep_wide.py).
//
// What changes:
// * one workgroup = one codeword (grid = batch, block = 64 W); V, N + 2 floats,
//   lives in the workgroup's LDS;
// * the passes of a layer are dealt to the waves interleaved: wave w takes
//   passes w, w + W, w + 2 W, ... (NPW = ceil(passes / W) slots per layer and
//   wave; a pass index past the layer plan's is an empty slot on V[N + 1]), so
//   a ragged last pass costs one wave one slot and the others nothing;
// * the checks of a layer share no variable, so the waves need no ordering
//   inside a layer; one workgroup barrier after a layer's V writes orders them
//   before the next layer's reads, and the last layer's before the syndrome
//   pass and the epilogue;
// * early termination is decided per workgroup: each wave ORs the parities of
//   its slots into an LDS word, a barrier, every wave reads the same word.
#include <algorithm>
#include <cstdlib>
#include <vector>

#include "kernels.h"
#include "lds.h"
#include "ldsep_common.h"   // EP_G, EP_CPP, kEpShapes (what the one-wave kernel takes), the DPP helpers

namespace {

using namespace ldsep;

// (layers, passes per wave, waves) compiled; a table runs on W waves where some
// entry of its layer count has W * NPW >= its passes (the least NPW of them)
struct EpwShape {
    int nl, npw, w;
};
constexpr EpwShape kEpwShapes[] = {
    {12, 6, 2}, {12, 3, 4},               // 1944x972 (Z = 81: 11 passes)
    {11, 7, 2}, {11, 4, 4},               // 1248x624 (Z = 104: 13 passes)
    {11, 6, 4},                           // 2304x1152 (Z = 192: 24 passes)
};
constexpr int kEpwShapeCount = (int)(sizeof(kEpwShapes) / sizeof(kEpwShapes[0]));
// the instantiations launch_ldsepw switches over: kEpwShapes again, entry by entry
#define EPW_SHAPES(X) X(0, 12, 6, 2) X(1, 12, 3, 4) X(2, 11, 7, 2) X(3, 11, 4, 4) X(4, 11, 6, 4)
#define EPW_SAME(i, NL, NPW, W) \
    static_assert(kEpwShapes[i].nl == NL && kEpwShapes[i].npw == NPW && kEpwShapes[i].w == W, "kEpwShapes vs EPW_SHAPES");
EPW_SHAPES(EPW_SAME)
static_assert(kEpwShapeCount == 5, "kEpwShapes vs EPW_SHAPES");
#undef EPW_SAME
constexpr int EPW_MAX_W = 4;

struct EpwArgs {
    const float *llr;       // frame-major [batch][N]
    uint8_t *hard;          // frame-major [batch][N], may be null
    float *soft;            // frame-major [batch][N], may be null
    const uint32_t *tab;    // [nl * np][64]: LDS byte offset of lane's variable in V (sinks N, N+1)
    int n, np, iters, early;
    float beta;
    int32_t *iters_used;
    unsigned long long *cnt;   // fused error count (DecodeLaunch::cnt), may be null
    const uint8_t *cnt_ref;
    int cnt_k;
};

// amdgpu_waves_per_eu(2): a budget of 256 registers.  A workgroup of 2 or 4
// waves would be allowed 512, and the scheduler then spends them: no shape
// needs more than 247 (DESIGN.md section 5 has the table; AGPRs and scratch 0).
template <int NL, int NPW, int W, bool NMS>
__global__ void __launch_bounds__(64 * W) __attribute__((amdgpu_waves_per_eu(2))) ldsepw_decode(EpwArgs a)
{
    constexpr int NS = NL * NPW;
    constexpr uint32_t SIGN = 0x80000000u;
    extern __shared__ __attribute__((aligned(16))) float epw_V[];
    __shared__ uint32_t epw_bad[2];                    // early termination: the workgroup's verdict, by iteration parity
    __shared__ unsigned long long epw_cnt[W][2];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x;                          // grid = batch: every workgroup has a codeword
    float *V = epw_V;
    char *L = (char *)epw_V;
    // LDS byte address of this lane's variable per (layer, this wave's q-th
    // pass).  Past 72 slots a wave (11 x 7) the offsets of two slots share a
    // register as 16-bit halves ((N + 2) * 4 <= 64 KB, ldsepw_plan): with a
    // register each, that shape passed 256 VGPRs and the compiler parked
    // values in AGPRs (NMS) or, held to two waves per SIMD, in scratch; the
    // extraction is one VALU per access.
    constexpr bool PACK = NS > 72;
    uint32_t off[PACK ? (NS + 1) / 2 : NS];
    float msg[NS];
#pragma unroll
    for (int l = 0; l < NL; l++)
#pragma unroll
        for (int q = 0; q < NPW; q++) {
            const int p = q * W + wave;                // wave-uniform
            const int s = l * NPW + q;
            const uint32_t o = p < a.np ? a.tab[(l * a.np + p) * 64 + lane] : (uint32_t)(a.n + 1) * 4u;
            if (!PACK) off[s] = o;
            else if (s & 1) off[s >> 1] |= o << 16;
            else off[s >> 1] = o;
            msg[s] = 0.0f;   // CDecoder_OMS_fixed_SSE.cpp:129-131
        }
    auto addr = [&](int s) -> uint32_t {
        return !PACK ? off[s] : (s & 1) ? off[s >> 1] >> 16 : off[s >> 1] & 0xFFFFu;
    };
    // LLRs in, -0.0 made +0.0 (x + 0.0f), as ldsep.hip: the sign bit of a
    // contribution is then exactly the reference's c < 0
    const float *src = a.llr + (size_t)b * a.n;
    for (int i = threadIdx.x; i < a.n; i += 64 * W) V[i] = src[i] + 0.0f;
    if (threadIdx.x < 2) {
        V[a.n + threadIdx.x] = -__builtin_huge_valf();
        epw_bad[threadIdx.x] = 0;
    }
    __syncthreads();
    int it = 0;
    // BARRIER INVARIANT: every wave of the workgroup executes the same number
    // of barriers.  The trip count and the break below depend only on kernel
    // arguments and on an LDS word all waves read after a barrier, so they are
    // workgroup-uniform; a wave whose passes are all empty slots still runs
    // every layer and arrives at every barrier; no wave returns before the
    // loop ends.  A wave that left early would leave the others waiting at
    // s_barrier for ever.
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
        repack();
#pragma unroll
        for (int l = 0; l < NL; l++) {
            float c[NPW];
#pragma unroll
            for (int q = 0; q < NPW; q++) c[q] = *(const float *)(L + addr(l * NPW + q));
#pragma unroll
            for (int q = 0; q < NPW; q++) {
                const int s = l * NPW + q;
                const float cj = c[q] - msg[s];
                const uint32_t aj = __float_as_uint(cj) & ~SIGN;   // |c| (as an ordered integer)
                const uint32_t sj = __float_as_uint(cj) & SIGN;    // c < 0
                // the minimum over the OTHER 7 lanes of the check: ldsep.hip's exclusive-min butterfly
                uint32_t e = dpp_xor1(aj);
                uint32_t mm = min(aj, e);
                e = min(e, dpp_xor2(mm));
                mm = min(mm, dpp_xor2(mm));
                e = min(e, dpp_hmirror(mm));
                uint32_t sg = sj ^ dpp_xor1(sj);
                sg ^= dpp_xor2(sg);
                sg ^= dpp_hmirror(sg);
                const float sel = __uint_as_float(e);
                const float r = NMS ? sel * a.beta : fmaxf(sel - a.beta, 0.0f);
                const float m = __uint_as_float(__float_as_uint(r) ^ (sg ^ sj));
                msg[s] = m;
                c[q] = cj + m;
            }
#pragma unroll
            for (int q = 0; q < NPW; q++) *(float *)(L + addr(l * NPW + q)) = c[q];
            // this layer's V writes, of every wave, before the next layer's
            // reads (after the last layer: before the syndrome and the epilogue)
            __syncthreads();
        }
        it++;
        if (a.early) {   // syndrome of hard(V) over every check (sinks read -inf or NaN: never 1)
            uint32_t bad = 0;
            repack();
#pragma unroll
            for (int l = 0; l < NL; l++) {
#pragma unroll
                for (int q = 0; q < NPW; q++) {
                    uint32_t h = *(const float *)(L + addr(l * NPW + q)) > 0.0f ? 1u : 0u;
                    h ^= dpp_xor1(h);
                    h ^= dpp_xor2(h);
                    h ^= dpp_hmirror(h);
                    bad |= h;
                }
            }
            const int par = it & 1;
            if (__builtin_amdgcn_ballot_w64(bad != 0) != 0 && lane == 0) atomicOr(&epw_bad[par], 1u);
            // the other word is next iteration's: nobody reads it before the
            // barrier below, and its writers come after that barrier
            if (threadIdx.x == 0) epw_bad[par ^ 1] = 0;
            __syncthreads();
            if (epw_bad[par] == 0) break;   // the same word for every wave: all leave together
        }
    }
    if (a.iters_used && threadIdx.x == 0) a.iters_used[b] = it;
    uint8_t *hd = a.hard ? a.hard + (size_t)b * a.n : nullptr;
    float *sd = a.soft ? a.soft + (size_t)b * a.n : nullptr;
    const uint8_t *rf = a.cnt_ref ? a.cnt_ref + (size_t)b * a.n : nullptr;
    int errs = 0;
    for (int i = threadIdx.x; i < a.n; i += 64 * W) {
        const float v = V[i];
        const uint8_t hb = v > 0.0f;   // code/x86/CTools/CTools.cpp:370
        if (hd) hd[i] = hb;
        if (sd) sd[i] = v;
        if (a.cnt && i < a.cnt_k) errs += (hb ^ (rf ? rf[i] : 0)) & 1;   // CErrorAnalyzer.cpp:123-154
    }
    if (a.cnt) {   // (kernel argument: uniform) the waves' partial bit errors, then one atomic pair per codeword
        for (int o = 32; o > 0; o >>= 1) errs += __shfl_xor(errs, o);
        if (lane == 0) epw_cnt[wave][0] = (unsigned long long)errs;
        __syncthreads();
        if (threadIdx.x == 0) {
            unsigned long long s = 0;
            for (int w = 0; w < W; w++) s += epw_cnt[w][0];
            if (s) {
                atomicAdd(&a.cnt[0], s);
                atomicAdd(&a.cnt[1], 1ull);
            }
        }
    }
}

// does ldsep.hip's one-wave kernel take this plan?  (ldsep_upload's and
// ldsep_applicable's conditions, on the host: where it fits, it stays)
bool one_wave_fits(const ldpc_code *h, int nl, int np, int maxd)
{
    if (h->n + 2 > 16384 || maxd > EP_G) return false;
    if ((size_t)EP_WAVES * ((h->n + 2 + 3) / 4 * 4) * 4 > kLdsMaxBytes) return false;
    for (const EpShape &s : kEpShapes)
        if (nl == s.nl && np <= s.np) return true;
    return false;
}

// index into kEpwShapes of the entry that runs (nl, np) on w waves, -1 if none
int shape_of(int nl, int np, int w)
{
    int best = -1;
    for (int i = 0; i < kEpwShapeCount; i++) {
        const EpwShape &s = kEpwShapes[i];
        if (s.nl == nl && s.w == w && s.w * s.npw >= np && (best < 0 || s.npw < kEpwShapes[best].npw)) best = i;
    }
    return best;
}

}  // namespace

EpwPlan ldsepw_plan(const ldpc_code *h, const std::vector<int4> &layers)
{
    EpwPlan pl;
    if (layers.empty() || h->n > 65535 || ((size_t)h->n + 2) * 4 > kLdsMaxBytes) return pl;
    int maxw = 0, maxd = 0;
    for (const int4 &L : layers) {
        maxw = std::max(maxw, L.y);
        maxd = std::max(maxd, L.z);
    }
    const int nl = (int)layers.size(), np = (maxw + EP_CPP - 1) / EP_CPP;
    if (maxd > EP_G || one_wave_fits(h, nl, np, maxd)) return pl;
    for (int w = 2; w <= EPW_MAX_W; w += 2)
        if (shape_of(nl, np, w) >= 0) pl.mask |= 1 << w;
    if (pl.mask) {
        pl.nl = nl;
        pl.np = np;
    }
    return pl;
}

// The automatic W by plan shape and batch, fitted to profiles/ep_wide_rate.json
// (tools/ep_wide_rate.py; tests/test_ep_wide_cpu.py
// restates it).  Two waves wherever they are compiled, but for the 12-layer
// shape (1944x972) past 2048 codewords: there four waves hold 12 x 3 slots in
// 132 VGPRs, three workgroups' waves per SIMD, and were 1.08 .. 1.13x faster
// from 4096 codewords on, while at 1024 two waves were 1.06 .. 1.08x faster (the
// threshold is the geometric mean of the two batches).  For the 11-layer shape
// of 13 passes (1248x624) four waves run 16 slots a layer for 13 passes, two run
// 14, and two were faster at every batch.  More than 14 passes (2304x1152) are
// compiled for four waves only.  At every measured point the faster W beat the
// LDS-resident family 7 (0.21 .. 0.90 of its time), so the rule never hands a
// qualifying table back to it: *beats_old is always true.
int ldsepw_rule(int nl, int np, int mask, int batch, bool *beats_old)
{
    (void)np;
    if (beats_old) *beats_old = mask != 0;
    if (!mask) return 0;
    if (!(mask & (1 << 2))) return 4;
    return nl == 12 && batch > 2048 && (mask & (1 << 4)) ? 4 : 2;
}

int ldsepw_waves(const LdsCode &lc, int batch)
{
    const char *e = getenv("LDPC_EPW_WAVES");
    if (e && *e) {
        const int w = atoi(e);
        return (w == 2 || w == 4) && (lc.epw_mask & (1 << w)) ? w : 0;
    }
    return ldsepw_rule(lc.epw_nl, lc.epw_np, lc.epw_mask, batch, nullptr);
}

int ldsepw_upload(const ldpc_code *h, const std::vector<int4> &layers, LdsCode *lc)
{
    lc->epw_valid = 0;
    const EpwPlan pl = ldsepw_plan(h, layers);
    if (!pl.mask) return LDPC_OK;
    // [slot][lane] LDS byte offsets, as ldsep_upload's: slot (l, p), lane (g, j) = edge j of check 8p + g of layer l
    std::vector<uint32_t> tab((size_t)pl.nl * pl.np * 64, (uint32_t)(h->n + 1) * 4u);
    for (int l = 0; l < pl.nl; l++) {
        const int4 L = layers[l];
        for (int p = 0; p < pl.np; p++)
            for (int lane = 0; lane < 64; lane++) {
                const int ck = p * EP_CPP + lane / EP_G, j = lane % EP_G;
                uint32_t v = (uint32_t)(h->n + 1);
                if (ck < L.y) v = j < L.z ? h->edge_var[L.x + ck * L.z + j] : (uint32_t)h->n;
                tab[((size_t)l * pl.np + p) * 64 + lane] = v * 4u;
            }
    }
    if (hipMalloc(&lc->d_epw_tab, tab.size() * 4) != hipSuccess) return ldpc_set_error(LDPC_ENOMEM, "ldsepw table");
    if (hipMemcpy(lc->d_epw_tab, tab.data(), tab.size() * 4, hipMemcpyHostToDevice) != hipSuccess)
        return ldpc_set_error(LDPC_EDEVICE, "ldsepw table upload");
    lc->epw_nl = pl.nl;
    lc->epw_np = pl.np;
    lc->epw_mask = pl.mask;
    lc->epw_degs = 0;
    lc->epw_later = 0;
    for (int l = 0; l < pl.nl; l++) {   // for ldsepwi.hip, as ldsep_upload's (nl <= 12, degree <= EP_G: 4 bits per layer)
        lc->epw_degs |= (unsigned long long)layers[l].z << (4 * l);
        lc->epw_later |= (layers[l].w ? 1u : 0u) << l;
    }
    lc->epw_valid = 1;
    return LDPC_OK;
}

bool ldsepw_applicable(const ldpc_code *h, const LdsCode &lc, bool is_float)
{
    return is_float && lc.epw_valid && ((size_t)h->n + 2) * 4 <= kLdsMaxBytes;
}

int launch_ldsepw(const LdsCode &lc, const ldpc_code *h, const float *llr, uint8_t *hard, float *soft, int batch,
                  int iters, int waves, const DecodeLaunch &L, hipStream_t s)
{
    if (!ldsepw_applicable(h, lc, true) || !(lc.epw_mask & (1 << waves))) return -1;
    const int shape = shape_of(lc.epw_nl, lc.epw_np, waves);
    if (shape < 0) return -1;
    EpwArgs a{};
    a.llr = llr;
    a.hard = hard;
    a.soft = soft;
    a.tab = lc.d_epw_tab;
    a.n = h->n;
    a.np = lc.epw_np;
    a.iters = iters;
    a.early = L.early;
    a.beta = L.beta;
    a.iters_used = L.iters_used;
    a.cnt = L.cnt;
    a.cnt_ref = L.cnt_ref;
    a.cnt_k = L.cnt_k;
    const bool nms = L.algo == 1;
    const size_t shm = ((size_t)h->n + 2) * 4;
    const dim3 grid(batch), block(64 * waves);
#define EPW_CASE(i, NL, NPW, W)                                                                        \
    case 2 * (i): hipLaunchKernelGGL((ldsepw_decode<NL, NPW, W, false>), grid, block, shm, s, a); break; \
    case 2 * (i) + 1: hipLaunchKernelGGL((ldsepw_decode<NL, NPW, W, true>), grid, block, shm, s, a); break;
    switch (shape * 2 + (nms ? 1 : 0)) {
        EPW_SHAPES(EPW_CASE)
    default: return -1;
    }
#undef EPW_CASE
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
