// stairh.hip -- the launch of stairh_decode (stairh_kernel.h, one object per
// degree from stairh_deg.hip), its group-width rule and the binary16 syndrome
// pass of its early termination.  The launch sequence is stairf_et.h's.
#include <cstdlib>
#include <cstring>

#include "stairf_et.h"
#include "stairh.h"
#include "stairh_kernel.h"

namespace {

using namespace stairf_dev;

// stairf_syndrome_k on binary16 V: one lane per codeword, a chunk of checks per workgroup
__global__ void __launch_bounds__(64) stairh_syndrome_k(const _Float16 *V, const uint32_t *ev, const uint8_t *live,
                                                        uint32_t *bad, int m, int d0, int chunk, int stride)
{
    const int b = blockIdx.x * 64 + threadIdx.x;
    const bool on = live[b] != 0;
    if (!__any(on)) return;
    const int c0 = blockIdx.y * chunk, c1 = min(m, c0 + chunk);
    const _Float16 *Vb = V + b;
    int fail = 0;
    for (int c = c0; c < c1; c++) {
        const uint32_t *e = ev + (size_t)c * d0;   // layered order: every check d0 edges apart, the tail last
        const int d = c == m - 1 ? d0 - 1 : d0;
        int par = 0;
        for (int j = 0; j < d; j++) par ^= Vb[(size_t)e[j] * stride] > (_Float16)0.0f;
        fail |= par;
    }
    if (on && fail) bad[b] = 1;
}

uint32_t half_bits(float x)
{
    const _Float16 h = (_Float16)x;   // round to nearest even
    uint16_t u;
    memcpy(&u, &h, 2);
    return u;
}

}  // namespace

bool stairh_stride_ok(const StairfCode &sc, int n, int stride)
{
    return sc.valid && stride % 64 == 0 && ((size_t)n + 1) * stride * 2 < (1ull << 32);
}

size_t stairh_v_bytes(int n, int stride) { return ((size_t)n + 1) * stride * 2; }

size_t stairh_msg_bytes(const StairfCode &sc, int stride) { return (size_t)stride * sc.m * (sc.X + 2) * 2; }

// Group width by batch, among the widths the code has (bit S of `widths` set).
// A wave holds 128 / S codewords, so a batch fills half the waves it fills in
// float, and a wave alone on its SIMD needs a fixed time per iteration whatever
// the batch (the chain and the check arithmetic of its M / S groups): 162 / 90 /
// 52 / 39 ms per 20 iterations at S = 2 / 4 / 8 / 16.  A width pays off once the
// next wider one has more waves than the chip can run at that floor.  Measured
// (DVB-S2 r1/2, 20 it, plain min-sum, tools/f16_rate.py, two runs in one session
// on one machine: its four batches, then --batches 2048 8192 24576), S = 2 / 4 /
// 8 / 16, ms.  profiles/f16_rate.json is a later run of the four batches on
// another machine, where the figures that HBM bounds came out up to 20 % lower
// (16384: 176 / 135 / 202 / 372, float32 199 against 239 here) and the order of
// the widths the same:
//   batch  1024: 162.2 /  90.5 /  52.4 /  39.5
//   batch  2048: 162.9 /  91.2 /  53.1 /  41.6
//   batch  4096: 165.0 /  93.6 /  56.3 /  69.6
//   batch  8192: 169.2 /  96.7 /  98.7 / 166.4
//   batch 16384: 181.5 / 167.0 / 238.0 / 414.2
//   batch 24576: 199.9 / 221.9 / 319.4 / 570.1
//   batch 32768: 246.7 / 312.8 / 513.4 / 854.0 (S = 2: 4.8 TB/s of algorithmic HBM traffic)
static int rule_width(int stride, unsigned widths)
{
    const int want = stride >= 24576 ? 2 : stride >= 8192 ? 4 : stride >= 4096 ? 8 : 16;
    // (2 last: a code whose min_hazard leaves only the narrowest table is valid, so some width must be found)
    for (int S : {want, 8, 4, 16, 2})
        if (widths & (unsigned)S) return S;
    return 0;
}

extern "C" int ldpc_f16_staircase_width_rule(int stride, unsigned widths) { return rule_width(stride, widths & 30u); }

// group width of a launch: LDPC_STAIRF_S (2 / 4 / 8 / 16) if set and the code has that table, else the rule's
int stairh_width(const StairfCode &sc, int stride)
{
    unsigned have = 0;
    for (int S : {2, 4, 8, 16})
        if (sc.d_tab[s_index(S)]) have |= (unsigned)S;
    const char *e = getenv("LDPC_STAIRF_S");
    const int forced = (e && *e) ? atoi(e) : 0;
    if ((forced == 2 || forced == 4 || forced == 8 || forced == 16) && (have & (unsigned)forced)) return forced;
    return rule_width(stride, have);
}

int launch_stairh(const DecodeLaunch &L, const StairfCode &sc, hipStream_t s)
{
    if (!stairh_stride_ok(sc, L.n, L.stride) || L.vpitch != L.stride) return -1;
    if (L.early && (!L.live || !L.bad || !L.iters_used || !L.d_edge_var)) return -1;
    const int S = stairh_width(sc, L.stride);
    if (!S) return -1;
    stairh::StairhArgs a;
    a.V = (uint32_t *)L.V;
    a.msg = (uint32_t *)L.msg;
    a.tab = sc.d_tab[s_index(S)];
    a.G = sc.m / S;
    a.T = sc.m - 1;
    a.stride = L.stride;
    a.iters = L.iters;
    a.x0 = sc.x0;
    const uint32_t b16 = half_bits(L.beta) & 0x7FFFu;   // (-0.0 is +0)
    a.beta2 = b16 | (b16 << 16);
    a.live = nullptr;
    const int algo = L.algo == 1 ? 1 : (b16 & 0x7FFFu) == 0 ? 2 : 0;
    const int blocks = L.stride / (128 / S);
    auto run = [&](const stairh::StairhArgs &aa) {
        switch (sc.X) {
        case 5: return stairh_launch_x5(aa, S, blocks, algo, s);
        case 8: return stairh_launch_x8(aa, S, blocks, algo, s);
        case 12: return stairh_launch_x12(aa, S, blocks, algo, s);
        case 20: return stairh_launch_x20(aa, S, blocks, algo, s);
        case 25: return stairh_launch_x25(aa, S, blocks, algo, s);
        case 28: return stairh_launch_x28(aa, S, blocks, algo, s);
        }
        return -1;
    };
    // stairf_et.h's run_decode with the binary16 syndrome: all the iterations in
    // one launch, or with early termination one launch per iteration
    if (!L.early) {
        if (L.iters_used) {
            hipLaunchKernelGGL(stairf_fill_iters_k, dim3((L.batch + 63) / 64), dim3(64), 0, s, L.iters_used, L.batch,
                               L.iters);
            if (hipGetLastError() != hipSuccess) return -1;
        }
        return L.iters <= 0 ? 0 : run(a);
    }
    const int cb = L.stride / 64;
    hipLaunchKernelGGL(stairf_et_init_k, dim3(cb), dim3(64), 0, s, L.live, L.bad, L.iters_used, L.batch, L.stride,
                       L.iters);
    if (hipGetLastError() != hipSuccess) return -1;
    const int chunks = std::max(1, std::min(sc.m, 4096 / cb)), chunk = (sc.m + chunks - 1) / chunks;
    a.iters = 1;
    a.live = L.live;
    for (int it = 1; it <= L.iters; it++) {
        if (run(a)) return -1;
        hipLaunchKernelGGL(stairh_syndrome_k, dim3(cb, (sc.m + chunk - 1) / chunk), dim3(64), 0, s,
                           (const _Float16 *)L.V, L.d_edge_var, L.live, L.bad, sc.m, sc.X + 2, chunk, L.stride);
        hipLaunchKernelGGL(stairf_et_step_k, dim3(cb), dim3(64), 0, s, L.live, L.bad, L.iters_used, L.batch, it);
        if (hipGetLastError() != hipSuccess) return -1;
    }
    return 0;
}
