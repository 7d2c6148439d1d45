// stairf_et.h -- the launch sequence around the decode launch of the two
// staircase float kernels (stairf.hip min-sum, stairbp.hip belief propagation)
// and the helper kernels of its early termination.  Each of the two
// translation units that launch a decode includes it; internal to them.
#pragma once
#include <algorithm>

#include "stairf_dev.h"

namespace stairf_dev {

// early termination (oracle_decode_f32: stop a codeword after the first
// iteration whose hard decisions V > 0 satisfy every check): after each
// one-iteration launch, every check of every live codeword is tested (one
// lane per codeword, a chunk of checks per workgroup, the check's nodes
// wave-uniform), any failing check marks the codeword bad; then live
// codewords without a bad mark stop with that iteration count
static __global__ void __launch_bounds__(64) stairf_et_init_k(uint8_t *live, uint32_t *bad, int32_t *iters_used,
                                                              int batch, int stride, int iters)
{
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= stride) return;
    live[b] = b < batch;
    bad[b] = 0;
    if (b < batch) iters_used[b] = iters;
}

// without early termination every codeword runs all the iterations
static __global__ void __launch_bounds__(64) stairf_fill_iters_k(int32_t *iters_used, int batch, int iters)
{
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b < batch) iters_used[b] = iters;
}

static __global__ void __launch_bounds__(64) stairf_syndrome_k(const float *V, const uint32_t *ev,
                                                               const uint8_t *live, uint32_t *bad, int m, int d0,
                                                               int chunk, int stride)
{
    const int b = blockIdx.x * 64 + threadIdx.x;
    const bool on = live[b] != 0;
    if (!__any(on)) return;
    const int c0 = blockIdx.y * chunk, c1 = min(m, c0 + chunk);
    const float *Vb = V + b;
    int fail = 0;
    for (int c = c0; c < c1; c++) {
        const uint32_t *e = ev + (size_t)c * d0;   // layered order: every check d0 edges apart, the tail last
        const int d = c == m - 1 ? d0 - 1 : d0;
        int par = 0;
        for (int j = 0; j < d; j++) par ^= Vb[(size_t)e[j] * stride] > 0.0f;
        fail |= par;
    }
    if (on && fail) bad[b] = 1;
}

static __global__ void __launch_bounds__(64) stairf_et_step_k(uint8_t *live, uint32_t *bad, int32_t *iters_used,
                                                              int batch, int it)
{
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= batch) return;
    if (live[b] && !bad[b]) {
        live[b] = 0;
        iters_used[b] = it;
    }
    bad[b] = 0;
}

// the launch arguments of a decode at group width S (live unset)
inline StairfArgs make_args(const DecodeLaunch &L, const StairfCode &sc, int S)
{
    StairfArgs a;
    a.V = (float *)L.V;
    a.msg = (float *)L.msg;
    a.tab = sc.d_tab[s_index(S)];
    a.G = sc.m / S;
    a.T = sc.m - 1;
    a.stride = L.stride;
    a.iters = L.iters;
    a.x0 = sc.x0;
    a.beta = L.beta;
    a.live = nullptr;
    return a;
}

// the launches of one decode around run(a), the decode launch of either
// kernel: all the iterations in one launch, or with early termination one
// launch per iteration, then the syndrome
template <class Run>
int run_decode(const DecodeLaunch &L, const StairfCode &sc, StairfArgs a, hipStream_t s, Run run)
{
    if (!L.early) {
        if (L.iters_used) {   // as the other kernels report it (generic.hip, coop3.hip fill_iters3_k)
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
        hipLaunchKernelGGL(stairf_syndrome_k, dim3(cb, (sc.m + chunk - 1) / chunk), dim3(64), 0, s, (const float *)L.V,
                           L.d_edge_var, L.live, L.bad, sc.m, sc.X + 2, chunk, L.stride);
        hipLaunchKernelGGL(stairf_et_step_k, dim3(cb), dim3(64), 0, s, L.live, L.bad, L.iters_used, L.batch, it);
        if (hipGetLastError() != hipSuccess) return -1;
    }
    return 0;
}

}  // namespace stairf_dev
