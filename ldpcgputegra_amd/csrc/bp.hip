// bp.hip -- layered belief propagation (sum-product, LDPC_ALGO_BP), float only.
//
// The arithmetic is bp_math.h's: g(x) ~ ln(1 + e^-x) written out in IEEE
// + - *, the box-plus built on it and the forward / backward recursion of one
// check.  The host decoder (host.cpp) runs the same header, so
// both kernels here equal it bit for bit.  A check of degree D costs 3 (D - 2)
// box-plus, about 60 VALU operations each: these kernels are VALU-bound where
// their min-sum twins are bound by LDS / memory latency.
//
// Two kernels, each the shape of a min-sum one:
//   bp_lds_decode      lds.hip's non-split kernel (family LDPC_KERNEL_LDS): the
//                      codeword's V and messages in LDS, one lane per check of a
//                      layer, 64 >> lpc_log2 codewords per wave, LdsCode's edge
//                      table and layers.  Never two lanes per check: splitting
//                      the recursion would change the order of the operations.
//   bp_generic_decode  generic.hip's (family LDPC_KERNEL_GENERIC): one lane per
//                      codeword, V[node][stride] and msg[edge][stride] in device
//                      scratch, H indices wave-uniform.  Any code.
// The degree is a template parameter (2 .. 32), so t, F and the indices of a
// check stay in registers.
#include "bp_math.h"
#include "ctx.h"

namespace {

#define LDPC_BP_DEG_CASES(X) \
    X(2) X(3) X(4) X(5) X(6) X(7) X(8) X(9) X(10) X(11) X(12) X(13) X(14) X(15) X(16) X(17) X(18) X(19) \
    X(20) X(21) X(22) X(23) X(24) X(25) X(26) X(27) X(28) X(29) X(30) X(31) X(32)

// ---- LDS-resident ------------------------------------------------------------

struct BpLdsArgs {
    const float *llr;         // frame-major [batch][N]
    uint8_t *hard;            // frame-major [batch][N] 0/1, may be null
    float *soft;              // frame-major [batch][N], may be null
    const uint16_t *tab;      // [E] layer-major edge -> variable
    const int4 *layers;       // [nl] (edge base, checks, degree, later-group flag)
    int nl, n, e, batch, iters;
    int lpc_log2;             // lanes per codeword = 1 << lpc_log2
    int early;
    int32_t *iters_used;
    int tab_bytes;            // LDS bytes of the table, 16-B aligned
};

// check i of a layer of cnt checks: edge j at tab / msg [j * cnt]
template <int D>
LDPC_DEV void bp_lds_check(float *V, float *msg, const uint16_t *tab, int cnt)
{
    float t[D], fm[D];
    int idx[D];
#pragma unroll
    for (int j = 0; j < D; j++) {
        idx[j] = tab[j * cnt];
        t[j] = fm[j] = V[idx[j]] - msg[j * cnt];
    }
    bp_check(D, t, fm);
#pragma unroll
    for (int j = 0; j < D; j++) {
        msg[j * cnt] = fm[j];
        V[idx[j]] = t[j] + fm[j];
    }
}

// the checks li, li + lpc, ... of one layer (lane li of its codeword)
template <int D>
LDPC_DEV void bp_lds_layer(float *V, float *msg, const uint16_t *tab, int base, int cnt, int li, int lpc)
{
    for (int i = li; i < cnt; i += lpc) bp_lds_check<D>(V, msg + base + i, tab + base + i, cnt);
}

__global__ void __launch_bounds__(64) bp_lds_decode(BpLdsArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = threadIdx.x;
    const int lpc = 1 << a.lpc_log2, cpw = 64 >> a.lpc_log2;
    const int cl = lane >> a.lpc_log2, li = lane & (lpc - 1);
    const int b = blockIdx.x * cpw + cl;
    const bool active = b < a.batch;
    const int N = a.n, E = a.e;
    uint16_t *tab = (uint16_t *)smem;
    float *Vall = (float *)(smem + a.tab_bytes);
    float *V = Vall + (size_t)cl * N;
    float *msg = Vall + (size_t)cpw * N + (size_t)cl * E;

    // stage the table (whole wave, 16-B chunks: the device table is padded to
    // tab_bytes), the LLRs (one codeword per lane group) and zero the messages
    {
        const uint4 *g = (const uint4 *)a.tab;
        uint4 *l = (uint4 *)smem;
#pragma unroll 8
        for (int i = lane; i < a.tab_bytes / 16; i += 64) l[i] = g[i];
    }
    if (active) {
        const float *src = a.llr + (size_t)b * N;
#pragma unroll 8
        for (int i = li; i < N; i += lpc) V[i] = src[i];
    } else {
        for (int i = li; i < N; i += lpc) V[i] = 0.0f;
    }
#pragma unroll 8
    for (int i = li; i < E; i += lpc) msg[i] = 0.0f;
    __syncthreads();

    const unsigned long long gmask = (lpc == 64 ? ~0ull : ((1ull << lpc) - 1)) << (cl * lpc);
    bool live = active;
    int it = 0;
    for (; it < a.iters; it++) {
        if (!__builtin_amdgcn_ballot_w64(live)) break;
        for (int l = 0; l < a.nl; l++) {
            const int4 L = a.layers[l];   // wave-uniform
            if (live) {
                switch (L.z) {
#define X(DD) \
    case DD: bp_lds_layer<DD>(V, msg, tab, L.x, L.y, li, lpc); break;
                    LDPC_BP_DEG_CASES(X)
#undef X
                default: break;
                }
            }
            __syncthreads();   // one wave: orders the layer's LDS writes before the next layer's reads
        }
        if (a.early && live) {
            // syndrome of hard(V) over this lane's checks of every layer
            int bad = 0;
            for (int l = 0; l < a.nl; l++) {
                const int4 L = a.layers[l];
                for (int i = li; i < L.y; i += lpc) {
                    int par = 0;
                    for (int j = 0; j < L.z; j++) par ^= (V[tab[L.x + j * L.y + i]] > 0.0f);
                    bad |= par;
                }
            }
            const unsigned long long anybad = __builtin_amdgcn_ballot_w64(bad != 0) & gmask;
            if (!anybad) {
                live = false;
                if (a.iters_used && li == 0) a.iters_used[b] = it + 1;
            }
        }
    }
    if (active && live && a.iters_used && li == 0) a.iters_used[b] = it;
    __syncthreads();
    if (!active) return;
    uint8_t *hd = a.hard ? a.hard + (size_t)b * N : nullptr;
    float *sd = a.soft ? a.soft + (size_t)b * N : nullptr;
    for (int i = li; i < N; i += lpc) {
        const float v = V[i];
        if (hd) hd[i] = v > 0.0f;
        if (sd) sd[i] = v;
    }
}

// ---- any H -------------------------------------------------------------------

struct BpGenArgs {
    float *V;                 // V[node][stride]
    float *msg;               // msg[edge][stride]
    const uint32_t *ev;
    const int *gdeg;
    const int *gcnt;
    int n_groups, stride, batch, iters, early;
    int32_t *iters_used;
};

template <int D>
LDPC_DEV void bp_gen_check(float *__restrict__ V, float *__restrict__ mp, const uint32_t *__restrict__ ev,
                           size_t stride, int b)
{
    float t[D], fm[D];
#pragma unroll
    for (int j = 0; j < D; j++) t[j] = fm[j] = V[(size_t)ev[j] * stride + b] - mp[(size_t)j * stride];
    bp_check(D, t, fm);
#pragma unroll
    for (int j = 0; j < D; j++) {
        mp[(size_t)j * stride] = fm[j];
        V[(size_t)ev[j] * stride + b] = t[j] + fm[j];
    }
}

template <int D>
LDPC_DEV void bp_gen_group(float *V, float *msg, const uint32_t *ev, int cnt, size_t stride, int b)
{
    for (int i = 0; i < cnt; i++) bp_gen_check<D>(V, msg + (size_t)i * D * stride, ev + i * D, stride, b);
}

LDPC_DEV bool bp_syndrome_ok(const float *__restrict__ V, const uint32_t *__restrict__ ev, const int *gdeg,
                             const int *gcnt, int n_groups, size_t stride, int b)
{
    for (int g = 0; g < n_groups; g++) {
        const int d = gdeg[g];
        for (int i = 0; i < gcnt[g]; i++, ev += d) {
            int par = 0;
            for (int j = 0; j < d; j++) par ^= (V[(size_t)ev[j] * stride + b] > 0.0f);
            if (par) return false;
        }
    }
    return true;
}

__global__ void __launch_bounds__(64) bp_generic_decode(BpGenArgs a)
{
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= a.batch) return;
    float *V = a.V;
    float *msg = a.msg + b;    // this codeword's column of msg[edge][stride]
    const size_t stride = a.stride;
    int it = 0;
    while (it < a.iters) {
        const uint32_t *ev = a.ev;
        float *mp = msg;
        for (int g = 0; g < a.n_groups; g++) {
            const int d = a.gdeg[g], cnt = a.gcnt[g];
            switch (d) {
#define X(DD) \
    case DD: bp_gen_group<DD>(V, mp, ev, cnt, stride, b); break;
                LDPC_BP_DEG_CASES(X)
#undef X
            default: break;
            }
            ev += (size_t)d * cnt;
            mp += (size_t)d * cnt * stride;
        }
        it++;
        if (a.early && bp_syndrome_ok(a.V, a.ev, a.gdeg, a.gcnt, a.n_groups, stride, b)) break;
    }
    if (a.iters_used) a.iters_used[b] = it;
}

// ---- box-plus alone ----------------------------------------------------------

__global__ void __launch_bounds__(256) bp_boxplus_k(const float *__restrict__ a, const float *__restrict__ b,
                                                    float *__restrict__ out, long count)
{
    const long step = (long)gridDim.x * 256;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < count; i += step) out[i] = bp_boxplus(a[i], b[i]);
}

}  // namespace

int launch_bp_lds(const LdsCode &lc, const ldpc_code *h, const float *llr, uint8_t *hard, float *soft,
                  const DecodeLaunch &L, hipStream_t s, int *lanes_per_codeword)
{
    if (!lds_applicable(h, lc, true)) return -1;
    BpLdsArgs a{};
    a.llr = llr;
    a.hard = hard;
    a.soft = soft;
    a.tab = lc.d_tab;
    a.layers = lc.d_layers;
    a.nl = lc.nl;
    a.n = h->n;
    a.e = h->e;
    a.batch = L.batch;
    a.iters = L.iters;
    // lanes per codeword: the widest layer's, whatever the batch -- a wave's
    // instruction stream is as long with idle lanes, so spreading a small
    // batch over more waves (lds.hip does, with two lanes per check) buys nothing
    a.lpc_log2 = lc.lpc_log2;
    a.early = L.early;
    a.iters_used = L.iters_used;
    a.tab_bytes = lc.tab_bytes;
    if (lanes_per_codeword) *lanes_per_codeword = 1 << lc.lpc_log2;
    const int cpw = 64 >> lc.lpc_log2;
    dim3 grid((L.batch + cpw - 1) / cpw), block(64);
    hipLaunchKernelGGL(bp_lds_decode, grid, block, lds_bytes(h, lc, true), s, a);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_bp_generic(const DecodeLaunch &L, hipStream_t s)
{
    BpGenArgs a{};
    a.V = (float *)L.V;
    a.msg = (float *)L.msg;
    a.ev = L.d_edge_var;
    a.gdeg = L.d_group_deg;
    a.gcnt = L.d_group_cnt;
    a.n_groups = L.n_groups;
    a.stride = L.stride;
    a.batch = L.batch;
    a.iters = L.iters;
    a.early = L.early;
    a.iters_used = L.iters_used;
    dim3 grid((L.batch + 63) / 64), block(64);
    hipLaunchKernelGGL(bp_generic_decode, grid, block, 0, s, a);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// a [+] b, element by element, on the device: the twin of ldpc_boxplus_f32_host
// (host.cpp) -- the only way to look at the box-plus of the kernels alone
extern "C" int ldpc_boxplus_f32_async(ldpc_ctx *c, void *s, const float *d_a, const float *d_b, float *d_out,
                                      long count)
{
    if (!c || count < 0 || (count > 0 && (!d_a || !d_b || !d_out))) return ldpc_set_error(LDPC_EINVAL, "boxplus args");
    if (c->device < 0) return host_only(c);
    if (count == 0) return LDPC_OK;
    HIP_TRY(hipSetDevice(c->device));
    const long blocks = (count + 255) / 256;
    hipLaunchKernelGGL(bp_boxplus_k, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, (hipStream_t)s,
                       d_a, d_b, d_out, count);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return ldpc_set_error(LDPC_EDEVICE, "boxplus: %s", hipGetErrorString(e));
    return LDPC_OK;
}
