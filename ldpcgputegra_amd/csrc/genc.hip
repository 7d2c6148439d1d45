// genc.hip -- device twin of ldpc_encode (genc_host.cpp): the GF(2) product
// parity[b][j] = parity(popcount(P[j] & info[b])) for any code.
//
// A workgroup owns kGencCols parity columns (thread t: column j0 + t) of
// kGencCw codewords.  It walks K in chunks of kGencChunk 64-bit words: the
// four waves pack the chunk's information bytes of the tile's codewords into
// words in LDS, one wave64 ballot per word (lane l holds information bit
// 64 w + l); then every thread loads its column's word of P once per w --
// P is stored word-major, Pt[w][j], so the lanes' loads are consecutive --
// and folds it into one 64-bit accumulator per codeword with the codeword's
// word read from LDS (all lanes read one address: a broadcast, no bank
// conflict).  parity = popcount(acc) & 1 at the end.  The workgroups of the
// first column tile also write the information bytes and the forced zeros, so
// every byte of the codeword is written exactly once.
#include "genc_dev.h"

namespace {

inline int ok() { return hipGetLastError() == hipSuccess ? 0 : -1; }

// SYS: a systematic code of full rank -- information positions 0 .. K-1,
// parity positions K .. N-1, nothing forced (no position tables, contiguous
// stores)
template <bool SYS>
__global__ void __launch_bounds__(kGencCols) genc_k(const uint8_t *__restrict__ info, uint8_t *__restrict__ cw,
                                                    const uint64_t *__restrict__ pt,
                                                    const int32_t *__restrict__ info_pos,
                                                    const int32_t *__restrict__ parity_pos,
                                                    const int32_t *__restrict__ forced_pos, int N, int K, int rank,
                                                    int n_forced, int kw, int stride, int batch)
{
    __shared__ __attribute__((aligned(16))) uint64_t sI[kGencChunk * kGencCw];   // [w][codeword]
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int j = blockIdx.x * kGencCols + t;              // < stride: Pt is padded with zero columns
    const int b0 = blockIdx.y * kGencCw;
    const int nb = min(kGencCw, batch - b0);               // >= 1
    const bool first = blockIdx.x == 0;

    uint64_t acc[kGencCw];
#pragma unroll
    for (int b = 0; b < kGencCw; b++) acc[b] = 0;

    for (int w0 = 0; w0 < kw; w0 += kGencChunk) {
        const int cw_n = min(kGencChunk, kw - w0);
        // the column's words of P for the chunk, issued ahead of the packing
        // (zero past the end: such a word folds nothing in, whatever LDS holds)
        uint64_t p[kGencChunk];
#pragma unroll
        for (int w = 0; w < kGencChunk; w++) p[w] = w < cw_n ? pt[(size_t)(w0 + w) * stride + j] : 0;
        if (w0) __syncthreads();                           // the previous chunk's readers are done
        // word w of codewords wave, wave + 4, .. (wave-uniform): the loads of a
        // word's kGencCw / 4 codewords are in flight together
        for (int w = 0; w < cw_n; w++) {
            const int i = (w0 + w) * 64 + lane;
            constexpr int NW = kGencCols / 64;
            uint8_t bit[kGencCw / NW];
#pragma unroll
            for (int u = 0; u < kGencCw / NW; u++) {
                const int b = wave + NW * u;
                bit[u] = (b < nb && i < K) ? info[(size_t)(b0 + b) * K + i] & 1 : 0;
            }
#pragma unroll
            for (int u = 0; u < kGencCw / NW; u++) {
                const int b = wave + NW * u;
                if (first && b < nb && i < K) cw[(size_t)(b0 + b) * N + (SYS ? i : info_pos[i])] = bit[u];
                const unsigned long long word = __ballot(bit[u]);
                if (lane == 0) sI[w * kGencCw + b] = word;
            }
        }
        __syncthreads();
#pragma unroll
        for (int w = 0; w < kGencChunk; w++) {
#pragma unroll
            for (int b = 0; b < kGencCw; b++) acc[b] ^= p[w] & sI[w * kGencCw + b];
        }
    }

    if (j < rank) {
        const size_t col = SYS ? (size_t)K + j : (size_t)parity_pos[j];
#pragma unroll
        for (int b = 0; b < kGencCw; b++)
            if (b < nb) cw[(size_t)(b0 + b) * N + col] = (uint8_t)(__popcll(acc[b]) & 1);
    }
    if (!SYS && first)
        for (int x = t; x < n_forced * nb; x += kGencCols)
            cw[(size_t)(b0 + x / n_forced) * N + forced_pos[x % n_forced]] = 0;
}

template <typename T>
int up(T **d, const T *src, size_t count, const char *what)
{
    *d = nullptr;
    if (count == 0) return LDPC_OK;
    if (hipMalloc(d, count * sizeof(T)) != hipSuccess) {
        *d = nullptr;
        return ldpc_set_error(LDPC_ENOMEM, "general encoder: %s (%zu bytes)", what, count * sizeof(T));
    }
    if (hipMemcpy(*d, src, count * sizeof(T), hipMemcpyHostToDevice) != hipSuccess)
        return ldpc_set_error(LDPC_EDEVICE, "general encoder: %s upload", what);
    return LDPC_OK;
}

}  // namespace

int genc_upload(const ldpc_encoder *e, GencDev *g)
{
    *g = GencDev{};
    const bool contiguous = e->systematic && e->rank == e->m;
    int rc;
    if ((rc = up(&g->d_pt, e->pt.data(), e->pt.size(), "P")) != LDPC_OK ||
        (!contiguous &&
         ((rc = up(&g->d_info_pos, e->info_pos.data(), e->info_pos.size(), "information positions")) != LDPC_OK ||
          (rc = up(&g->d_parity_pos, e->parity_pos.data(), e->parity_pos.size(), "parity positions")) != LDPC_OK ||
          (rc = up(&g->d_forced_pos, e->forced_pos.data(), e->forced_pos.size(), "forced positions")) != LDPC_OK))) {
        genc_free(g);
        return rc;
    }
    g->n = e->n;
    g->k = e->k;
    g->rank = e->rank;
    g->n_forced = (int)e->forced_pos.size();
    g->kw = e->kw;
    g->stride = e->stride;
    g->systematic = contiguous;
    g->valid = true;
    return LDPC_OK;
}

void genc_free(GencDev *g)
{
    if (g->d_pt) (void)hipFree(g->d_pt);
    if (g->d_info_pos) (void)hipFree(g->d_info_pos);
    if (g->d_parity_pos) (void)hipFree(g->d_parity_pos);
    if (g->d_forced_pos) (void)hipFree(g->d_forced_pos);
    *g = GencDev{};
}

int launch_genc(const GencDev &g, const uint8_t *info, uint8_t *codeword, int batch, hipStream_t s)
{
    if (batch <= 0) return 0;
    // the y dimension of a grid holds 65535 workgroups: larger batches go in slices
    const int slice = 65535 * kGencCw;
    for (long b = 0; b < batch; b += slice) {
        const int nb = (int)(batch - b < slice ? batch - b : slice);
        const dim3 grid(g.stride / kGencCols, (nb + kGencCw - 1) / kGencCw);
        const uint8_t *in = info + (size_t)b * g.k;
        uint8_t *out = codeword + (size_t)b * g.n;
        if (g.systematic)
            hipLaunchKernelGGL(genc_k<true>, grid, dim3(kGencCols), 0, s, in, out, g.d_pt, g.d_info_pos,
                               g.d_parity_pos, g.d_forced_pos, g.n, g.k, g.rank, g.n_forced, g.kw, g.stride, nb);
        else
            hipLaunchKernelGGL(genc_k<false>, grid, dim3(kGencCols), 0, s, in, out, g.d_pt, g.d_info_pos,
                               g.d_parity_pos, g.d_forced_pos, g.n, g.k, g.rank, g.n_forced, g.kw, g.stride, nb);
    }
    return ok();
}
