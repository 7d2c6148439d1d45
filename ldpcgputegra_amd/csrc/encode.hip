// encode.hip -- the head of the Monte-Carlo chain on the device: the bit
// source (the reference's CBitGenerator::generate, code/x86/main_p.cpp:431-445)
// and the DVB-S2 IRA encoder (GenericEncoder::encode,
// code/x86/CEncoder/GenericEncoder.cpp:38-78; host twin: ldpc_dvbs2_encode,
// code.cpp).
//
// Encoder: the quasi-cyclic form of the Annex-B rule.  Write a table address
// of row g as x = q tx + sx (0 <= sx < q, 0 <= tx < 360).  Information bit
// 360 g + k hits check (x + k q) mod 360 q = q ((tx + k) mod 360) + sx, so with
// the checks viewed as A[s][t] (check r = q t + s) every (row, address) pair
// adds the 360-bit group info[g], rotated by tx, into A[sx].  One workgroup
// encodes one codeword, thread t < 360 is column t: it reads
// info[360 g + (t - tx) mod 360] for the entries of s = 0, 1, .. q - 1 in turn
// (the table is sorted by sx on the host), which are exactly the accumulators
// of its own run of checks r = q t .. q t + q - 1 in staircase order.  So the
// accumulators never leave the thread's registers: it keeps the running XOR of
// its run, stores that local prefix as parity byte q t + s, and the carry into
// the run -- the exclusive prefix-XOR of the 360 run totals -- comes from one
// ballot per wave plus the six wave totals through LDS.
#include <algorithm>
#include <vector>

#include "encode.h"

namespace {

inline int ok() { return hipGetLastError() == hipSuccess ? 0 : -1; }

LDPC_DEV uint4 and1(uint4 v)
{
    return make_uint4(v.x & 0x01010101u, v.y & 0x01010101u, v.z & 0x01010101u, v.w & 0x01010101u);
}
LDPC_DEV uint2 and1(uint2 v) { return make_uint2(v.x & 0x01010101u, v.y & 0x01010101u); }
LDPC_DEV uint8_t and1(uint8_t v) { return v & 1; }

// info[e] = bit 63 of splitmix64((base + e) ^ key), e the flat index b K + i of
// the [batch][K] array (base = first_cw K): 8 bytes per lane and step
__global__ void __launch_bounds__(256) info_bits_k(uint8_t *__restrict__ info, size_t total, uint64_t base,
                                                   uint64_t key, int vec)
{
    for (size_t e = ((size_t)blockIdx.x * 256 + threadIdx.x) * 8; e < total; e += (size_t)gridDim.x * 256 * 8) {
        uint32_t w[2] = {0, 0};
#pragma unroll
        for (int j = 0; j < 8; j++)
            w[j >> 2] |= (uint32_t)(splitmix64((base + e + j) ^ key) >> 63) << (8 * (j & 3));
        if (vec && e + 8 <= total) {
            *(uint2 *)(info + e) = make_uint2(w[0], w[1]);
        } else {
#pragma unroll
            for (int j = 0; j < 8; j++)
                if (e + j < total) info[e + j] = (uint8_t)(w[j >> 2] >> (8 * (j & 3)));
        }
    }
}

// V: the widest vector the rows' alignment allows (uint4 / uint2 / uint8_t)
template <typename V>
__global__ void __launch_bounds__(kEncThreads) dvbs2_encode_k(const uint8_t *__restrict__ info,
                                                              uint8_t *__restrict__ cw,
                                                              const uint32_t *__restrict__ tab, int K, int M, int q,
                                                              int p_off, int w_off)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char enc_smem[];
    uint8_t *sI = enc_smem;                        // [K] information bits
    uint8_t *sP = enc_smem + p_off;                // [M] parity, check order
    uint32_t *sW = (uint32_t *)(enc_smem + w_off); // [6] run-total parity of each wave
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const uint8_t *in = info + (size_t)blockIdx.x * K;
    uint8_t *out = cw + (size_t)blockIdx.x * ((size_t)K + M);

    // systematic part: one global load feeds LDS and the codeword
    for (int i = t; i < K / (int)sizeof(V); i += kEncThreads) {
        const V v = and1(((const V *)in)[i]);
        ((V *)sI)[i] = v;
        ((V *)out)[i] = v;
    }
    __syncthreads();

    // thread t: checks q t .. q t + q - 1, local prefix-XOR into sP
    uint32_t run = 0;
    if (t < 360) {
        const uint32_t *ent = tab + q + 1;
        uint8_t *p = sP + q * t;
        uint32_t e = tab[0];
        for (int s = 0; s < q; s++) {
            const uint32_t e1 = tab[s + 1];
#pragma unroll 4
            for (; e < e1; e++) {
                const uint32_t w = ent[e];
                int i = t - (int)(w & 0xFFFFu);
                i += i < 0 ? 360 : 0;
                run ^= sI[(w >> 16) + i];
            }
            p[s] = (uint8_t)run;
        }
    }

    // carry into the run: exclusive prefix-XOR of the run totals
    const unsigned long long mask = __ballot(run & 1);
    if (lane == 0) sW[wave] = (uint32_t)__popcll(mask) & 1u;
    __syncthreads();
    uint32_t carry = (uint32_t)__popcll(mask & ((1ull << lane) - 1ull)) & 1u;
    for (int w = 0; w < wave; w++) carry ^= sW[w];
    if (t < 360 && carry) {
        uint8_t *p = sP + q * t;
        for (int s = 0; s < q; s++) p[s] ^= 1;
    }
    __syncthreads();

    // parity out, coalesced in check order
    uint8_t *po = out + K;
    for (int i = t; i < M / (int)sizeof(V); i += kEncThreads) ((V *)po)[i] = ((const V *)sP)[i];
}

template <typename V>
int launch_enc(const EncodeCode &ec, const uint8_t *info, uint8_t *cw, int batch, hipStream_t s)
{
    hipLaunchKernelGGL(dvbs2_encode_k<V>, dim3(batch), dim3(kEncThreads), ec.lds_bytes, s, info, cw, ec.d_tab, ec.k,
                       ec.m, ec.q, ec.p_off, ec.w_off);
    return ok();
}

}  // namespace

size_t encode_lds_bytes(int k, int m)
{
    return ((size_t)k + 15) / 16 * 16 + ((size_t)m + 15) / 16 * 16 + 32;
}

int encode_upload(const ldpc_code *h, EncodeCode *ec)
{
    *ec = EncodeCode{};
    if (h->dvbs2_q <= 0) return LDPC_OK;
    const int q = h->dvbs2_q, m = h->m, k = h->n - m;
    // the entries pack 360 g into 16 bits; 360 | k and m = 360 q by construction
    if (encode_lds_bytes(k, m) > kEncMaxLds || k > 65536 || k % 360 || m != 360 * q) return LDPC_OK;
    std::vector<std::vector<uint32_t>> by_s(q);
    const int *a = h->dvbs2_row_addr.data();
    for (size_t g = 0; g < h->dvbs2_row_len.size(); g++) {
        for (int j = 0; j < h->dvbs2_row_len[g]; j++) {
            const int x = a[j];   // 0 <= x < m: checked by ldpc_code_from_dvbs2_table
            by_s[x % q].push_back((uint32_t)(360 * g) << 16 | (uint32_t)(x / q));
        }
        a += h->dvbs2_row_len[g];
    }
    std::vector<uint32_t> tab(q + 1);
    for (int s = 0; s < q; s++) {
        tab[s] = (uint32_t)(tab.size() - (q + 1));
        tab.insert(tab.end(), by_s[s].begin(), by_s[s].end());
    }
    tab[q] = (uint32_t)(tab.size() - (q + 1));
    if (hipMalloc(&ec->d_tab, tab.size() * 4) != hipSuccess) {
        ec->d_tab = nullptr;
        return ldpc_set_error(LDPC_ENOMEM, "encoder table");
    }
    if (hipMemcpy(ec->d_tab, tab.data(), tab.size() * 4, hipMemcpyHostToDevice) != hipSuccess) {
        encode_free(ec);
        return ldpc_set_error(LDPC_EDEVICE, "encoder table upload");
    }
    ec->q = q;
    ec->k = k;
    ec->m = m;
    ec->p_off = (k + 15) / 16 * 16;
    ec->w_off = ec->p_off + (m + 15) / 16 * 16;
    ec->lds_bytes = (unsigned)encode_lds_bytes(k, m);
    ec->valid = true;
    return LDPC_OK;
}

void encode_free(EncodeCode *ec)
{
    if (ec->d_tab) (void)hipFree(ec->d_tab);
    *ec = EncodeCode{};
}

int launch_info_bits(uint8_t *info, int k, int batch, uint64_t first_cw, uint64_t seed, hipStream_t s)
{
    const size_t total = (size_t)k * batch;
    if (total == 0) return 0;
    const int blocks = (int)std::min<size_t>((total + 2047) / 2048, 8192);
    hipLaunchKernelGGL(info_bits_k, dim3(blocks), dim3(256), 0, s, info, total, first_cw * (uint64_t)k,
                       seed * 0xA0761D6478BD642Full, (int)(((uintptr_t)info & 7) == 0));
    return ok();
}

int launch_dvbs2_encode(const EncodeCode &ec, const uint8_t *info, uint8_t *codeword, int batch, hipStream_t s)
{
    if (batch <= 0) return 0;
    // every row of info ([K]) and both parts of every codeword row ([K | M]) start aligned
    const uintptr_t al = (uintptr_t)info | (uintptr_t)codeword | (uintptr_t)ec.k | (uintptr_t)ec.m;
    if ((al & 15) == 0) return launch_enc<uint4>(ec, info, codeword, batch, s);
    if ((al & 7) == 0) return launch_enc<uint2>(ec, info, codeword, batch, s);
    return launch_enc<uint8_t>(ec, info, codeword, batch, s);
}
