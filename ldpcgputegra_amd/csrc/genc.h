// genc.h -- general GF(2) encoder: the host object (genc_host.cpp); its device copy
// and kernel launch are in genc_dev.h (genc.hip).
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "ldpc_internal.h"

// Dense M x N bit matrix the elimination may hold (documented in
// include/ldpc_mi355x.h and DESIGN.md): 20000x10000, the largest shipped
// table, is 10000 rows x 313 words = 25 MB.
constexpr size_t kGencMaxDenseBytes = 64ull << 20;

// tile of the kernel: kGencCols parity columns (one per thread) x kGencCw
// codewords per workgroup, K walked in chunks of kGencChunk 64-bit words
constexpr int kGencCols = 256;
constexpr int kGencCw = 16;
constexpr int kGencChunk = 16;

struct ldpc_encoder {
    const ldpc_code *code = nullptr;   // must outlive the encoder (IRA delegation reads its table)
    uint64_t code_hash = 0;            // of (n, m, groups, edges): "the same code" for ldpc_ctx_set_encoder
    int n = 0, m = 0, k = 0, rank = 0;
    bool systematic = false;
    bool ira = false;                  // Annex-B code: ldpc_dvbs2_encode / _async do the work, no matrix
    std::vector<int32_t> info_pos;     // [k] ascending
    std::vector<int32_t> parity_pos;   // [rank] ascending
    std::vector<int32_t> forced_pos;   // [m - rank] ascending, always 0
    // P word-major: pt[w * stride + j] = bits 64 w .. 64 w + 63 of parity j's
    // row over the information bits (bit i: info i); stride = rank rounded up to
    // kGencCols, the padding columns zero
    int kw = 0, stride = 0;
    std::vector<uint64_t> pt;
};

uint64_t genc_code_hash(const ldpc_code *h);
