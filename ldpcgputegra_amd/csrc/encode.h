// encode.h -- on-device bit source and DVB-S2 IRA encoder (encode.hip).
#pragma once
#include <cstddef>
#include <cstdint>

#include "kernels.h"
#include "ldpc_internal.h"

// one workgroup encodes one codeword out of LDS: K information bytes, M parity
// bytes (each rounded up to 16) and the scan's wave totals.  Dynamic LDS up to
// this limit needs no function attribute; every N = 64800 code of rate >= 1/2
// and every N = 16200 code fits.
constexpr size_t kEncMaxLds = 64 * 1024;
constexpr int kEncThreads = 384;   // 6 waves: thread t < 360 is column t of the quasi-cyclic form

struct EncodeCode {
    bool valid = false;      // an Annex-B code whose codeword fits one workgroup's LDS
    int q = 0, k = 0, m = 0;
    int p_off = 0, w_off = 0;   // LDS offsets of the parity bytes / the wave totals
    unsigned lds_bytes = 0;
    // [q + 1] first entry of residue s = 0 .. q, then the entries sorted by s:
    // (360 g) << 16 | tx for the address x = q tx + s of table row g
    uint32_t *d_tab = nullptr;
};

// leaves ec->valid false (and returns LDPC_OK) for a code without an Annex-B
// table or one too long for the kernel
int encode_upload(const ldpc_code *h, EncodeCode *ec);
void encode_free(EncodeCode *ec);
// LDS bytes one codeword of the code needs (the kernel's layout)
size_t encode_lds_bytes(int k, int m);

int launch_info_bits(uint8_t *info, int k, int batch, uint64_t first_cw, uint64_t seed, hipStream_t s);
int launch_dvbs2_encode(const EncodeCode &ec, const uint8_t *info, uint8_t *codeword, int batch, hipStream_t s);
