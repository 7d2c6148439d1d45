// genc_dev.h -- device copy of a general encoder and its kernel launch (genc.hip).
#pragma once
#include "genc.h"
#include "kernels.h"

// device copy of one encoder, owned by a context
struct GencDev {
    bool valid = false;
    int n = 0, k = 0, rank = 0, n_forced = 0, kw = 0, stride = 0;
    bool systematic = false;
    uint64_t *d_pt = nullptr;
    int32_t *d_info_pos = nullptr, *d_parity_pos = nullptr, *d_forced_pos = nullptr;
};

int genc_upload(const ldpc_encoder *e, GencDev *g);
void genc_free(GencDev *g);
int launch_genc(const GencDev &g, const uint8_t *info, uint8_t *codeword, int batch, hipStream_t s);
