// host.h -- the host decoder behind the C-ABI's device = -1 contexts (host.cpp).
#pragma once
#include "ldpc_internal.h"

bool host_has_avx2();
// frame-major [batch][N] in, 0/1 hard decisions out; same semantics as the device decoders
int host_decode_i8(const ldpc_code *h, const int8_t *llr, uint8_t *hard, int batch, int n_iter, const ldpc_params *p);
// soft (final V, [batch][N]) and iters_used ([batch]) may be NULL
int host_decode_f32(const ldpc_code *h, const float *llr, uint8_t *hard, float *soft, int32_t *iters_used, int batch,
                    int n_iter, const ldpc_params *p);
// binary16 (bit patterns), the half contract of DESIGN.md §3: the definition the packed kernel is compared with
int host_decode_f16(const ldpc_code *h, const uint16_t *llr, uint8_t *hard, uint16_t *soft, int32_t *iters_used,
                    int batch, int n_iter, const ldpc_params *p);
// RNE16(min(max(y, -1024), 1024))
uint16_t host_f16_from_f32(float y);
