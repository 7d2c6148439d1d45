// stairh.h -- binary16 layered min-sum for staircase (DVB-S2 IRA) codes: the
// packed half-precision element type of kernel family 11 (stairh_kernel.h), on
// stairf's tables (StairfCode).
#pragma once
#include "stairf.h"

// V offsets are u32 bytes of 2-byte elements: (n + 1) * stride * 2 < 2^32 (stride <= 33088 for n = 64800)
bool stairh_stride_ok(const StairfCode &sc, int n, int stride);
// V and message scratch of one decode (messages in the kernel's own layout, zeroed by the caller)
size_t stairh_v_bytes(int n, int stride);
size_t stairh_msg_bytes(const StairfCode &sc, int stride);
// group width S of a launch at this stride (0: the code has no table)
int stairh_width(const StairfCode &sc, int stride);
// L.V / L.msg: the binary16 state; L.beta: the float beta of the request (rounded here)
int launch_stairh(const DecodeLaunch &L, const StairfCode &sc, hipStream_t s);

// frame-major [batch][N] binary16 <-> V[N][stride] (layout.hip): the load clamps
// to +-1024, the store's hard decision is V > 0 as a binary16 comparison
int launch_interleave_f16(const uint16_t *llr, uint16_t *V, int n, int batch, int stride, hipStream_t s);
int launch_deinterleave_f16(const uint16_t *V, uint8_t *hard, uint16_t *soft, int n, int batch, int stride,
                            hipStream_t s);
// h = RNE16(min(max(y, -1024), 1024))
int launch_convert_f32_f16(const float *y, uint16_t *h, long count, hipStream_t s);
