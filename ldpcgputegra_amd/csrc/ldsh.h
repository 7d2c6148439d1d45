// ldsh.h -- the binary16 decode of the codes without a staircase: the packed
// LDS-resident kernel (ldsh_kernel.h, kernel family 7 on LdsCode's tables) and
// the packed any-H kernel (generich.hip, kernel family 1).  Both hold two
// codewords per 32-bit lane and compute the half contract.
#pragma once
#include "lds.h"

// The launch shape of ldsh at this batch: lanes per pair (log2) and two lanes
// per check or not -- LDPC_LDSH_LANES (8 / 16 / 32 / 64) if set, else the rule
// (ldpc_f16_lds_shape_rule, a cost model fitted to measured runs, ldsh.hip).
// -1: the forced shape cannot run this code (fewer lanes than the widest layer
// needs, or more than 64 KB of LDS); nothing is launched then.
int ldsh_shape(const ldpc_code *h, const LdsCode &lc, int batch, int *lpp_log2, int *split);
// reads frame-major llr, writes frame-major hard / soft / L.iters_used directly;
// L.algo / L.beta / L.early / L.iters of the request (beta rounded here)
int launch_ldsh(const LdsCode &lc, const ldpc_code *h, const uint16_t *llr, uint8_t *hard, uint16_t *soft,
                const DecodeLaunch &L, int lpp_log2, int split, hipStream_t s);

// ldseph (ldseph.hip): the binary16 form of the edge-parallel kernel, family 9 on
// LdsCode::d_ep_tab, one wave per pair of codewords; behind
// ldpc_ctx_set_f16_edge_parallel.  Applicable where the float kernel is (the
// same LDS bytes per wave).  Frame-major in and out, no scratch.
bool ldseph_applicable(const ldpc_code *h, const LdsCode &lc);
int launch_ldseph(const LdsCode &lc, const ldpc_code *h, const uint16_t *llr, uint8_t *hard, uint16_t *soft,
                  const DecodeLaunch &L, hipStream_t s);

// generich: V[node][stride] and msg[edge][stride] binary16 in L.V / L.msg (the
// messages zeroed by the caller), one lane per pair of codewords.  The stride is
// the batch rounded up to 128: a wave's piece of a row is one whole run of 64
// pairs (256 B).
inline int generich_stride(int batch) { return (batch + 127) / 128 * 128; }
int launch_generich(const DecodeLaunch &L, hipStream_t s);
