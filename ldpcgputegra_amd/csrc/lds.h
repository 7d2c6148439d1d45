// lds.h -- LDS-resident layered decoder for short codes (lds.hip).
#pragma once
#include <vector>

#include "kernels.h"
#include "ldpc_internal.h"

constexpr size_t kLdsMaxBytes = 64 * 1024;   // per wave (one workgroup); 160 KB per CU

struct LdsCode {
    int valid;
    int nl;            // layers per iteration
    int max_width;     // checks in the widest layer
    int lpc_log2;      // lanes per codeword (log2)
    int tab_bytes;     // LDS bytes of the u16 edge table (16-B aligned)
    uint16_t *d_tab;   // [E] layer-major edge -> variable
    int4 *d_layers;    // [nl] (edge base, checks, degree, later-group flag)
    // edge-parallel float kernel (ldsep.hip): compiled shape, layers, per-slot lane table
    int ep_valid = 0, ep_nl = 0, ep_shape = -1;
    uint32_t *d_ep_tab = nullptr;
    // what the int8 form (ldsepi.hip) needs of each layer besides the table: its check degree (4 bits per
    // layer) and whether it is of a later degree group (bit l)
    unsigned long long ep_degs = 0;
    uint32_t ep_later = 0;
    // the same kernel spread over several waves (ldsepw.hip): layers, passes of 8 checks in the widest layer,
    // the W compiled for the table (bit W set), per-slot lane table [epw_nl * epw_np][64]
    int epw_valid = 0, epw_nl = 0, epw_np = 0, epw_mask = 0;
    uint32_t *d_epw_tab = nullptr;
    // what the int8 form of that kernel (ldsepwi.hip) needs besides: as ep_degs / ep_later, of the wide plan's layers
    unsigned long long epw_degs = 0;
    uint32_t epw_later = 0;
};

// host-side plan of ldsepw (no GPU): what ldpc_code_ep_wide_info reports
struct EpwPlan {
    int nl = 0, np = 0, mask = 0;   // mask 0: the table does not qualify
};

int lds_upload(const ldpc_code *h, LdsCode *lc);
void lds_free(LdsCode *lc);
size_t lds_bytes(const ldpc_code *h, const LdsCode &lc, bool is_float);
bool lds_applicable(const ldpc_code *h, const LdsCode &lc, bool is_float);   // fits in LDS
bool lds_preferred(const ldpc_code *h, const LdsCode &lc, bool is_float);    // auto selection
// edge-parallel float kernel (kernel 9, ldsep.hip): one wave per codeword, one lane per edge
int ldsep_upload(const ldpc_code *h, const std::vector<int4> &layers, LdsCode *lc);
bool ldsep_applicable(const ldpc_code *h, const LdsCode &lc, bool is_float);
int launch_ldsep(const LdsCode &lc, const ldpc_code *h, const float *llr, uint8_t *hard, float *soft, int batch,
                 int iters, const DecodeLaunch &L, hipStream_t s);
// its int8 form behind ldpc_ctx_set_i8_edge_parallel (ldsepi.hip): two codewords per lane as i16 halves.
// Applicable where the float kernel is; ldsepi_params_ok: the parameter domain it takes (var_min >= -127)
bool ldsepi_applicable(const ldpc_code *h, const LdsCode &lc);
bool ldsepi_params_ok(const ldpc_params *p);
int launch_ldsepi(const LdsCode &lc, const ldpc_code *h, const int8_t *llr, uint8_t *hard, int8_t *soft,
                  const DecodeLaunch &L, hipStream_t s);
// edge-parallel float kernel over W waves per codeword (ldsepw.hip; kernel 9 behind ldpc_ctx_set_ep_wide)
EpwPlan ldsepw_plan(const ldpc_code *h, const std::vector<int4> &layers);
int ldsepw_upload(const ldpc_code *h, const std::vector<int4> &layers, LdsCode *lc);
bool ldsepw_applicable(const ldpc_code *h, const LdsCode &lc, bool is_float);
// W the fitted rule launches at `batch` among mask (never 0 for a mask != 0); *beats_old: whether that W was
// measured faster than the family the table ran on before
int ldsepw_rule(int nl, int np, int mask, int batch, bool *beats_old);
// W of this launch: LDPC_EPW_WAVES if set, else the rule's; 0 when the forced W is not compiled for the table
int ldsepw_waves(const LdsCode &lc, int batch);
int launch_ldsepw(const LdsCode &lc, const ldpc_code *h, const float *llr, uint8_t *hard, float *soft, int batch,
                  int iters, int waves, const DecodeLaunch &L, hipStream_t s);
// its int8 form behind ldpc_ctx_set_i8_ep_wide (ldsepwi.hip): one workgroup of W waves per pair of codewords, on
// ldsepw's plan and table.  ldsepwi_mask: the W compiled for a plan in int8 (bit W set); the parameter domain is
// ldsepi_params_ok; ldsepwi_rule / ldsepwi_waves as ldsepw_rule / ldsepw_waves, fitted to the int8 measurement
int ldsepwi_mask(int nl, int np);
bool ldsepwi_applicable(const ldpc_code *h, const LdsCode &lc);
int ldsepwi_rule(int nl, int np, int mask, int batch, bool *beats_old);
int ldsepwi_waves(const LdsCode &lc, int batch);
int launch_ldsepwi(const LdsCode &lc, const ldpc_code *h, const int8_t *llr, uint8_t *hard, int8_t *soft, int waves,
                   const DecodeLaunch &L, hipStream_t s);
// reads frame-major llr, writes frame-major hard / soft directly (no interleave);
// *lanes_per_codeword / *split (either may be null): the shape launched
int launch_lds(const LdsCode &lc, const ldpc_code *h, const void *llr, uint8_t *hard, void *soft, int batch,
               int iters, const DecodeLaunch &L, hipStream_t s, int *lanes_per_codeword = nullptr,
               int *split = nullptr);
// belief propagation on the same tables (bp.hip; float, one lane per check, never split)
int launch_bp_lds(const LdsCode &lc, const ldpc_code *h, const float *llr, uint8_t *hard, float *soft,
                  const DecodeLaunch &L, hipStream_t s, int *lanes_per_codeword = nullptr);
