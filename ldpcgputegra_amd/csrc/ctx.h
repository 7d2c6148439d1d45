// ctx.h -- the decoder context and the decode request, shared by the C-ABI
// entry points (capi.hip) and the decode dispatcher (dispatch.hip).
#pragma once
#include <cstdlib>
#include <utility>

#include "kernels.h"
#include "ldpc_internal.h"
#include "windowed.h"
#include "coop.h"
#include "stairf.h"
#include "lds.h"
#include "encode.h"
#include "genc_dev.h"

#define HIP_TRY(expr)                                                                          \
    do {                                                                                       \
        hipError_t _e = (expr);                                                                \
        if (_e != hipSuccess)                                                                  \
            return ldpc_set_error(LDPC_EDEVICE, "%s: %s", #expr, hipGetErrorString(_e));       \
    } while (0)

// per-decode device scratch (lazily sized)
struct Scratch {
    void *d_V = nullptr;
    size_t V_bytes = 0;
    void *d_msg = nullptr;
    size_t msg_bytes = 0;
    void *d_early = nullptr;        // coop early termination: live[stride] u8, bad[stride] u32, iters[stride]
    size_t early_bytes = 0;
    void *d_V2 = nullptr;           // coop3 staged early termination: compacted state, map | iterations | count
    size_t V2_bytes = 0;
    void *d_et2 = nullptr;
    size_t et2_bytes = 0;
    void release()
    {
        (void)hipFree(d_V);
        (void)hipFree(d_msg);
        (void)hipFree(d_early);
        (void)hipFree(d_V2);
        (void)hipFree(d_et2);
        *this = Scratch{};
    }
};

struct Lane {
    hipStream_t stream = nullptr;
    Scratch sc;
    void *d_io = nullptr;           // chunk input (LLRs) | output (hard decisions)
    size_t io_bytes = 0;
    hipEvent_t h2d_done = nullptr;  // this lane's input copy finished (the next lane's copy waits on it)
};

struct ldpc_ctx {
    const ldpc_code *code = nullptr;
    int device = 0;
    int max_batch = 0;
    int max_stride = 0;
    int kernel = LDPC_KERNEL_AUTO;  // the family asked for (ldpc_ctx_set_kernel)
    int last_kernel = 0;
    int last_et_stage = 0;          // coop3 staged early termination: first-stage iterations (0: one launch)
    int last_lds_lanes = 0;         // LDPC_KERNEL_LDS's last launch: lanes per codeword, two lanes per check or not
    int last_lds_split = 0;         // (0 / 0 when the last decode was not on that kernel)
    int last_skipped = 0;   // the preferred kernel the last decode could not use at its batch size (0: none)
    bool bp_staircase = false;   // LDPC_ALGO_BP may run on the staircase kernel (ldpc_ctx_set_bp_staircase)
    bool f16_all_codes = false;  // the binary16 decode takes every code: ldsh / generich (ldpc_ctx_set_f16_all_codes)
    bool f16_edge_parallel = false;   // the binary16 decode runs family 9 where it fits: ldseph (ldpc_ctx_set_f16_edge_parallel)
    bool i8_edge_parallel = false;    // the int8 decode runs family 9 where it fits: ldsepi (ldpc_ctx_set_i8_edge_parallel)
    bool ep_wide = false;  // float min-sum may run ldsepw, family 9 spread over several waves (ldpc_ctx_set_ep_wide)
    bool i8_ep_wide = false;  // the int8 decode may run ldsepwi, family 9 over several waves (ldpc_ctx_set_i8_ep_wide)
    int last_ep_waves = 0;  // waves per codeword (float) or pair (int8) of the last launch if it was ldsepw / ldsepwi, else 0
    int lds_pad = 0;        // extra dynamic LDS per windowed2 workgroup (ldpc_ctx_set_lds_pad)
    hipStream_t stream = nullptr;
    // device copy of the code
    uint32_t *d_edge_var = nullptr;
    int *d_group_deg = nullptr, *d_group_cnt = nullptr;
    WindowedCode wcode{};           // windowed-kernel tables (windowed.hip)
    Windowed2Code w16{};            // windowed2.hip tables, S = 16
    CoopCode coop{};                // coop.hip tables (workgroup-cooperative DVB-S2 path)
    CoopCode coop3{};               // coop3.hip tables (pre + post slab waves, i16 chain, D0 = 7)
    LdsCode lds{};                  // lds.hip tables (LDS-resident short-code decoder)
    StairfCode stairf{};            // stairf.hip table (float staircase codes)
    EncodeCode enc{};               // encode.hip table (DVB-S2 IRA encoder)
    bool genc_attached = false;     // ldpc_ctx_set_encoder: an encoder of this code is attached
    bool genc_ira = false;          // ... which delegates to enc (Annex-B code), else:
    GencDev genc{};                 // genc.hip copy of the attached general encoder
    Scratch sc;                     // device-API decodes and the unchunked host path
    void *d_io = nullptr;           // staging for the quantiser's host-buffer API
    size_t io_bytes = 0;
    // host-buffer API pipeline (decode_host): chunk i of a batch runs on lane
    // i % lanes.size(): its own stream, scratch and input / output staging
    std::vector<Lane> lanes;
    // asynchronous host-buffer API: an event of the context's own, recorded
    // after each call's D2H copy (ldpc_ctx_synchronize / destroy wait on it,
    // never on the caller's stream, which may be gone by then; a call on
    // another stream waits on it before reusing d_io and the scratch)
    hipEvent_t host_done = nullptr;
    bool host_pending = false;
    // kernel timing (ldpc_ctx_profile)
    bool profile = false;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> events;
};

// shared between capi.hip and dispatch.hip only: not exported from the library
#define LDPC_LOCAL __attribute__((visibility("hidden")))

inline int getenv_int(const char *name, int def)
{
    const char *e = getenv(name);
    return (e && *e) ? atoi(e) : def;
}

// grow *p to `need` bytes (capi.hip); the old contents are not kept
LDPC_LOCAL int ensure(void **p, size_t *have, size_t need);
// device = -1 context handed to a device-buffer entry point (capi.hip)
LDPC_LOCAL int host_only(const ldpc_ctx *c);
LDPC_LOCAL int check_params(const ldpc_ctx *c, int batch, int n_iter, const ldpc_params *p, bool is_float);

// error count requested with a decode (ldpc_decode_*_count_async)
struct ErrCount {
    int k;
    const uint8_t *ref;
    unsigned long long *counts;
};

// one decode of device buffers, frame-major unless nm_ld is set
struct DecodeRequest {
    const void *d_llr;
    uint8_t *d_hard;
    void *d_soft;
    int32_t *d_iters;
    int batch, n_iter;
    const ldpc_params *p;
    bool is_float;
    size_t nm_ld = 0;               // int8 input is node-major with this pitch (0: frame-major)
    const ErrCount *ec = nullptr;   // NULL: no count
};

// dispatch.hip: queue the decode on s, with sc as its scratch
LDPC_LOCAL int decode_device(ldpc_ctx *c, Scratch &sc, hipStream_t s, const DecodeRequest &rq);
// size sc for that decode and queue nothing (the host-buffer paths size every
// lane before they queue any work: a hipFree mid-pipeline would wait for the
// device)
LDPC_LOCAL int reserve_scratch(ldpc_ctx *c, Scratch &sc, const DecodeRequest &rq);
