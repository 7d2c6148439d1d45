// dispatch.hip -- one decode of device buffers, from request to queued work:
// validate, choose the kernel family, plan and size the scratch, then one of
// two launch bodies (LDS-resident families; families with V and messages in
// device scratch).  Host code only.
#include <algorithm>

#include "ctx.h"

int check_params(const ldpc_ctx *c, int batch, int n_iter, const ldpc_params *p, bool is_float)
{
    if (batch < 0 || batch > c->max_batch)
        return ldpc_set_error(LDPC_EINVAL, "batch %d outside [0, max_batch=%d]", batch, c->max_batch);
    if (n_iter < 0) return ldpc_set_error(LDPC_EINVAL, "n_iter < 0");
    if (!p) return ldpc_set_error(LDPC_EINVAL, "params NULL");
    if (p->algo < 0 || p->algo > LDPC_ALGO_BP) return ldpc_set_error(LDPC_EINVAL, "algo %d", p->algo);
    if (!is_float) {
        if (p->algo == LDPC_ALGO_BP)
            return ldpc_set_error(LDPC_EUNSUPPORTED, "belief propagation takes float input (the reference has no "
                                  "fixed-point BP)");
        // CDecoder_OMS_fixed_SSE::decode / CDecoder_NMS_fixed_SSE::decode exit
        // unless vSAT_POS_VAR == 127 (OMS .cpp:116-119, NMS .cpp:119-122)
        if (p->var_max != 127)
            return ldpc_set_error(LDPC_EUNSUPPORTED, "var_max must be 127 (reference decode_8bits only)");
        if (p->var_min < -128 || p->var_min > 0) return ldpc_set_error(LDPC_EINVAL, "var_min %d", p->var_min);
        if (p->msg_max < 0 || p->msg_max > 127) return ldpc_set_error(LDPC_EINVAL, "msg_max %d", p->msg_max);
        if (p->algo == LDPC_ALGO_OMS && (p->offset < 0 || p->offset > 255))
            return ldpc_set_error(LDPC_EINVAL, "offset %d", p->offset);
    }
    return LDPC_OK;
}

// ---- selection -------------------------------------------------------------

// can family k schedule this context's code at all, whatever the parameters?
static bool family_fits(const ldpc_ctx *c, int k)
{
    switch (k) {
    case LDPC_KERNEL_AUTO:
    case LDPC_KERNEL_GENERIC: return true;
    case LDPC_KERNEL_WINDOWED: return windowed_supported(c->code);
    case LDPC_KERNEL_WINDOWED2: return c->w16.valid;
    case LDPC_KERNEL_COOP: return c->coop.valid;
    case LDPC_KERNEL_LDS: return c->lds.valid;
    case LDPC_KERNEL_COOP3: return c->coop3.valid;
    case LDPC_KERNEL_LDSEP: return c->lds.ep_valid;
    case LDPC_KERNEL_STAIRF: return c->stairf.valid;
    default: return false;   // the retired 4 and 6, LDPC_KERNEL_HOST, out of range
    }
}

bool ldpc_ctx_has_kernel(const ldpc_ctx *c, int k)
{
    if (!c) return false;
    return c->device < 0 ? k == LDPC_KERNEL_AUTO : family_fits(c, k);
}

// kernel family for this call, -1 when the family asked for cannot take these
// parameters.  last_skipped records the fastest kernel of this code that the
// automatic choice could not use for them (algorithm, message / variable
// ranges), 0 if none
static int pick_kernel(ldpc_ctx *c, const ldpc_params *p, bool is_float, int stride, int batch)
{
    c->last_skipped = 0;
    const ldpc_code *h = c->code;
    const bool automatic = c->kernel == LDPC_KERNEL_AUTO;
    const bool sf = family_fits(c, LDPC_KERNEL_STAIRF) && stairf_stride_ok(c->stairf, h->n, stride);
    if (p->algo == LDPC_ALGO_BP) {   // float only (check_params); bp.hip has the LDS-resident and the any-H kernel,
                                     // stairbp.hip the staircase one behind ldpc_ctx_set_bp_staircase
        if (c->kernel == LDPC_KERNEL_LDS) return lds_applicable(h, c->lds, true) ? LDPC_KERNEL_LDS : -1;
        if (c->kernel == LDPC_KERNEL_GENERIC) return LDPC_KERNEL_GENERIC;
        if (c->kernel == LDPC_KERNEL_STAIRF) return (c->bp_staircase && sf) ? LDPC_KERNEL_STAIRF : -1;
        if (!automatic) return -1;
        if (ldsep_applicable(h, c->lds, true))
            c->last_skipped = LDPC_KERNEL_LDSEP;
        else if (sf && c->bp_staircase)
            return LDPC_KERNEL_STAIRF;
        else if (sf || (c->bp_staircase && family_fits(c, LDPC_KERNEL_STAIRF)))
            c->last_skipped = LDPC_KERNEL_STAIRF;   // no BP there (switch off), or on and the stride too large
        return lds_preferred(h, c->lds, true) ? LDPC_KERNEL_LDS : LDPC_KERNEL_GENERIC;
    }
    // family 9 on several waves per codeword (ldsepw), min-sum only: only where the one-wave kernel does not fit
    const bool wide = c->ep_wide && ldsepw_applicable(h, c->lds, is_float);
    // family 9 in int8 (ldsepi), behind ldpc_ctx_set_i8_edge_parallel: the tables of the one-wave kernel
    const bool epi = !is_float && c->i8_edge_parallel && ldsepi_applicable(h, c->lds);
    // the same over several waves (ldsepwi), behind ldpc_ctx_set_i8_ep_wide: the tables of ldsepw
    const bool epwi = !is_float && c->i8_ep_wide && ldsepwi_applicable(h, c->lds);
    switch (c->kernel) {
    case LDPC_KERNEL_LDS: return lds_applicable(h, c->lds, is_float) ? LDPC_KERNEL_LDS : -1;
    case LDPC_KERNEL_LDSEP: {
        const bool i8 = (epi || epwi) && ldsepi_params_ok(p);
        return ldsep_applicable(h, c->lds, is_float) || wide || i8 ? LDPC_KERNEL_LDSEP : -1;
    }
    case LDPC_KERNEL_STAIRF: return (is_float && sf) ? LDPC_KERNEL_STAIRF : -1;
    default: break;
    }
    if (is_float) {
        if (automatic && ldsep_applicable(h, c->lds, true)) return LDPC_KERNEL_LDSEP;
        if (automatic && wide) {   // where the fitted rule found it faster than the family chosen below
            bool beats = false;
            ldsepw_rule(c->lds.epw_nl, c->lds.epw_np, c->lds.epw_mask, batch, &beats);
            if (beats) return LDPC_KERNEL_LDSEP;
        }
        if (automatic && sf) return LDPC_KERNEL_STAIRF;
        if (automatic && lds_preferred(h, c->lds, true)) return LDPC_KERNEL_LDS;
        return c->kernel <= LDPC_KERNEL_GENERIC ? LDPC_KERNEL_GENERIC : -1;
    }
    const bool w1 = family_fits(c, LDPC_KERNEL_WINDOWED) && windowed_params_ok(p);
    const bool w2 = family_fits(c, LDPC_KERNEL_WINDOWED2) && windowed2_params_ok(p);
    const bool co = family_fits(c, LDPC_KERNEL_COOP) && coop_params_ok(p);
    const bool co3 = family_fits(c, LDPC_KERNEL_COOP3) && coop3_params_ok(p, c->coop3) && coop3_stride_ok(stride) &&
                     (!p->early_term || coop3_et_in_kernel(c->coop3, h->n));
    switch (c->kernel) {
    case LDPC_KERNEL_GENERIC: return LDPC_KERNEL_GENERIC;
    case LDPC_KERNEL_WINDOWED: return w1 ? LDPC_KERNEL_WINDOWED : -1;
    case LDPC_KERNEL_WINDOWED2: return w2 ? LDPC_KERNEL_WINDOWED2 : -1;
    case LDPC_KERNEL_COOP: return co ? LDPC_KERNEL_COOP : -1;
    case LDPC_KERNEL_COOP3: return co3 ? LDPC_KERNEL_COOP3 : -1;
    default:
        if (epi) {   // checked first, as for float; outside its domain (var_min = -128) the choice is as before
            if (ldsepi_params_ok(p)) return LDPC_KERNEL_LDSEP;
            c->last_skipped = LDPC_KERNEL_LDSEP;
        }
        if (epwi) {   // inside its domain where the fitted rule found it faster than the family chosen below
            if (ldsepi_params_ok(p)) {
                bool beats = false;
                ldsepwi_rule(c->lds.epw_nl, c->lds.epw_np, ldsepwi_mask(c->lds.epw_nl, c->lds.epw_np), batch, &beats);
                if (beats) return LDPC_KERNEL_LDSEP;
            } else {
                c->last_skipped = LDPC_KERNEL_LDSEP;
            }
        }
        if (co3) return LDPC_KERNEL_COOP3;
        if (family_fits(c, LDPC_KERNEL_COOP3)) c->last_skipped = LDPC_KERNEL_COOP3;
        if (co) return LDPC_KERNEL_COOP;
        if (family_fits(c, LDPC_KERNEL_COOP) && !c->last_skipped) c->last_skipped = LDPC_KERNEL_COOP;
        if (w2) return LDPC_KERNEL_WINDOWED2;
        if (lds_preferred(h, c->lds, false)) return LDPC_KERNEL_LDS;
        if (w1) return LDPC_KERNEL_WINDOWED;
        return LDPC_KERNEL_GENERIC;
    }
}

static int stride_of(int batch) { return (batch + 63) / 64 * 64; }

// frame-major in and out, the whole state in LDS: no V, no messages in scratch
static bool lds_resident(int kern) { return kern == LDPC_KERNEL_LDS || kern == LDPC_KERNEL_LDSEP; }

// what every decode and every reservation starts with: *kern = the family of
// this call (recorded as last_kernel), LDPC_KERNEL_AUTO for an empty batch,
// which touches nothing
static int select_kernel(ldpc_ctx *c, const DecodeRequest &rq, int *kern)
{
    *kern = LDPC_KERNEL_AUTO;
    int rc = check_params(c, rq.batch, rq.n_iter, rq.p, rq.is_float);
    if (rc != LDPC_OK) return rc;
    if (c->device < 0) return host_only(c);
    if (rq.batch == 0) return LDPC_OK;
    HIP_TRY(hipSetDevice(c->device));
    const int k = pick_kernel(c, rq.p, rq.is_float, stride_of(rq.batch), rq.batch);
    if (k < 0)
        return ldpc_set_error(LDPC_EUNSUPPORTED, "kernel %d selected but not applicable to these params", c->kernel);
    int waves = 0;
    // ldsepw, or in int8 ldsepwi (on the tables of the one-wave kernel an int8 decode on family 9 is ldsepi, one wave
    // per pair): refuse before anything is recorded
    if (k == LDPC_KERNEL_LDSEP && !ldsep_applicable(c->code, c->lds, true)) {
        waves = rq.is_float ? ldsepw_waves(c->lds, rq.batch) : ldsepwi_waves(c->lds, rq.batch);
        if (!waves)
            return ldpc_set_error(LDPC_EUNSUPPORTED, "LDPC_EPW_WAVES asks for a number of waves per codeword that is not "
                                  "compiled for this %dx%d code (mask 0x%x)", c->code->n, c->code->m,
                                  rq.is_float ? c->lds.epw_mask : ldsepwi_mask(c->lds.epw_nl, c->lds.epw_np));
    }
    c->last_ep_waves = waves;
    c->last_kernel = *kern = k;
    return LDPC_OK;
}

// ---- scratch ---------------------------------------------------------------

// Device scratch of a decode on a family that keeps V and messages there.
// V is V[n + 1][vpitch] (row n: the sink row of the coop kernel's masked
// stores), the messages a buffer of their own with 4096 sink bytes behind
// them -- except on coop3, which keeps V grouped per 16 codewords and each
// group's messages behind its V rows (vgroup bytes per group, messages from
// vpart), so msg_bytes is then what to zero in each group.
struct ScratchPlan {
    int vpitch;                // V row pitch, codewords
    size_t vgroup, vpart;      // coop3 only, else 0
    size_t v_bytes, msg_bytes;
    size_t early_bytes;        // early termination: bad u32 | iterations used i32 | live u8 (0: none)
    size_t v2_bytes, et2_bytes;
    int et_staged;             // coop3 staged early termination: first-stage iterations (0: one launch)
};

static ScratchPlan plan_scratch(const ldpc_ctx *c, int kern, int stride, const DecodeRequest &rq)
{
    const ldpc_code *h = c->code;
    const size_t esz = rq.is_float ? 4 : 1;
    const bool early = rq.p->early_term != 0;
    ScratchPlan pl{};
    // V row pitch (codewords): the coop kernel pads it by LDPC_VPITCH_PAD
    // (default 64; multiple of 64) codewords.  A workgroup touches its 16-B
    // piece of every row and the XCD remap gives each XCD a fixed 512-B window
    // of a row: with a power-of-two pitch (batch 4096) every row's window of an
    // XCD falls on the same few L2 channels.  Measured (DVB-S2 r1/2, 4096 cw,
    // 50 it, the row-layout coop3 of r02): pitch 4096 57.6 ms, 4160 / 4224
    // 49.7 / 49.6 ms, 4352 50.4, 4608 52.7, 5120 57.2.  coop3
    // keeps V grouped per 16 codewords instead (coop3_group_bytes per group).
    pl.vpitch = stride;
    if (kern == LDPC_KERNEL_COOP) pl.vpitch += std::max(0, getenv_int("LDPC_VPITCH_PAD", 64)) / 64 * 64;
    if (kern == LDPC_KERNEL_COOP3) {
        coop3_group_layout(h, &pl.vpart, &pl.vgroup);
        pl.v_bytes = (size_t)(stride / 16) * pl.vgroup;
        pl.msg_bytes = ((size_t)(h->m + 1) * coop3_mrec(h->group_deg[0]) + 15) / 16 * 16;
        pl.et_staged = early ? coop3_et_stage_iters(rq.batch, rq.n_iter) : 0;
    } else {
        pl.v_bytes = ((size_t)h->n + 1) * pl.vpitch * esz;
        pl.msg_bytes = (kern == LDPC_KERNEL_STAIRF    ? stairf_msg_bytes(c->stairf, stride)
                        : kern == LDPC_KERNEL_GENERIC ? (size_t)h->e * stride * esz
                                                      : windowed_msg_bytes(h, stride)) +
                       4096;
    }
    if (early && (kern == LDPC_KERNEL_COOP || kern == LDPC_KERNEL_COOP3 || kern == LDPC_KERNEL_STAIRF))
        pl.early_bytes = (size_t)stride * 12;
    if (pl.et_staged) {
        pl.v2_bytes = 2 * pl.v_bytes;
        pl.et2_bytes = (size_t)stride * 20 + 256;
    }
    return pl;
}

// the buffers of every decode, then those of a staged one (a size of 0 asks for nothing)
static int ensure_unstaged(Scratch &sc, const ScratchPlan &pl)
{
    int rc = ensure(&sc.d_V, &sc.V_bytes, pl.v_bytes);
    if (rc == LDPC_OK && !pl.vgroup) rc = ensure(&sc.d_msg, &sc.msg_bytes, pl.msg_bytes);
    if (rc == LDPC_OK) rc = ensure(&sc.d_early, &sc.early_bytes, pl.early_bytes);
    return rc;
}

static int ensure_staged(Scratch &sc, const ScratchPlan &pl)
{
    const int rc = ensure(&sc.d_V2, &sc.V2_bytes, pl.v2_bytes);
    return rc != LDPC_OK ? rc : ensure(&sc.d_et2, &sc.et2_bytes, pl.et2_bytes);
}

int reserve_scratch(ldpc_ctx *c, Scratch &sc, const DecodeRequest &rq)
{
    int kern;
    int rc = select_kernel(c, rq, &kern);
    if (rc != LDPC_OK || kern == LDPC_KERNEL_AUTO || lds_resident(kern)) return rc;
    c->last_lds_lanes = c->last_lds_split = 0;
    const ScratchPlan pl = plan_scratch(c, kern, stride_of(rq.batch), rq);
    return (rc = ensure_unstaged(sc, pl)) != LDPC_OK ? rc : ensure_staged(sc, pl);
}

// ---- launch ----------------------------------------------------------------

// the request's part of a launch descriptor; plain min-sum runs as offset min-sum with offset 0
static void fill_params(DecodeLaunch &L, const DecodeRequest &rq)
{
    const ldpc_params *p = rq.p;
    const bool ms = p->algo == LDPC_ALGO_MS;
    L.batch = rq.batch;
    L.iters = rq.n_iter;
    L.is_float = rq.is_float;
    L.algo = ms ? LDPC_ALGO_OMS : p->algo;
    L.param = (p->algo == LDPC_ALGO_NMS) ? p->factor : (ms ? 0 : p->offset);
    L.beta = ms ? 0.0f : p->beta;
    L.var_min = p->var_min;
    L.msg_max = p->msg_max;
    L.early = p->early_term;
    L.iters_used = rq.d_iters;
}

// *lr = launch(), between two events on s when the context is profiling
// (ldpc_ctx_kernel_time); the pair is kept whether or not the launch succeeded
template <class Launch> static int profiled(ldpc_ctx *c, hipStream_t s, int *lr, Launch launch)
{
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    if (c->profile) {
        HIP_TRY(hipEventCreate(&ev0));
        HIP_TRY(hipEventCreate(&ev1));
        HIP_TRY(hipEventRecord(ev0, s));
    }
    *lr = launch();
    if (c->profile) {
        HIP_TRY(hipEventRecord(ev1, s));
        c->events.emplace_back(ev0, ev1);
    }
    return LDPC_OK;
}

static int count_errors(const ldpc_ctx *c, hipStream_t s, const DecodeRequest &rq)
{
    if (launch_count_errors(rq.d_hard, c->code->n, rq.batch, rq.ec->k, rq.ec->ref, rq.ec->counts, s))
        return ldpc_set_error(LDPC_EDEVICE, "count_errors: %s", hipGetErrorString(hipGetLastError()));
    return LDPC_OK;
}

static int decode_lds_resident(ldpc_ctx *c, Scratch &sc, hipStream_t s, int kern, const DecodeRequest &rq)
{
    const ldpc_code *h = c->code;
    const void *d_llr = rq.d_llr;
    const int batch = rq.batch;
    int rc, lr;
    if (rq.nm_ld) {   // node-major input (int8: family 7, ldsepi or ldsepwi): transpose it to frame-major scratch first
        if ((rc = ensure(&sc.d_msg, &sc.msg_bytes, (size_t)h->n * batch)) != LDPC_OK) return rc;
        if (launch_deinterleave_i8((const int8_t *)d_llr, nullptr, (int8_t *)sc.d_msg, h->n, batch, (int)rq.nm_ld, s))
            return ldpc_set_error(LDPC_EDEVICE, "node-major transpose: %s", hipGetErrorString(hipGetLastError()));
        d_llr = sc.d_msg;
    }
    DecodeLaunch L{};
    fill_params(L, rq);
    const bool fuse = rq.ec && kern == LDPC_KERNEL_LDSEP && rq.is_float && getenv_int("LDPC_FUSED_COUNT", 1) != 0;
    if (fuse) {   // ldsep and ldsepw count in their epilogue (one wave / one workgroup = one codeword); ldsepi
                  // and ldsepwi (int8, a pair per wave / workgroup) leave it to the separate count below
        L.cnt = rq.ec->counts;
        L.cnt_ref = rq.ec->ref;
        L.cnt_k = rq.ec->k;
    }
    rc = profiled(c, s, &lr, [&] {
        if (kern == LDPC_KERNEL_LDSEP && c->last_ep_waves && !rq.is_float)
            return launch_ldsepwi(c->lds, h, (const int8_t *)d_llr, rq.d_hard, (int8_t *)rq.d_soft, c->last_ep_waves, L,
                                  s);
        if (kern == LDPC_KERNEL_LDSEP && c->last_ep_waves)
            return launch_ldsepw(c->lds, h, (const float *)d_llr, rq.d_hard, (float *)rq.d_soft, batch, rq.n_iter,
                                 c->last_ep_waves, L, s);
        if (kern == LDPC_KERNEL_LDSEP && !rq.is_float)
            return launch_ldsepi(c->lds, h, (const int8_t *)d_llr, rq.d_hard, (int8_t *)rq.d_soft, L, s);
        if (kern == LDPC_KERNEL_LDSEP)
            return launch_ldsep(c->lds, h, (const float *)d_llr, rq.d_hard, (float *)rq.d_soft, batch, rq.n_iter, L, s);
        if (L.algo == LDPC_ALGO_BP)
            return launch_bp_lds(c->lds, h, (const float *)d_llr, rq.d_hard, (float *)rq.d_soft, L, s,
                                 &c->last_lds_lanes);
        return launch_lds(c->lds, h, d_llr, rq.d_hard, rq.d_soft, batch, rq.n_iter, L, s, &c->last_lds_lanes,
                          &c->last_lds_split);
    });
    if (rc != LDPC_OK) return rc;
    if (lr) return ldpc_set_error(LDPC_EDEVICE, "lds decode launch: %s", hipGetErrorString(hipGetLastError()));
    return rq.ec && !fuse ? count_errors(c, s, rq) : LDPC_OK;
}

// queue the start state of a decode in scratch: messages zero, V = the input LLRs
static int load_state(Scratch &sc, hipStream_t s, const ScratchPlan &pl, int n, int stride, const DecodeRequest &rq)
{
    const bool grouped = pl.vgroup != 0;
    const int batch = rq.batch;
    // messages start at 0 (CDecoder_OMS_fixed_SSE.cpp:129-131); the all-zero
    // compressed word is the all-zero message set as well.
    if (grouped) {
        if (launch_zero_rows((char *)sc.d_V + pl.vpart, pl.vgroup, pl.msg_bytes, stride / 16, s))
            return ldpc_set_error(LDPC_EDEVICE, "message zeroing: %s", hipGetErrorString(hipGetLastError()));
    } else {
        const size_t msg_zero = pl.msg_bytes;
        HIP_TRY(hipMemsetAsync(sc.d_msg, 0, msg_zero, s));
    }
    if (rq.nm_ld) {   // node-major input: 16-codeword pieces copied straight into V (no transpose)
        if (launch_nm_pieces_i8((const int8_t *)rq.d_llr, rq.nm_ld, n, batch, pl.vpitch, (int8_t *)sc.d_V,
                                grouped ? pl.vgroup : 16, grouped ? 16 : (size_t)pl.vpitch, s))
            return ldpc_set_error(LDPC_EDEVICE, "node-major load: %s", hipGetErrorString(hipGetLastError()));
    } else if (rq.is_float ? launch_interleave_f32((const float *)rq.d_llr, (float *)sc.d_V, n, batch, pl.vpitch, s)
               : grouped   ? launch_interleave_grp_i8((const int8_t *)rq.d_llr, (int8_t *)sc.d_V, n, batch, stride,
                                                      pl.vgroup, s)
                           : launch_interleave_i8((const int8_t *)rq.d_llr, (int8_t *)sc.d_V, n, batch, pl.vpitch, s))
        return ldpc_set_error(LDPC_EDEVICE, "interleave: %s", hipGetErrorString(hipGetLastError()));
    return LDPC_OK;
}

// queue V -> the caller's frame-major hard / soft outputs
static int store_outputs(const Scratch &sc, hipStream_t s, const ScratchPlan &pl, int n, const DecodeRequest &rq)
{
    uint8_t *const hard = rq.d_hard;
    void *const soft = rq.d_soft;
    const int batch = rq.batch;
    if (!hard && !soft) return LDPC_OK;
    if (rq.is_float ? launch_deinterleave_f32((const float *)sc.d_V, hard, (float *)soft, n, batch, pl.vpitch, s)
        : pl.vgroup ? launch_deinterleave_grp_i8((const int8_t *)sc.d_V, hard, (int8_t *)soft, n, batch, pl.vgroup, s)
                    : launch_deinterleave_i8((const int8_t *)sc.d_V, hard, (int8_t *)soft, n, batch, pl.vpitch, s))
        return ldpc_set_error(LDPC_EDEVICE, "deinterleave: %s", hipGetErrorString(hipGetLastError()));
    return LDPC_OK;
}

// size the scratch, load it, decode, write the outputs, count
static int decode_in_scratch(ldpc_ctx *c, Scratch &sc, hipStream_t s, int kern, const DecodeRequest &rq)
{
    const ldpc_code *h = c->code;
    const int stride = stride_of(rq.batch);
    const ScratchPlan pl = plan_scratch(c, kern, stride, rq);
    int rc, lr;
    if ((rc = ensure_unstaged(sc, pl)) != LDPC_OK) return rc;
    c->last_et_stage = pl.et_staged;
    if ((rc = ensure_staged(sc, pl)) != LDPC_OK || (rc = load_state(sc, s, pl, h->n, stride, rq)) != LDPC_OK) return rc;
    DecodeLaunch L{};
    fill_params(L, rq);
    L.V = sc.d_V;
    L.msg = pl.vgroup ? (void *)((char *)sc.d_V + pl.vpart) : sc.d_msg;
    L.vgroup = pl.vgroup;
    L.stride = stride;
    L.vpitch = pl.vpitch;
    L.d_edge_var = c->d_edge_var;
    L.d_group_deg = c->d_group_deg;
    L.d_group_cnt = c->d_group_cnt;
    L.n_groups = h->n_groups;
    L.n = h->n;
    L.m = h->m;
    L.e = h->e;
    L.lds_pad = c->lds_pad;
    L.V2 = pl.et_staged ? sc.d_V2 : nullptr;
    L.et2 = pl.et_staged ? (int32_t *)sc.d_et2 : nullptr;
    if (pl.early_bytes) {   // (iterations used land in the scratch when the caller passed no array)
        L.bad = (uint32_t *)sc.d_early;
        if (!L.iters_used) L.iters_used = (int32_t *)((char *)sc.d_early + (size_t)stride * 4);
        L.live = (uint8_t *)sc.d_early + (size_t)stride * 8;
    }
    rc = profiled(c, s, &lr, [&] {
        switch (kern) {
        case LDPC_KERNEL_COOP3: return launch_coop3(L, c->coop3, s);
        case LDPC_KERNEL_COOP: return launch_coop(L, c->coop, s);
        case LDPC_KERNEL_STAIRF:
            return L.algo == LDPC_ALGO_BP ? launch_stairbp(L, c->stairf, s) : launch_stairf(L, c->stairf, s);
        case LDPC_KERNEL_WINDOWED2: return launch_windowed2(L, c->w16, s);
        case LDPC_KERNEL_WINDOWED: return launch_windowed(L, c->wcode, s);
        default: return L.algo == LDPC_ALGO_BP ? launch_bp_generic(L, s) : launch_generic(L, s);
        }
    });
    if (rc != LDPC_OK) return rc;
    if (lr) {
        const hipError_t e = hipGetLastError();
        const char *why = e != hipSuccess ? hipGetErrorString(e) : "launch configuration rejected by the host side";
        return ldpc_set_error(LDPC_EDEVICE, "decode launch (kernel %d): %s", kern, why);
    }
    if ((rc = store_outputs(sc, s, pl, h->n, rq)) != LDPC_OK) return rc;
    return rq.ec ? count_errors(c, s, rq) : LDPC_OK;
}

int decode_device(ldpc_ctx *c, Scratch &sc, hipStream_t s, const DecodeRequest &rq)
{
    int kern;
    const int rc = select_kernel(c, rq, &kern);
    if (rc != LDPC_OK || kern == LDPC_KERNEL_AUTO) return rc;
    c->last_lds_lanes = c->last_lds_split = 0;
    return lds_resident(kern) ? decode_lds_resident(c, sc, s, kern, rq) : decode_in_scratch(c, sc, s, kern, rq);
}
