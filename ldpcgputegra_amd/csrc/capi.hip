// capi.hip -- the C-ABI decoder context (ctx.h): its lifecycle and getters,
// the decode entry points over dispatch.hip's decode_device, the host-buffer
// pipeline and the non-decode entry points.  Host code only.
//
// A context mirrors the reference decoder objects: it owns the device scratch
// (V and messages, allocated up front for max_batch codewords, as
// CDecoder_fixed_SSE's constructor does, code/x86/CDecoder/template/
// CDecoder_fixed_SSE.cpp:23-27, and CGPUDecoder(nb_frames, n, k, m),
// code/gpu_fixed/decoder_template/CGPUDecoder.cpp:14-38) plus its own HIP
// stream -- created once, not per call as the reference's decode_stream does
// (code/gpu_fixed/decoder_ms/CGPU_Decoder_MS_SIMD.cu:223-224).
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>

#include "ctx.h"
#include "host.h"

int ensure(void **p, size_t *have, size_t need)
{
    if (*have >= need) return LDPC_OK;
    if (*p) (void)hipFree(*p);
    *p = nullptr;
    *have = 0;
    hipError_t e = hipMalloc(p, need);
    if (e != hipSuccess) {
        *p = nullptr;
        return ldpc_set_error(LDPC_ENOMEM, "hipMalloc(%zu): %s", need, hipGetErrorString(e));
    }
    *have = need;
    return LDPC_OK;
}

extern "C" int ldpc_device_count(int *count)
{
    if (!count) return ldpc_set_error(LDPC_EINVAL, "count is NULL");
    int c = 0;
    hipError_t e = hipGetDeviceCount(&c);
    *count = (e == hipSuccess) ? c : 0;
    return LDPC_OK;
}

// device = -1: a host context (host.cpp) -- host-buffer decodes on the CPU,
// no HIP call at all; the device-pointer entry points reject it
int host_only(const ldpc_ctx *c)
{
    return ldpc_set_error(LDPC_EUNSUPPORTED, "context %p is a host context (device -1): device buffers need a GPU "
                          "context", (const void *)c);
}

extern "C" int ldpc_ctx_create(const ldpc_code *h, int device, int max_batch, ldpc_ctx **out)
{
    if (!out) return ldpc_set_error(LDPC_EINVAL, "out is NULL");
    *out = nullptr;
    if (!h || max_batch <= 0) return ldpc_set_error(LDPC_EINVAL, "NULL code or max_batch <= 0");
    if (h->max_deg > 32) return ldpc_set_error(LDPC_EUNSUPPORTED, "check degree %d > 32", h->max_deg);
    if (device != -1) {
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
            return ldpc_set_error(LDPC_EDEVICE, "no HIP device visible");
        if (device < 0 || device >= ndev) return ldpc_set_error(LDPC_EINVAL, "device %d of %d", device, ndev);
        HIP_TRY(hipSetDevice(device));
    }
    auto *c = new ldpc_ctx();
    c->code = h;
    c->device = device;
    c->max_batch = max_batch;
    c->max_stride = (max_batch + 63) / 64 * 64;
    if (device == -1) {   // a host context holds nothing else
        *out = c;
        return LDPC_OK;
    }
    int rc = LDPC_OK;
    auto fail = [&](int r) {
        ldpc_ctx_destroy(c);
        return r;
    };
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess)
        return fail(ldpc_set_error(LDPC_EDEVICE, "hipStreamCreate"));
    if (hipMalloc(&c->d_edge_var, 4ull * h->e) != hipSuccess ||
        hipMalloc(&c->d_group_deg, sizeof(int) * h->n_groups) != hipSuccess ||
        hipMalloc(&c->d_group_cnt, sizeof(int) * h->n_groups) != hipSuccess)
        return fail(ldpc_set_error(LDPC_ENOMEM, "code tables"));
    if (hipMemcpy(c->d_edge_var, h->edge_var.data(), 4ull * h->e, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(c->d_group_deg, h->group_deg.data(), sizeof(int) * h->n_groups, hipMemcpyHostToDevice) !=
            hipSuccess ||
        hipMemcpy(c->d_group_cnt, h->group_cnt.data(), sizeof(int) * h->n_groups, hipMemcpyHostToDevice) !=
            hipSuccess)
        return fail(ldpc_set_error(LDPC_EDEVICE, "code table upload"));
    if ((rc = windowed_code_upload(h, &c->wcode)) != LDPC_OK) return fail(rc);
    if ((rc = windowed2_upload(h, 16, 2, &c->w16)) != LDPC_OK) return fail(rc);
    if ((rc = coop_upload(h, &c->coop)) != LDPC_OK) return fail(rc);
    if ((rc = coop3_upload(h, &c->coop3)) != LDPC_OK) return fail(rc);
    if ((rc = lds_upload(h, &c->lds)) != LDPC_OK) return fail(rc);
    if ((rc = stairf_upload(h, &c->stairf)) != LDPC_OK) return fail(rc);
    if ((rc = encode_upload(h, &c->enc)) != LDPC_OK) return fail(rc);
    *out = c;
    return LDPC_OK;
}

extern "C" void ldpc_ctx_destroy(ldpc_ctx *c)
{
    if (!c) return;
    if (c->device < 0) {
        delete c;
        return;
    }
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->host_pending) (void)hipEventSynchronize(c->host_done);
    if (c->host_done) (void)hipEventDestroy(c->host_done);
    windowed_code_free(&c->wcode);
    windowed2_free(&c->w16);
    coop_free(&c->coop);
    coop_free(&c->coop3);
    lds_free(&c->lds);
    stairf_free(&c->stairf);
    encode_free(&c->enc);
    genc_free(&c->genc);
    for (auto &pr : c->events) {
        (void)hipEventDestroy(pr.first);
        (void)hipEventDestroy(pr.second);
    }
    (void)hipFree(c->d_edge_var);
    (void)hipFree(c->d_group_deg);
    (void)hipFree(c->d_group_cnt);
    c->sc.release();
    (void)hipFree(c->d_io);
    for (Lane &l : c->lanes) {
        if (l.stream) (void)hipStreamSynchronize(l.stream);
        l.sc.release();
        (void)hipFree(l.d_io);
        if (l.h2d_done) (void)hipEventDestroy(l.h2d_done);
        if (l.stream) (void)hipStreamDestroy(l.stream);
    }
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

extern "C" int ldpc_ctx_stream(ldpc_ctx *c, void **s)
{
    if (!c || !s) return ldpc_set_error(LDPC_EINVAL, "NULL ctx/stream");
    *s = (void *)c->stream;
    return LDPC_OK;
}

extern "C" int ldpc_ctx_set_kernel(ldpc_ctx *c, int k)
{
    if (!c || k < LDPC_KERNEL_AUTO || k > LDPC_KERNEL_STAIRF || k == LDPC_KERNEL_HOST)
        return ldpc_set_error(LDPC_EINVAL, "kernel must be 0 (auto) .. 9 or 11");
    // family 9 also takes the tables of its several-wave kernel once ldpc_ctx_set_ep_wide is on
    // or, for the int8 decode, ldpc_ctx_set_i8_ep_wide
    const bool wide = k == LDPC_KERNEL_LDSEP && c->device >= 0 && (c->ep_wide || c->i8_ep_wide) && c->lds.epw_valid;
    if (!ldpc_ctx_has_kernel(c, k) && !wide)
        return ldpc_set_error(LDPC_EUNSUPPORTED, "kernel %d cannot schedule this code", k);
    c->kernel = k;
    return LDPC_OK;
}

extern "C" int ldpc_ctx_set_bp_staircase(ldpc_ctx *c, int enable)
{
    if (!c) return ldpc_set_error(LDPC_EINVAL, "NULL ctx");
    if (c->device < 0 || !c->stairf.valid)
        return ldpc_set_error(LDPC_EUNSUPPORTED, "belief propagation on the staircase kernel: %s",
                              c->device < 0 ? "host context" : "the code has no staircase table");
    c->bp_staircase = enable != 0;
    return LDPC_OK;
}

extern "C" int ldpc_ctx_get_bp_staircase(ldpc_ctx *c, int *enable)
{
    if (!c || !enable) return ldpc_set_error(LDPC_EINVAL, "NULL");
    *enable = c->bp_staircase ? 1 : 0;
    return LDPC_OK;
}

extern "C" int ldpc_ctx_set_f16_all_codes(ldpc_ctx *c, int enable)
{
    if (!c) return ldpc_set_error(LDPC_EINVAL, "NULL ctx");
    c->f16_all_codes = enable != 0;   // (a host context decodes every code either way)
    return LDPC_OK;
}

extern "C" int ldpc_ctx_get_f16_all_codes(ldpc_ctx *c, int *enable)
{
    if (!c || !enable) return ldpc_set_error(LDPC_EINVAL, "NULL");
    *enable = c->f16_all_codes ? 1 : 0;
    return LDPC_OK;
}

extern "C" int ldpc_ctx_set_f16_edge_parallel(ldpc_ctx *c, int enable)
{
    if (!c) return ldpc_set_error(LDPC_EINVAL, "NULL ctx");
    if (c->device < 0 || !ldpc_ctx_has_kernel(c, LDPC_KERNEL_LDSEP))
        return ldpc_set_error(LDPC_EUNSUPPORTED, "the edge-parallel binary16 kernel: %s",
                              c->device < 0 ? "host context" : "the code is not in the shape of kernel family 9");
    c->f16_edge_parallel = enable != 0;
    return LDPC_OK;
}

extern "C" int ldpc_ctx_get_f16_edge_parallel(ldpc_ctx *c, int *enable)
{
    if (!c || !enable) return ldpc_set_error(LDPC_EINVAL, "NULL");
    *enable = c->f16_edge_parallel ? 1 : 0;
    return LDPC_OK;
}

extern "C" int ldpc_ctx_set_i8_edge_parallel(ldpc_ctx *c, int enable)
{
    if (!c) return ldpc_set_error(LDPC_EINVAL, "NULL ctx");
    if (c->device < 0 || !ldpc_ctx_has_kernel(c, LDPC_KERNEL_LDSEP))
        return ldpc_set_error(LDPC_EUNSUPPORTED, "the edge-parallel int8 kernel: %s",
                              c->device < 0 ? "host context" : "the code is not in the shape of kernel family 9");
    c->i8_edge_parallel = enable != 0;
    return LDPC_OK;
}

extern "C" int ldpc_ctx_get_i8_edge_parallel(ldpc_ctx *c, int *enable)
{
    if (!c || !enable) return ldpc_set_error(LDPC_EINVAL, "NULL");
    *enable = c->i8_edge_parallel ? 1 : 0;
    return LDPC_OK;
}

extern "C" int ldpc_ctx_set_i8_ep_wide(ldpc_ctx *c, int enable)
{
    if (!c) return ldpc_set_error(LDPC_EINVAL, "NULL ctx");
    if (c->device < 0 || !ldsepwi_applicable(c->code, c->lds))
        return ldpc_set_error(LDPC_EUNSUPPORTED, "the edge-parallel int8 kernel over several waves: %s",
                              c->device < 0 ? "host context" : "the code has no several-wave plan of kernel family 9");
    c->i8_ep_wide = enable != 0;
    return LDPC_OK;
}

extern "C" int ldpc_ctx_get_i8_ep_wide(ldpc_ctx *c, int *enable)
{
    if (!c || !enable) return ldpc_set_error(LDPC_EINVAL, "NULL");
    *enable = c->i8_ep_wide ? 1 : 0;
    return LDPC_OK;
}

extern "C" int ldpc_ctx_set_ep_wide(ldpc_ctx *c, int enable)
{
    if (!c) return ldpc_set_error(LDPC_EINVAL, "NULL ctx");
    if (c->device < 0)
        return ldpc_set_error(LDPC_EUNSUPPORTED, "the edge-parallel float kernel over several waves: host context");
    c->ep_wide = enable != 0;
    return LDPC_OK;
}

extern "C" int ldpc_ctx_get_ep_wide(ldpc_ctx *c, int *enable)
{
    if (!c || !enable) return ldpc_set_error(LDPC_EINVAL, "NULL");
    *enable = c->ep_wide ? 1 : 0;
    return LDPC_OK;
}

extern "C" int ldpc_ctx_last_ep_waves(ldpc_ctx *c, int *w)
{
    if (!c || !w) return ldpc_set_error(LDPC_EINVAL, "NULL");
    *w = c->last_ep_waves;
    return LDPC_OK;
}

extern "C" int ldpc_ctx_profile(ldpc_ctx *c, int enable)
{
    if (!c) return ldpc_set_error(LDPC_EINVAL, "NULL ctx");
    c->profile = enable != 0;
    return LDPC_OK;
}

extern "C" int ldpc_ctx_kernel_time(ldpc_ctx *c, double *total_ms, int *launches, int reset)
{
    if (!c) return ldpc_set_error(LDPC_EINVAL, "NULL ctx");
    if (c->device < 0) {   // host context: no kernels
        if (total_ms) *total_ms = 0.0;
        if (launches) *launches = 0;
        return LDPC_OK;
    }
    HIP_TRY(hipSetDevice(c->device));
    double tot = 0.0;
    for (auto &pr : c->events) {
        HIP_TRY(hipEventSynchronize(pr.second));
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, pr.first, pr.second));
        tot += ms;
    }
    if (total_ms) *total_ms = tot;
    if (launches) *launches = (int)c->events.size();
    if (reset) {
        for (auto &pr : c->events) {
            (void)hipEventDestroy(pr.first);
            (void)hipEventDestroy(pr.second);
        }
        c->events.clear();
    }
    return LDPC_OK;
}

// library-internal (mixed.hip): windowed2 workgroups of this context request
// `bytes` of dynamic LDS they do not use, so that none fits beside a coop3
// workgroup (124.5 KB of the CU's 160 KB): a mixed batch's windowed2 waves
// then stay off the CUs running the coop3 decode, whose slab waves are
// VALU-bound and would lose issue slots to them
int ldpc_ctx_set_lds_pad(ldpc_ctx *c, int bytes)
{
    if (!c || bytes < 0 || bytes > 65536) return ldpc_set_error(LDPC_EINVAL, "lds pad");
    c->lds_pad = bytes;
    return LDPC_OK;
}

extern "C" int ldpc_ctx_last_kernel(ldpc_ctx *c, int *k)
{
    if (!c || !k) return ldpc_set_error(LDPC_EINVAL, "NULL");
    *k = c->last_kernel;
    return LDPC_OK;
}

extern "C" int ldpc_ctx_last_skipped(ldpc_ctx *c, int *k)
{
    if (!c || !k) return ldpc_set_error(LDPC_EINVAL, "NULL");
    *k = c->last_skipped;
    return LDPC_OK;
}

extern "C" int ldpc_ctx_last_et_stage(ldpc_ctx *c, int *k)
{
    if (!c || !k) return ldpc_set_error(LDPC_EINVAL, "NULL");
    *k = c->last_et_stage;
    return LDPC_OK;
}

extern "C" int ldpc_ctx_last_lds_shape(ldpc_ctx *c, int *lanes_per_codeword, int *split)
{
    if (!c || !lanes_per_codeword || !split) return ldpc_set_error(LDPC_EINVAL, "NULL");
    *lanes_per_codeword = c->last_lds_lanes;
    *split = c->last_lds_split;
    return LDPC_OK;
}

extern "C" int ldpc_ctx_get_kernel(ldpc_ctx *c, int *k)
{
    if (!c || !k) return ldpc_set_error(LDPC_EINVAL, "NULL");
    *k = c->kernel;
    return LDPC_OK;
}

extern "C" int ldpc_decode_i8_async(ldpc_ctx *c, void *s, const int8_t *d_llr, uint8_t *d_hard, int8_t *d_soft,
                                    int32_t *d_iters, int batch, int n_iter, const ldpc_params *p)
{
    if (!c || (!d_llr && batch > 0)) return ldpc_set_error(LDPC_EINVAL, "NULL ctx/llr");
    return decode_device(c, c->sc, (hipStream_t)s, {d_llr, d_hard, d_soft, d_iters, batch, n_iter, p, false});
}

// Node-major input: LLR of bit i of codeword b at d_llr[i * ld + b] -- the
// layout the reference's decoders run on (Interleaver_uint8's output,
// code/gpu_fixed/transpose/GPU_Transpose_uint8.cu:80-130), which its v2 decoder
// takes straight from the caller (CGPU_Decoder_MS_SIMD_v2::decode,
// code/gpu_fixed/decoder_oms_v2/CGPU_Decoder_MS_SIMD_v2.cu:120-251: copy,
// decode, InvInterleaver_uint8 with the hard decision).  Outputs frame-major,
// as there.
extern "C" int ldpc_decode_i8_nm_async(ldpc_ctx *c, void *s, const int8_t *d_llr, size_t ld, uint8_t *d_hard,
                                       int8_t *d_soft, int32_t *d_iters, int batch, int n_iter, const ldpc_params *p)
{
    if (!c || (!d_llr && batch > 0)) return ldpc_set_error(LDPC_EINVAL, "NULL ctx/llr");
    if (batch > 0 && ld < (size_t)batch)
        return ldpc_set_error(LDPC_EINVAL, "node-major pitch %zu < batch %d", ld, batch);
    return decode_device(c, c->sc, (hipStream_t)s,
                         {d_llr, d_hard, d_soft, d_iters, batch, n_iter, p, false, batch > 0 ? ld : 0, nullptr});
}

extern "C" int ldpc_decode_f32_async(ldpc_ctx *c, void *s, const float *d_llr, uint8_t *d_hard, float *d_soft,
                                     int32_t *d_iters, int batch, int n_iter, const ldpc_params *p)
{
    if (!c || (!d_llr && batch > 0)) return ldpc_set_error(LDPC_EINVAL, "NULL ctx/llr");
    return decode_device(c, c->sc, (hipStream_t)s, {d_llr, d_hard, d_soft, d_iters, batch, n_iter, p, true});
}

// decode + error count in one call (the reference's decode followed by
// CErrorAnalyzer::generate, code/x86/CErrorAnalyzer/CErrorAnalyzer.cpp:123-154;
// code/x86/main_p.cpp:511-540): fused into the decode kernel's epilogue where
// the kernel writes the hard decisions itself (ldsep), else one count launch
// after the decode (it needs d_hard then)
static int decode_count(ldpc_ctx *c, void *s, const void *d_llr, uint8_t *d_hard, void *d_soft, int32_t *d_iters,
                        int batch, int n_iter, const ldpc_params *p, bool is_float, int k, const uint8_t *d_ref,
                        unsigned long long *d_counts)
{
    if (!c || (!d_llr && batch > 0)) return ldpc_set_error(LDPC_EINVAL, "NULL ctx/llr");
    if (!d_counts || k < 0 || k > c->code->n) return ldpc_set_error(LDPC_EINVAL, "count: NULL counts or k %d", k);
    if (!d_hard) return ldpc_set_error(LDPC_EINVAL, "count: d_hard is required");
    const ErrCount ec{k, d_ref, d_counts};
    return decode_device(c, c->sc, (hipStream_t)s,
                         {d_llr, d_hard, d_soft, d_iters, batch, n_iter, p, is_float, 0, &ec});
}

extern "C" int ldpc_decode_i8_count_async(ldpc_ctx *c, void *s, const int8_t *d_llr, uint8_t *d_hard, int8_t *d_soft,
                                          int32_t *d_iters, int batch, int n_iter, const ldpc_params *p, int k,
                                          const uint8_t *d_ref, unsigned long long *d_counts)
{
    return decode_count(c, s, d_llr, d_hard, d_soft, d_iters, batch, n_iter, p, false, k, d_ref, d_counts);
}

extern "C" int ldpc_decode_f32_count_async(ldpc_ctx *c, void *s, const float *d_llr, uint8_t *d_hard, float *d_soft,
                                           int32_t *d_iters, int batch, int n_iter, const ldpc_params *p, int k,
                                           const uint8_t *d_ref, unsigned long long *d_counts)
{
    return decode_count(c, s, d_llr, d_hard, d_soft, d_iters, batch, n_iter, p, true, k, d_ref, d_counts);
}

// Chunks of the host-buffer path: whole 64-codeword rows, at least 256
// codewords each (16 coop workgroups), LDPC_HOST_CHUNKS of them (default 2
// when the input is large enough for its copy time to matter, >= 64 MB, else
// 1), and no more than the hardware queues left for them.  Concurrent chunk
// decodes need hardware queues of their own: HIP maps streams round-robin onto
// GPU_MAX_HW_QUEUES (default 4) queues per process, and the null stream and
// the context's stream hold two of them, so a third lane would share a queue
// -- and wait for -- the first one's decode (measured: 4 lanes on 2 queues,
// 114 ms per DVB-S2 4096-codeword call vs 68 ms unchunked).
static int host_chunks(int batch, size_t in_bytes)
{
    const int def = in_bytes >= ((size_t)64 << 20) ? 2 : 1;
    const int lanes = std::max(1, getenv_int("GPU_MAX_HW_QUEUES", 4) - 2);
    const int want = std::min(lanes, std::max(1, getenv_int("LDPC_HOST_CHUNKS", def)));
    return std::max(1, std::min(want, batch / 256));
}

// The host-buffer path (CDecoder::decode(char*, char*, int), synchronous).
// The batch is cut into chunks; chunk i runs on lane i (own stream, scratch
// and staging): H2D(i) -> decode(i) -> D2H(i), so the copies of one chunk
// overlap the decodes of the others -- the reference's W streams x F frames
// scheme (paper/ldpcGpuTegra.tex:279-289; its decode_stream,
// code/gpu_fixed/decoder_ms/CGPU_Decoder_MS_SIMD.cu:219-275, runs one stream
// with blocking copies).  A staircase-code decode takes about as long for one
// 16-codeword workgroup as for a whole chip of them (its serial chain is per
// workgroup), so the concurrent chunk decodes cost nothing.  The input copies
// are chained (lane i's waits for lane i-1's): two concurrent copies share
// the link and both finish at the end (measured r03e, pinned, 2 chunks: 4.7
// ms each, side by side), which held every decode back until all the input
// had arrived.  A call therefore takes about H2D(batch) + one decode +
// D2H(one chunk) -- no chunking can do better, since the last chunk cannot
// start before all the input is on the device.  Every lane's
// scratch is sized before any work is queued.  Pinned host buffers
// (ldpc_host_alloc) make the copies asynchronous DMA; pageable ones are
// staged by the HIP runtime (the host thread blocks in the copy, the GPU
// keeps decoding).
static int decode_host(ldpc_ctx *c, const void *llr, uint8_t *hard, int batch, int n_iter, const ldpc_params *p,
                       bool is_float)
{
    if (!c || ((!llr || !hard) && batch > 0)) return ldpc_set_error(LDPC_EINVAL, "NULL ctx/llr/hard");
    int rc = check_params(c, batch, n_iter, p, is_float);
    if (rc != LDPC_OK || batch == 0) return rc;
    if (c->device < 0) {   // host context: the CPU decoder (host.cpp)
        c->last_kernel = LDPC_KERNEL_HOST;
        return is_float ? host_decode_f32(c->code, (const float *)llr, hard, nullptr, nullptr, batch, n_iter, p)
                        : host_decode_i8(c->code, (const int8_t *)llr, hard, batch, n_iter, p);
    }
    HIP_TRY(hipSetDevice(c->device));
    const size_t esz = is_float ? 4 : 1;
    const int n = c->code->n, nc_want = host_chunks(batch, (size_t)batch * n * esz);
    // chunk boundaries: equal chunks in units of 1024 codewords where the
    // batch allows (64 coop workgroups: the XCD-aware workgroup remap keeps
    // the 8 workgroups that share a V line on one XCD only when a grid splits
    // evenly into 8 x 8 of them; a chunk with the groups split across XCDs
    // runs ~20 % slower, measured r03h with a 2:1 split of 4096 codewords:
    // 60.2 vs 55.7 ms per call), else 128 (the remap's grid % 8).  The 1024
    // unit is used only while the chunks stay even (the last one at least half
    // of the others): 2049 codewords as 2048 + 1 would leave the big chunk's
    // decode and copy with nothing to overlap
    std::vector<int> b0s(1, 0);
    {
        auto size_for = [&](int unit) { return ((batch + nc_want - 1) / nc_want + unit - 1) / unit * unit; };
        auto even = [&](int cs) {
            const int full = std::min(nc_want, (batch + cs - 1) / cs);
            return full <= 1 || 2 * (batch - (full - 1) * cs) >= cs;
        };
        int cs0 = size_for(128);
        if (batch >= nc_want * 1024 && even(size_for(1024))) cs0 = size_for(1024);
        for (int i = 1; i < nc_want && i * cs0 < batch; i++) b0s.push_back(i * cs0);
        b0s.push_back(batch);
    }
    const int nc = (int)b0s.size() - 1;   // (rounding up can leave fewer chunks)
    int cs = 0;   // largest chunk (the staging size of every lane)
    for (int i = 0; i < nc; i++) cs = std::max(cs, b0s[i + 1] - b0s[i]);
    if ((int)c->lanes.size() < nc) c->lanes.resize(nc);
    auto in_al = [&](int nb) { return ((size_t)nb * n * esz + 255) / 256 * 256; };
    // streams, events and every lane's buffers first (no hipFree between queued work)
    for (int i = 0; i < nc; i++) {
        Lane &l = c->lanes[i];
        const int b0 = b0s[i], nb = b0s[i + 1] - b0;
        if (!l.stream && hipStreamCreateWithFlags(&l.stream, hipStreamNonBlocking) != hipSuccess) {
            l.stream = nullptr;
            return ldpc_set_error(LDPC_EDEVICE, "host path: hipStreamCreate");
        }
        if (!l.h2d_done && hipEventCreateWithFlags(&l.h2d_done, hipEventDisableTiming) != hipSuccess) {
            l.h2d_done = nullptr;
            return ldpc_set_error(LDPC_EDEVICE, "host path: hipEventCreate");
        }
        if ((rc = ensure(&l.d_io, &l.io_bytes, in_al(nb) + (size_t)cs * n)) != LDPC_OK) return rc;
        if ((rc = reserve_scratch(c, l.sc, {l.d_io, nullptr, nullptr, nullptr, nb, n_iter, p, is_float})) != LDPC_OK)
            return rc;
    }
    int used = 0;
    // every queued lane is joined before returning, on success and on error
    auto finish = [&](int r) {
        for (int i = 0; i < used; i++) {
            const hipError_t e = hipStreamSynchronize(c->lanes[i].stream);
            if (e != hipSuccess && r == LDPC_OK) r = ldpc_set_error(LDPC_EDEVICE, "host path: %s", hipGetErrorString(e));
        }
        return r;
    };
    for (int i = 0; i < nc; i++) {
        Lane &l = c->lanes[i];
        const int b0 = b0s[i], nb = b0s[i + 1] - b0;
        char *d_in = (char *)l.d_io, *d_out = d_in + in_al(nb);
        used = i + 1;
        if (i > 0 && hipStreamWaitEvent(l.stream, c->lanes[i - 1].h2d_done, 0) != hipSuccess)
            return finish(ldpc_set_error(LDPC_EDEVICE, "host path: hipStreamWaitEvent"));
        if (hipMemcpyAsync(d_in, (const char *)llr + (size_t)b0 * n * esz, (size_t)nb * n * esz,
                           hipMemcpyHostToDevice, l.stream) != hipSuccess ||
            hipEventRecord(l.h2d_done, l.stream) != hipSuccess)
            return finish(ldpc_set_error(LDPC_EDEVICE, "host path H2D: %s", hipGetErrorString(hipGetLastError())));
        rc = decode_device(c, l.sc, l.stream, {d_in, (uint8_t *)d_out, nullptr, nullptr, nb, n_iter, p, is_float});
        if (rc != LDPC_OK) return finish(rc);
    }
    for (int i = 0; i < nc; i++) {
        Lane &l = c->lanes[i];
        const int b0 = b0s[i], nb = b0s[i + 1] - b0;
        if (hipMemcpyAsync(hard + (size_t)b0 * n, (char *)l.d_io + in_al(nb), (size_t)nb * n, hipMemcpyDeviceToHost,
                           l.stream) != hipSuccess)
            return finish(ldpc_set_error(LDPC_EDEVICE, "host path D2H: %s", hipGetErrorString(hipGetLastError())));
    }
    return finish(LDPC_OK);
}

// The asynchronous host-buffer path: one batch, H2D -> decode -> D2H queued on
// the caller's stream through the context's own staging (c->d_io) and scratch
// (c->sc), nothing waited for.  Two contexts on two streams keep two batches in
// flight: the copies of one overlap the decode of the other (the reference's
// W streams x F frames, paper/ldpcGpuTegra.tex:279-289).
static int decode_host_async(ldpc_ctx *c, void *sv, const void *llr, uint8_t *hard, int batch, int n_iter,
                             const ldpc_params *p, bool is_float)
{
    if (!c || ((!llr || !hard) && batch > 0)) return ldpc_set_error(LDPC_EINVAL, "NULL ctx/llr/hard");
    int rc = check_params(c, batch, n_iter, p, is_float);
    if (rc != LDPC_OK || batch == 0) return rc;
    if (c->device < 0) return host_only(c);
    HIP_TRY(hipSetDevice(c->device));
    const hipStream_t s = (hipStream_t)sv;
    const size_t n = (size_t)c->code->n, esz = is_float ? 4 : 1;
    const size_t in_al = ((size_t)batch * n * esz + 255) / 256 * 256;
    // size the staging and the scratch before anything is queued (a hipFree of
    // a buffer the previous call still uses would wait for the device anyway)
    if (!c->host_done) HIP_TRY(hipEventCreateWithFlags(&c->host_done, hipEventDisableTiming));
    // a previous call (possibly on another stream) still using d_io / the scratch:
    // resizing frees them, so wait for it on the host; otherwise order this
    // stream after it on the device
    const bool grow = c->io_bytes < in_al + (size_t)batch * n;
    if (c->host_pending && grow) HIP_TRY(hipEventSynchronize(c->host_done));
    if ((rc = ensure(&c->d_io, &c->io_bytes, in_al + (size_t)batch * n)) != LDPC_OK) return rc;
    DecodeRequest rq{c->d_io, nullptr, nullptr, nullptr, batch, n_iter, p, is_float};
    if ((rc = reserve_scratch(c, c->sc, rq)) != LDPC_OK) return rc;
    if (c->host_pending) HIP_TRY(hipStreamWaitEvent(s, c->host_done, 0));
    char *d_in = (char *)c->d_io, *d_out = d_in + in_al;
    HIP_TRY(hipMemcpyAsync(d_in, llr, (size_t)batch * n * esz, hipMemcpyHostToDevice, s));
    rq.d_hard = (uint8_t *)d_out;
    if ((rc = decode_device(c, c->sc, s, rq)) != LDPC_OK) return rc;
    HIP_TRY(hipMemcpyAsync(hard, d_out, (size_t)batch * n, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipEventRecord(c->host_done, s));
    c->host_pending = true;
    return LDPC_OK;
}

extern "C" int ldpc_decode_i8_host_async(ldpc_ctx *c, void *s, const int8_t *llr, uint8_t *hard, int batch,
                                         int n_iter, const ldpc_params *p)
{
    return decode_host_async(c, s, llr, hard, batch, n_iter, p, false);
}

extern "C" int ldpc_decode_f32_host_async(ldpc_ctx *c, void *s, const float *llr, uint8_t *hard, int batch,
                                          int n_iter, const ldpc_params *p)
{
    return decode_host_async(c, s, llr, hard, batch, n_iter, p, true);
}

extern "C" int ldpc_ctx_synchronize(ldpc_ctx *c)
{
    if (!c) return ldpc_set_error(LDPC_EINVAL, "NULL ctx");
    if (!c->host_pending) return LDPC_OK;
    HIP_TRY(hipSetDevice(c->device));
    c->host_pending = false;
    HIP_TRY(hipEventSynchronize(c->host_done));
    return LDPC_OK;
}

extern "C" int ldpc_host_alloc(void **p, size_t bytes)
{
    if (!p) return ldpc_set_error(LDPC_EINVAL, "NULL pointer");
    *p = nullptr;
    if (bytes == 0) return LDPC_OK;
    const hipError_t e = hipHostMalloc(p, bytes, hipHostMallocDefault);
    if (e != hipSuccess) {
        *p = nullptr;
        return ldpc_set_error(LDPC_ENOMEM, "hipHostMalloc(%zu): %s", bytes, hipGetErrorString(e));
    }
    return LDPC_OK;
}

extern "C" void ldpc_host_free(void *p)
{
    if (p) (void)hipHostFree(p);
}

extern "C" int ldpc_decode_i8(ldpc_ctx *c, const int8_t *llr, uint8_t *hard, int batch, int n_iter,
                              const ldpc_params *p)
{
    return decode_host(c, llr, hard, batch, n_iter, p, false);
}

extern "C" int ldpc_decode_f32(ldpc_ctx *c, const float *llr, uint8_t *hard, int batch, int n_iter,
                               const ldpc_params *p)
{
    return decode_host(c, llr, hard, batch, n_iter, p, true);
}

// the host decoder's float decode with the outputs the device entry points
// have: what a test compares the kernels' soft output and iteration counts to
extern "C" int ldpc_decode_f32_soft(ldpc_ctx *c, const float *llr, uint8_t *hard, float *soft, int32_t *iters_used,
                                    int batch, int n_iter, const ldpc_params *p)
{
    if (!c || ((!llr || !hard) && batch > 0)) return ldpc_set_error(LDPC_EINVAL, "NULL ctx/llr/hard");
    const int rc = check_params(c, batch, n_iter, p, true);
    if (rc != LDPC_OK || batch == 0) return rc;
    if (c->device >= 0)
        return ldpc_set_error(LDPC_EUNSUPPORTED, "ldpc_decode_f32_soft takes a host context (device -1); a GPU "
                              "context returns soft output through ldpc_decode_f32_async");
    c->last_kernel = LDPC_KERNEL_HOST;
    return host_decode_f32(c->code, llr, hard, soft, iters_used, batch, n_iter, p);
}

extern "C" int ldpc_awgn_i8_async(ldpc_ctx *c, void *s, int8_t *d_llr, int batch, uint64_t first_cw, uint64_t seed,
                                  const uint32_t *table, const uint8_t *d_codeword)
{
    if (!c || !d_llr || !table || batch < 0) return ldpc_set_error(LDPC_EINVAL, "awgn args");
    if (c->device < 0) return host_only(c);
    if (table[63] < 1 || table[63] > 31) return ldpc_set_error(LDPC_EINVAL, "awgn table sat");
    HIP_TRY(hipSetDevice(c->device));
    AwgnTable t;
    memcpy(t.t, table, sizeof(t.t));
    if (launch_awgn_i8(d_llr, c->code->n, batch, first_cw, seed, t, d_codeword, (hipStream_t)s))
        return ldpc_set_error(LDPC_EDEVICE, "awgn: %s", hipGetErrorString(hipGetLastError()));
    return LDPC_OK;
}

// the float channel (generator: awgn_f32.h; host twin: ldpc_awgn_f32_host), where the reference calls
// CChanelAWGN_MKL::generate (code/x86/CChanel/CChanelAWGN_MKL.cpp:127-143)
extern "C" int ldpc_awgn_f32_async(ldpc_ctx *c, void *s, float *d_y, int batch, uint64_t first_cw, uint64_t seed,
                                   double sigma, double amp, double norm, const uint8_t *d_codeword)
{
    if (!c || !d_y || batch < 0 || !(sigma > 0.0) || !(amp > 0.0) || !(norm > 0.0) || ((uintptr_t)d_y & 3))
        return ldpc_set_error(LDPC_EINVAL, "awgn f32 args: y non-NULL and 4-byte aligned, batch>=0, sigma>0, "
                                           "amp>0, norm>0");
    if (c->device < 0) return host_only(c);
    if (batch == 0) return LDPC_OK;
    HIP_TRY(hipSetDevice(c->device));
    if (launch_awgn_f32(d_y, c->code->n, batch, first_cw, seed, sigma, amp, norm, d_codeword, (hipStream_t)s))
        return ldpc_set_error(LDPC_EDEVICE, "awgn f32: %s", hipGetErrorString(hipGetLastError()));
    return LDPC_OK;
}

// the bit source of the chain (the reference's CBitGenerator::generate): K = n - m bits per codeword
extern "C" int ldpc_info_bits_async(ldpc_ctx *c, void *s, uint8_t *d_info, int batch, uint64_t first_cw,
                                    uint64_t seed)
{
    if (!c || batch < 0 || (batch > 0 && !d_info)) return ldpc_set_error(LDPC_EINVAL, "info_bits args");
    if (c->device < 0) return host_only(c);
    if (batch == 0) return LDPC_OK;
    HIP_TRY(hipSetDevice(c->device));
    if (launch_info_bits(d_info, c->code->n - c->code->m, batch, first_cw, seed, (hipStream_t)s))
        return ldpc_set_error(LDPC_EDEVICE, "info_bits: %s", hipGetErrorString(hipGetLastError()));
    return LDPC_OK;
}

// do [batch][K] information bits and [batch][N] codewords share a byte?
static bool encode_overlap(const ldpc_code *h, const uint8_t *d_info, const uint8_t *d_codeword, int batch)
{
    const uintptr_t i0 = (uintptr_t)d_info, c0 = (uintptr_t)d_codeword;
    return i0 < c0 + (size_t)batch * h->n && c0 < i0 + (size_t)batch * (h->n - h->m);
}

// device twin of ldpc_dvbs2_encode (code.cpp): no scratch, so any batch
extern "C" int ldpc_dvbs2_encode_async(ldpc_ctx *c, void *s, const uint8_t *d_info, uint8_t *d_codeword, int batch)
{
    if (!c || batch < 0 || (batch > 0 && (!d_info || !d_codeword)))
        return ldpc_set_error(LDPC_EINVAL, "encode args");
    if (c->device < 0) return host_only(c);
    const ldpc_code *h = c->code;
    if (h->dvbs2_q <= 0) return ldpc_set_error(LDPC_EUNSUPPORTED, "code was not built from a DVB-S2 table");
    if (!c->enc.valid)
        return ldpc_set_error(LDPC_EUNSUPPORTED, "encoder: a codeword of n = %d needs %zu B of LDS, one workgroup "
                              "has %zu", h->n, encode_lds_bytes(h->n - h->m, h->m), kEncMaxLds);
    if (batch == 0) return LDPC_OK;
    if (encode_overlap(h, d_info, d_codeword, batch))
        return ldpc_set_error(LDPC_EINVAL, "encode: d_info and d_codeword overlap");
    HIP_TRY(hipSetDevice(c->device));
    if (launch_dvbs2_encode(c->enc, d_info, d_codeword, batch, (hipStream_t)s))
        return ldpc_set_error(LDPC_EDEVICE, "encode: %s", hipGetErrorString(hipGetLastError()));
    return LDPC_OK;
}

// attach a general encoder (genc_host.cpp): uploads P and the position tables of a
// code that needs them; an Annex-B code's encoder only marks the context, its
// table went up with the context
extern "C" int ldpc_ctx_set_encoder(ldpc_ctx *c, const ldpc_encoder *e)
{
    if (!c || !e) return ldpc_set_error(LDPC_EINVAL, "set_encoder: NULL %s", !c ? "context" : "encoder");
    const ldpc_code *h = c->code;
    if (e->code != h && (e->n != h->n || e->m != h->m || e->code_hash != genc_code_hash(h)))
        return ldpc_set_error(LDPC_EINVAL, "set_encoder: the encoder was built for another code (%dx%d, the "
                              "context's is %dx%d)", e->n, e->m, h->n, h->m);
    if (c->device < 0) return host_only(c);
    HIP_TRY(hipSetDevice(c->device));
    // the previous encoder's tables may still be read by queued launches
    if (c->genc.valid) HIP_TRY(hipDeviceSynchronize());
    genc_free(&c->genc);
    c->genc_attached = false;
    c->genc_ira = e->ira;
    if (!e->ira) {
        int rc = genc_upload(e, &c->genc);
        if (rc != LDPC_OK) return rc;
    }
    c->genc_attached = true;
    return LDPC_OK;
}

// device twin of ldpc_encode (genc_host.cpp): no scratch, so any batch
extern "C" int ldpc_encode_async(ldpc_ctx *c, void *s, const uint8_t *d_info, uint8_t *d_codeword, int batch)
{
    if (!c || batch < 0 || (batch > 0 && (!d_info || !d_codeword)))
        return ldpc_set_error(LDPC_EINVAL, "encode args");
    if (c->device < 0) return host_only(c);
    if (!c->genc_attached)
        return ldpc_set_error(LDPC_EINVAL, "encode: no encoder attached to the context (ldpc_ctx_set_encoder)");
    if (c->genc_ira) return ldpc_dvbs2_encode_async(c, s, d_info, d_codeword, batch);   // the IRA kernel
    if (batch == 0) return LDPC_OK;
    const ldpc_code *h = c->code;
    if (encode_overlap(h, d_info, d_codeword, batch))
        return ldpc_set_error(LDPC_EINVAL, "encode: d_info and d_codeword overlap");
    HIP_TRY(hipSetDevice(c->device));
    if (launch_genc(c->genc, d_info, d_codeword, batch, (hipStream_t)s))
        return ldpc_set_error(LDPC_EDEVICE, "encode: %s", hipGetErrorString(hipGetLastError()));
    return LDPC_OK;
}

static bool quantize_args_ok(long count, int factor, int sat_neg, int sat_pos)
{
    return count >= 0 && factor >= 1 && sat_neg >= -128 && sat_pos <= 127 && sat_neg <= sat_pos;
}

extern "C" int ldpc_quantize_f32_i8_async(ldpc_ctx *c, void *s, const float *d_y, int8_t *d_q, long count, int factor,
                                          int sat_neg, int sat_pos)
{
    if (!c || (count > 0 && (!d_y || !d_q)) || !quantize_args_ok(count, factor, sat_neg, sat_pos))
        return ldpc_set_error(LDPC_EINVAL, "quantize args");
    if (c->device < 0) return host_only(c);
    HIP_TRY(hipSetDevice(c->device));
    if (launch_quantize_f32_i8(d_y, d_q, count, factor, sat_neg, sat_pos, (hipStream_t)s))
        return ldpc_set_error(LDPC_EDEVICE, "quantize: %s", hipGetErrorString(hipGetLastError()));
    return LDPC_OK;
}

extern "C" int ldpc_quantize_f32_i8(ldpc_ctx *c, const float *y, int8_t *q, long count, int factor, int sat_neg,
                                    int sat_pos)
{
    if (!c || (count > 0 && (!y || !q)) || !quantize_args_ok(count, factor, sat_neg, sat_pos))
        return ldpc_set_error(LDPC_EINVAL, "quantize args");
    if (count == 0) return LDPC_OK;
    if (c->device < 0) {   // host context: CFastFixConversion::generate's rule on the CPU (quantize_k's)
        for (long i = 0; i < count; i++) {
            const float v = (float)factor * y[i];
            int value = (std::fabs(v) < 2147483648.0f) ? (int)v : INT_MIN;
            value = std::min(std::max(value, sat_neg), sat_pos);
            q[i] = (int8_t)value;
        }
        return LDPC_OK;
    }
    HIP_TRY(hipSetDevice(c->device));
    const size_t in_bytes = (size_t)count * sizeof(float), al = (in_bytes + 255) & ~(size_t)255;
    int rc;
    if ((rc = ensure(&c->d_io, &c->io_bytes, al + (size_t)count)) != LDPC_OK) return rc;
    float *d_y = (float *)c->d_io;
    int8_t *d_q = (int8_t *)c->d_io + al;
    const hipStream_t s = c->stream;
    HIP_TRY(hipMemcpyAsync(d_y, y, in_bytes, hipMemcpyHostToDevice, s));
    if (launch_quantize_f32_i8(d_y, d_q, count, factor, sat_neg, sat_pos, s))
        return ldpc_set_error(LDPC_EDEVICE, "quantize: %s", hipGetErrorString(hipGetLastError()));
    HIP_TRY(hipMemcpyAsync(q, d_q, (size_t)count, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return LDPC_OK;
}

extern "C" int ldpc_count_errors_async(ldpc_ctx *c, void *s, const uint8_t *d_hard, int batch, int k,
                                       const uint8_t *d_ref, unsigned long long *d_counts)
{
    if (!c || !d_hard || !d_counts || batch < 0 || k < 0 || k > c->code->n)
        return ldpc_set_error(LDPC_EINVAL, "count_errors args");
    if (c->device < 0) return host_only(c);
    HIP_TRY(hipSetDevice(c->device));
    if (launch_count_errors(d_hard, c->code->n, batch, k, d_ref, d_counts, (hipStream_t)s))
        return ldpc_set_error(LDPC_EDEVICE, "count_errors: %s", hipGetErrorString(hipGetLastError()));
    return LDPC_OK;
}
