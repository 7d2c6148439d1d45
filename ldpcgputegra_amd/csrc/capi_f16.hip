// capi_f16.hip -- the binary16 entry points of the C-ABI: the decode of device
// buffers on the packed staircase kernel (stairh.hip), the host-buffer decode,
// the host decoder's twin with soft output, and the float -> binary16
// conversion.  binary16 travels as uint16_t bit patterns.  Host code only.
//
// The f16 decode has a selection of its own (pick_f16 below), not dispatch.hip's.
// By default it has one GPU kernel: a code stairf_upload accepts runs on stairh
// (reported as LDPC_KERNEL_STAIRF, another element type of that family), any
// other code is LDPC_EUNSUPPORTED on a GPU context.  With
// ldpc_ctx_set_f16_all_codes on, the other codes run on the packed LDS-resident
// kernel (ldsh, reported as LDPC_KERNEL_LDS) or the packed any-H kernel
// (generich, LDPC_KERNEL_GENERIC), which can also be forced on any code.  The
// scratch is the context's own (the V and message buffers the other element
// types use, grown as needed).  ldpc_ctx_set_f16_edge_parallel, a switch of
// its own, puts the edge-parallel kernel of the short QC codes in front of all
// that (ldseph, LDPC_KERNEL_LDSEP): the automatic choice and a forced 9 where
// the code fits it, every other setting decided as without it.
#include <cmath>
#include <cstring>

#include "ctx.h"
#include "host.h"
#include "ldsh.h"
#include "stairh.h"

namespace {

int check_params_f16(const ldpc_ctx *c, int batch, int n_iter, const ldpc_params *p)
{
    int rc = check_params(c, batch, n_iter, p, true);   // batch, n_iter, p, the algorithm's range
    if (rc != LDPC_OK) return rc;
    if (p->algo == LDPC_ALGO_BP)
        return ldpc_set_error(LDPC_EUNSUPPORTED, "belief propagation has no binary16 decode (float32 input only)");
    if (p->algo != LDPC_ALGO_MS) {
        const float b = p->beta;
        if (!std::isfinite(b) || b < 0.0f || std::isinf((float)(_Float16)b))
            return ldpc_set_error(LDPC_EINVAL, "beta %g: the binary16 decode takes a finite beta >= 0 that rounds to a "
                                  "finite binary16 value", (double)b);
    }
    return LDPC_OK;
}

// the kernel family of this call, or a status < 0 with the error set.  Switch
// off: the staircase kernel or nothing, as before the switch existed.
int pick_f16(const ldpc_ctx *c)
{
    const ldpc_code *h = c->code;
    const bool automatic = c->kernel == LDPC_KERNEL_AUTO;
    // checked first, as dispatch.hip does for float32; independent of f16_all_codes
    if (c->f16_edge_parallel && (automatic || c->kernel == LDPC_KERNEL_LDSEP) && ldseph_applicable(h, c->lds))
        return LDPC_KERNEL_LDSEP;
    if (!c->f16_all_codes) {
        if (!c->stairf.valid)
            return ldpc_set_error(LDPC_EUNSUPPORTED, "the binary16 decode runs on the staircase kernel only (DVB-S2 and "
                                  "like-shaped codes); this %dx%d code has no staircase table: decode it in float32, or in "
                                  "binary16 on a host context", h->n, h->m);
        if (!automatic && c->kernel != LDPC_KERNEL_STAIRF)
            return ldpc_set_error(LDPC_EUNSUPPORTED, "kernel %d selected but not applicable to a binary16 decode",
                                  c->kernel);
        return LDPC_KERNEL_STAIRF;
    }
    if (automatic) {
        if (c->stairf.valid) return LDPC_KERNEL_STAIRF;
        return lds_preferred(h, c->lds, true) ? LDPC_KERNEL_LDS : LDPC_KERNEL_GENERIC;
    }
    if (c->kernel == LDPC_KERNEL_GENERIC) return LDPC_KERNEL_GENERIC;
    if (c->kernel == LDPC_KERNEL_LDS && lds_applicable(h, c->lds, true)) return LDPC_KERNEL_LDS;
    if (c->kernel == LDPC_KERNEL_STAIRF && c->stairf.valid) return LDPC_KERNEL_STAIRF;
    return ldpc_set_error(LDPC_EUNSUPPORTED, "kernel %d selected but not applicable to a binary16 decode", c->kernel);
}

int decode_f16_device(ldpc_ctx *c, Scratch &sc, hipStream_t s, const uint16_t *d_llr, uint8_t *d_hard, uint16_t *d_soft,
                      int32_t *d_iters, int batch, int n_iter, const ldpc_params *p)
{
    int rc = check_params_f16(c, batch, n_iter, p);
    if (rc != LDPC_OK) return rc;
    if (c->device < 0) return host_only(c);
    if (((uintptr_t)d_llr | (uintptr_t)d_soft) & 1)
        return ldpc_set_error(LDPC_EINVAL, "binary16 buffers must be 2-byte aligned");
    if (batch == 0) return LDPC_OK;
    const ldpc_code *h = c->code;
    const int kern = pick_f16(c);
    if (kern < 0) return kern;
    const bool ms = p->algo == LDPC_ALGO_MS, early = p->early_term != 0;
    DecodeLaunch L{};
    L.batch = batch;
    L.iters = n_iter;
    L.is_float = 1;
    L.d_edge_var = c->d_edge_var;
    L.d_group_deg = c->d_group_deg;
    L.d_group_cnt = c->d_group_cnt;
    L.n_groups = h->n_groups;
    L.n = h->n;
    L.m = h->m;
    L.e = h->e;
    L.algo = ms ? LDPC_ALGO_OMS : p->algo;
    L.beta = ms ? 0.0f : p->beta;
    L.early = early;
    L.iters_used = d_iters;
    // checks that refuse come before anything is allocated, read or recorded
    int stride = 0, lg = 0, split = 0;
    if (kern == LDPC_KERNEL_STAIRF) {
        stride = (batch + 63) / 64 * 64;
        if (!stairh_stride_ok(c->stairf, h->n, stride))
            return ldpc_set_error(LDPC_EUNSUPPORTED, "binary16 decode: batch %d of n = %d passes the kernel's 32-bit V "
                                  "offsets ((n + 1) * stride * 2 < 2^32); split the batch", batch, h->n);
    } else if (kern == LDPC_KERNEL_LDS) {
        if (ldsh_shape(h, c->lds, batch, &lg, &split))
            return ldpc_set_error(LDPC_EUNSUPPORTED, "binary16 decode: LDPC_LDSH_LANES asks for a shape this %dx%d code "
                                  "cannot run (its widest layer needs %d lanes per pair, and the state of the pairs of "
                                  "a wave must fit 64 KB of LDS)", h->n, h->m, 1 << c->lds.lpc_log2);
    } else if (kern == LDPC_KERNEL_GENERIC) {
        stride = generich_stride(batch);
    }   // (ldseph has nothing to refuse)
    HIP_TRY(hipSetDevice(c->device));
    c->last_kernel = kern;
    c->last_skipped = 0;
    c->last_lds_lanes = c->last_lds_split = 0;
    c->last_et_stage = 0;
    c->last_ep_waves = 0;
    // ldsh and ldseph: frame-major in and out, the whole state in LDS (and registers): no scratch
    const bool resident = kern == LDPC_KERNEL_LDS || kern == LDPC_KERNEL_LDSEP;
    if (kern == LDPC_KERNEL_LDS) {
        c->last_lds_lanes = 1 << lg;
        c->last_lds_split = split;
    } else if (!resident) {
        size_t v_bytes, msg_bytes, early_bytes = 0;
        if (kern == LDPC_KERNEL_STAIRF) {
            v_bytes = stairh_v_bytes(h->n, stride);
            msg_bytes = stairh_msg_bytes(c->stairf, stride);
            early_bytes = early ? (size_t)stride * 12 : 0;
        } else {
            v_bytes = (size_t)h->n * stride * 2;
            msg_bytes = (size_t)h->e * stride * 2;
        }
        if ((rc = ensure(&sc.d_V, &sc.V_bytes, v_bytes)) != LDPC_OK ||
            (rc = ensure(&sc.d_msg, &sc.msg_bytes, msg_bytes + 4096)) != LDPC_OK ||
            (rc = ensure(&sc.d_early, &sc.early_bytes, early_bytes)) != LDPC_OK)
            return rc;
        HIP_TRY(hipMemsetAsync(sc.d_msg, 0, msg_bytes, s));   // messages start at +0
        if (launch_interleave_f16(d_llr, (uint16_t *)sc.d_V, h->n, batch, stride, s))
            return ldpc_set_error(LDPC_EDEVICE, "interleave: %s", hipGetErrorString(hipGetLastError()));
        L.V = sc.d_V;
        L.msg = sc.d_msg;
        L.stride = L.vpitch = stride;
        if (early && kern == LDPC_KERNEL_STAIRF) {   // (iterations used land in the scratch when the caller passed no array)
            L.bad = (uint32_t *)sc.d_early;
            if (!L.iters_used) L.iters_used = (int32_t *)((char *)sc.d_early + (size_t)stride * 4);
            L.live = (uint8_t *)sc.d_early + (size_t)stride * 8;
        }
    }
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    if (c->profile) {
        HIP_TRY(hipEventCreate(&ev0));
        HIP_TRY(hipEventCreate(&ev1));
        HIP_TRY(hipEventRecord(ev0, s));
    }
    const int lr = kern == LDPC_KERNEL_STAIRF ? launch_stairh(L, c->stairf, s)
                   : kern == LDPC_KERNEL_LDS  ? launch_ldsh(c->lds, h, d_llr, d_hard, d_soft, L, lg, split, s)
                   : kern == LDPC_KERNEL_LDSEP ? launch_ldseph(c->lds, h, d_llr, d_hard, d_soft, L, s)
                                              : launch_generich(L, s);
    if (c->profile) {
        HIP_TRY(hipEventRecord(ev1, s));
        c->events.emplace_back(ev0, ev1);
    }
    if (lr) {
        const hipError_t e = hipGetLastError();
        const char *why = e != hipSuccess ? hipGetErrorString(e) : "launch configuration rejected by the host side";
        return ldpc_set_error(LDPC_EDEVICE, "binary16 decode launch: %s", why);
    }
    if (!resident && (d_hard || d_soft) &&
        launch_deinterleave_f16((const uint16_t *)sc.d_V, d_hard, d_soft, h->n, batch, stride, s))
        return ldpc_set_error(LDPC_EDEVICE, "deinterleave: %s", hipGetErrorString(hipGetLastError()));
    return LDPC_OK;
}

}  // namespace

extern "C" int ldpc_decode_f16_async(ldpc_ctx *c, void *s, const uint16_t *d_llr, uint8_t *d_hard, uint16_t *d_soft,
                                     int32_t *d_iters, int batch, int n_iter, const ldpc_params *p)
{
    if (!c || (!d_llr && batch > 0)) return ldpc_set_error(LDPC_EINVAL, "NULL ctx/llr");
    return decode_f16_device(c, c->sc, (hipStream_t)s, d_llr, d_hard, d_soft, d_iters, batch, n_iter, p);
}

// host buffers, synchronous: the host decoder on a device -1 context, else a
// plain copy in, decode, copy out on the context's stream and staging
extern "C" int ldpc_decode_f16(ldpc_ctx *c, const uint16_t *llr, uint8_t *hard, int batch, int n_iter,
                               const ldpc_params *p)
{
    if (!c || ((!llr || !hard) && batch > 0)) return ldpc_set_error(LDPC_EINVAL, "NULL ctx/llr/hard");
    int rc = check_params_f16(c, batch, n_iter, p);
    if (rc != LDPC_OK || batch == 0) return rc;
    if (c->device < 0) {
        c->last_kernel = LDPC_KERNEL_HOST;
        return host_decode_f16(c->code, llr, hard, nullptr, nullptr, batch, n_iter, p);
    }
    HIP_TRY(hipSetDevice(c->device));
    if (c->host_pending) {   // a queued asynchronous host-buffer decode still uses the staging
        c->host_pending = false;
        HIP_TRY(hipEventSynchronize(c->host_done));
    }
    const size_t n = (size_t)c->code->n, in_al = ((size_t)batch * n * 2 + 255) / 256 * 256;
    if ((rc = ensure(&c->d_io, &c->io_bytes, in_al + (size_t)batch * n)) != LDPC_OK) return rc;
    char *d_in = (char *)c->d_io, *d_out = d_in + in_al;
    const hipStream_t s = c->stream;
    HIP_TRY(hipMemcpyAsync(d_in, llr, (size_t)batch * n * 2, hipMemcpyHostToDevice, s));
    rc = decode_f16_device(c, c->sc, s, (const uint16_t *)d_in, (uint8_t *)d_out, nullptr, nullptr, batch, n_iter, p);
    if (rc == LDPC_OK) {
        const hipError_t e = hipMemcpyAsync(hard, d_out, (size_t)batch * n, hipMemcpyDeviceToHost, s);
        if (e != hipSuccess) rc = ldpc_set_error(LDPC_EDEVICE, "host path D2H: %s", hipGetErrorString(e));
    }
    const hipError_t e = hipStreamSynchronize(s);   // joined on success and on error
    if (e != hipSuccess && rc == LDPC_OK) rc = ldpc_set_error(LDPC_EDEVICE, "host path: %s", hipGetErrorString(e));
    return rc;
}

// the host decoder's binary16 decode with the outputs the device entry point
// has: the definition the kernel's soft output and iteration counts are compared to
extern "C" int ldpc_decode_f16_soft(ldpc_ctx *c, const uint16_t *llr, uint8_t *hard, uint16_t *soft,
                                    int32_t *iters_used, int batch, int n_iter, const ldpc_params *p)
{
    if (!c || ((!llr || !hard) && batch > 0)) return ldpc_set_error(LDPC_EINVAL, "NULL ctx/llr/hard");
    const int rc = check_params_f16(c, batch, n_iter, p);
    if (rc != LDPC_OK || batch == 0) return rc;
    if (c->device >= 0)
        return ldpc_set_error(LDPC_EUNSUPPORTED, "ldpc_decode_f16_soft takes a host context (device -1); a GPU "
                              "context returns soft output through ldpc_decode_f16_async");
    c->last_kernel = LDPC_KERNEL_HOST;
    return host_decode_f16(c->code, llr, hard, soft, iters_used, batch, n_iter, p);
}

extern "C" int ldpc_convert_f32_f16_host(const float *y, uint16_t *h, long count)
{
    if (count < 0 || (count > 0 && (!y || !h))) return ldpc_set_error(LDPC_EINVAL, "convert args");
    for (long i = 0; i < count; i++) h[i] = host_f16_from_f32(y[i]);
    return LDPC_OK;
}

extern "C" int ldpc_convert_f32_f16_async(ldpc_ctx *c, void *s, const float *d_y, uint16_t *d_h, long count)
{
    if (!c || count < 0 || (count > 0 && (!d_y || !d_h))) return ldpc_set_error(LDPC_EINVAL, "convert args");
    if (c->device < 0) return host_only(c);
    if (count == 0) return LDPC_OK;
    if (((uintptr_t)d_y & 3) || ((uintptr_t)d_h & 1))
        return ldpc_set_error(LDPC_EINVAL, "convert: y must be 4-byte, h 2-byte aligned");
    HIP_TRY(hipSetDevice(c->device));
    if (launch_convert_f32_f16(d_y, d_h, count, (hipStream_t)s))
        return ldpc_set_error(LDPC_EDEVICE, "convert: %s", hipGetErrorString(hipGetLastError()));
    return LDPC_OK;
}
