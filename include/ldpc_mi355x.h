/*
 * ldpc_mi355x.h -- C-ABI of the MI355X layered min-sum LDPC decoder.
 *
 * This is the drop-in boundary for the reference's decode path
 * (boiseHPSim/ldpcGpuTegra).  Plain C types only: no HIP or torch types in any
 * signature (streams are passed as `void *` holding a hipStream_t).  Every
 * function returns an int status (LDPC_OK == 0, negative on error) and never
 * exits the process -- unlike the reference, which prints and calls exit(0)
 * (code/x86/CDecoder/DecoderLibrary.h:37-41, code/gpu_fixed/custom_api/
 * custom_cuda.cu:5-17).
 *
 * Entry point -> reference interface it replaces:
 *   ldpc_code_create / ldpc_code_load / ldpc_code_from_dvbs2_table
 *       -> the compile-time H table PosNoeudsVariable[] + DEG_k macros
 *          (code/x86/Constantes/constantes_sse.h:1-2,
 *           code/x86/Constantes/64800x32400.dvb-s2/constantes_sse.h:6-36)
 *   ldpc_ctx_create(code, device, max_batch)
 *       -> CGPUDecoder(nb_frames, n, k, m) + initialize()
 *          (code/gpu_fixed/decoder_template/CGPUDecoder.h:20-37) and the
 *          decoder constructors that allocate V / msg scratch
 *          (code/x86/CDecoder/template/CDecoder_fixed_SSE.cpp:23-27)
 *   ldpc_params {algo, offset, factor, var/msg range}
 *       -> CreateDecoder(type, arch, format, p_decoder, vMin, vMax, mMin, mMax)
 *          (code/x86/CDecoder/DecoderLibrary.h:44-134), setOffset
 *          (OMS/CDecoder_OMS_fixed_SSE.cpp:104-112), setFactor
 *          (NMS/CDecoder_NMS_fixed_SSE.cpp:107-111), setVarRange/setMsgRange
 *          (template/CDecoder_fixed.h:40-41)
 *   ldpc_decode_i8(ctx, llr, hard, batch, n_iter, params)
 *       -> CDecoder::decode(char var_nodes[], char Rprime_fix[], int iters)
 *          (code/x86/CDecoder/template/CDecoder.h:37), 16 frames per call
 *          there, any batch here; same frame-major layout, same 0/1 output
 *   ldpc_decode_f32(...)
 *       -> CDecoder::decode(float var_nodes[], char Rprime_fix[], int)
 *          (CDecoder.h:38; a no-op for the reference's fixed-point decoders)
 *          and CGPUDecoder::decode(float[], int[], int) (CGPUDecoder.h:31)
 *   ldpc_decode_i8_async / _f32_async
 *       -> CGPU_Decoder_*_SIMD::decode_stream
 *          (code/gpu_fixed/decoder_ms/CGPU_Decoder_MS_SIMD.cu:219-275),
 *          device pointers, caller-owned stream, no hidden sync
 *   ldpc_awgn_*  -> CChanelAWGN_MKL::configure/generate + CFastFixConversion
 *          (code/x86/CChanel/CChanelAWGN_MKL.cpp:95-143,
 *           code/x86/CFixPointConversion/CFastFixConversion.cpp:55-65) and the
 *          on-GPU channel (code/gpu_fixed/awgn_channel/CChanel_AWGN_SIMD.cu:7-30)
 *   ldpc_count_errors_async -> CErrorAnalyzer::generate
 *          (code/x86/CErrorAnalyzer/CErrorAnalyzer.cpp:123-154)
 *   ldpc_info_bits_host / _async -> CBitGenerator::generate (rand() % 2 per
 *          information bit, called per frame at code/x86/main_p.cpp:431-445),
 *          with a counter-based generator indexed per codeword
 *   ldpc_dvbs2_encode / _async -> GenericEncoder::encode
 *          (code/x86/CEncoder/GenericEncoder.cpp:38-78)
 *   ldpc_encoder_* / ldpc_encode / _async -> nothing: the reference encodes
 *          IRA codes only; these encode every ldpc_code
 *
 * Threading: a ldpc_code is immutable and may be shared by any number of
 * contexts/threads.  A ldpc_ctx owns device scratch and is not re-entrant
 * (like the reference decoder objects); use one per host thread / stream.
 */
#ifndef LDPC_MI355X_H
#define LDPC_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LDPC_ABI_VERSION 1

enum {
    LDPC_OK = 0,
    LDPC_EINVAL = -1,      /* bad argument, H table, or saturation ranges */
    LDPC_EUNSUPPORTED = -2,/* valid request the reference would reject (exit) */
    LDPC_EDEVICE = -3,     /* HIP error; see ldpc_last_error() */
    LDPC_ENOMEM = -4,      /* host or device allocation failed */
    LDPC_EIO = -5          /* file not found / malformed table file */
};

enum {
    LDPC_ALGO_OMS = 0,     /* offset min-sum   (CDecoder_OMS_fixed_SSE) */
    LDPC_ALGO_NMS = 1,     /* normalised min-sum (CDecoder_NMS_fixed_SSE) */
    LDPC_ALGO_MS = 2,      /* plain min-sum == OMS with offset 0 */
    LDPC_ALGO_BP = 3       /* layered belief propagation (sum-product), float input only: the
                              algorithm the three above approximate.  Its check update is the
                              box-plus a [+] b = -2 atanh(tanh(a/2) tanh(b/2)) (negated: this
                              decoder reads V > 0 as bit 1), chained forward / backward over the
                              check's edges, with ln(1 + e^-x) written out in IEEE + - * so that
                              host and device agree bit for bit (csrc/bp_math.h).
                              beta is ignored.  Not scale-invariant as min-sum is: the input
                              must be the true LLR 2y / sigma^2.  Int8 input: LDPC_EUNSUPPORTED
                              (the reference has no fixed-point BP).  Runs on LDPC_KERNEL_LDS
                              (the automatic choice where lds_f32 of ldpc_code_layer_info
                              prefers it), LDPC_KERNEL_GENERIC (any code) and, on a context
                              with ldpc_ctx_set_bp_staircase on, LDPC_KERNEL_STAIRF (the
                              DVB-S2 staircase codes, bit for bit the same results); every
                              other forced family is LDPC_EUNSUPPORTED.  With that switch off
                              (the default) a DVB-S2 code decodes BP on the generic kernel:
                              correct, slow; ldpc_ctx_last_skipped then names
                              LDPC_KERNEL_STAIRF as the family passed over.
                              LDPC_KERNEL_LDSEP has no BP: its parallel prefix over the
                              edges would reorder the box-plus chain, and LDPC_KERNEL_LDS
                              serves those codes */
};

typedef struct ldpc_code ldpc_code;
typedef struct ldpc_ctx ldpc_ctx;

typedef struct {
    int algo;        /* LDPC_ALGO_*                                  default OMS */
    int offset;      /* int8 OMS offset (setOffset)                  default 1   */
    int factor;      /* int8 NMS factor, scaled by 1/32 (setFactor)  default 29  */
    float beta;      /* float path: OMS offset or NMS factor (BP: unused) default 0.15*/
    int var_min;     /* setVarRange(min, max)                   default -127,127 */
    int var_max;
    int msg_min;     /* setMsgRange(min, max)                   default -31, 31  */
    int msg_max;
    int early_term;  /* stop a codeword once H*x == 0 (0 = exact n_iter); the
                        DVB-S2 r1/2 kernel decodes batches >= 8192 in stages,
                        compacting the codewords still decoding every few
                        iterations (LDPC_COOP3_ET_K / _STEP / _STAGE_MIN) */
} ldpc_params;

/* ---- errors / version ------------------------------------------------ */
void ldpc_params_default(ldpc_params *p);
const char *ldpc_strerror(int status);
const char *ldpc_last_error(void);          /* thread-local detail of the last error */
int ldpc_abi_version(void);
int ldpc_device_count(int *count);

/* ---- code tables ----------------------------------------------------- */
/* Layered H: checks in schedule order, in n_groups runs of equal degree
 * (group g = group_cnt[g] checks of degree group_deg[g]); edge_var[E] lists
 * each check's variables.  Group 0 vs later groups matters for bit-exactness
 * (reference quirk). */
int ldpc_code_create(int n, int m, int n_groups, const int *group_deg, const int *group_cnt,
                     const uint32_t *edge_var, ldpc_code **out);
/* DVB-S2 IRA code from its Annex-B address table: row r lists row_len[r]
 * parity addresses (concatenated in row_addr).  Layered order as the
 * reference tables: checks 1..M-1 (info vars ascending, K+i-1, K+i), then
 * check 0 (info ascending, K). */
int ldpc_code_from_dvbs2_table(int n, int k_info, int n_rows, const int *row_len,
                               const int *row_addr, ldpc_code **out);
/* Load a ".ldpc" binary table or a DVB-S2 ".txt" address table. */
int ldpc_code_load(const char *path, ldpc_code **out);
int ldpc_code_info(const ldpc_code *h, int *n, int *m, int *e, int *n_groups, int *max_deg);
int ldpc_code_edges(const ldpc_code *h, uint32_t *edge_var, int *group_deg, int *group_cnt);
/* 1 if the layered schedule has the DVB-S2 staircase chain (fast kernel). */
int ldpc_code_plan_info(const ldpc_code *h, int *staircase, int *n_windows, int *min_hazard);
/* Window schedule of the windowed2 kernel for S checks per window and
 * read-ahead P: writes up to max_windows (first check, count) pairs and the
 * total count (0 when the code has no staircase schedule). */
int ldpc_code_window_plan(const ldpc_code *h, int S, int P, int *first, int *count, int max_windows,
                          int *n_windows);
/* Window schedule of the workgroup-cooperative kernel (S checks per window,
 * prefetch depth R windows): (first check, count) per window -- count 0 is
 * an empty window -- the window holding the tail check and the number of
 * info-edge reads per iteration forwarded through LDS.  n_windows = 0 when
 * the code has no such schedule. */
int ldpc_code_coop_plan(const ldpc_code *h, int S, int R, int *first, int *count, int max_windows,
                        int *n_windows, int *tail, int *n_fwd);
/* Same with the window distance rule of the kernel: dist = 1 (coop: consecutive
 * windows share no information variable) or 2 (coop2: nor do windows two
 * apart; reads written dist+1 .. R+dist windows earlier are forwarded). */
int ldpc_code_coop_plan_dist(const ldpc_code *h, int S, int R, int dist, int *first, int *count, int max_windows,
                             int *n_windows, int *tail, int *n_fwd);
/* Line cache of the DVB-S2 r1/2 kernel (kernel 8, coop3): the information
 * rows move between HBM and LDS as 128-B lines (8 rows x 16 codewords) on a
 * static plan checked by replaying it.  slots: LDS line slots the plan uses
 * (0 when the code has no coop3 schedule), max_slots: what the kernel has,
 * residencies: line loads per iteration, prologue / epilogue: lines filled /
 * written back at a segment start / end.  (Introspection for tests; replaces
 * no reference interface.) */
int ldpc_code_coop3_lc_info(const ldpc_code *h, int *slots, int *max_slots, int *residencies, int *prologue,
                            int *epilogue);
/* The line cache's modelled LDS bank conflicts: extra LDS cycles per
 * iteration and workgroup of coop3's pre reads / post writes of the line
 * cache with the planner's per-residency XOR swizzle (swizzled) and with
 * every line unswizzled (plain); 0 / 0 when the code has no coop3 schedule.
 * (Introspection for tests.) */
int ldpc_code_coop3_lc_banks(const ldpc_code *h, long long *swizzled, long long *plain);
/* The slots of the coop3 schedule as the kernel's records hold them: windows
 * per iteration, slots per window (S) and per slab wave, the window of the
 * tail check, and pt_mask: bit w set where slab wave w holds an inactive slot
 * in some window other than the tail's (only those waves run the pre's
 * pass-through selects in steady periods).  active (may be NULL, else room
 * for max_slots >= n_windows * S bytes): 1 where slot [window][slot] holds a
 * check.  n_windows = 0 when the code has no coop3 schedule.  (Introspection
 * for tests.) */
int ldpc_code_coop3_slots(const ldpc_code *h, int *n_windows, int *S, int *slots_per_wave, int *tail,
                          unsigned *pt_mask, unsigned char *active, int max_slots);
/* Layer plan of the LDS-resident kernel (kernel 7): maximal runs of
 * consecutive same-group checks sharing no variable (one block row of a
 * quasi-cyclic code).  lds_i8 / lds_f32: 1 if a codeword's state fits the
 * kernel's LDS budget for that element type. */
int ldpc_code_layer_info(const ldpc_code *h, int *n_layers, int *max_width, int *lds_i8, int *lds_f32);
void ldpc_code_destroy(ldpc_code *h);

/* ---- decoder context --------------------------------------------------- */
/* device >= 0: a GPU context on that HIP device.  device = -1: a host context
 * (no GPU needed): ldpc_decode_i8 / ldpc_decode_f32 /
 * ldpc_quantize_f32_i8 run on the CPU (AVX2 int8 over blocks of 32 codewords
 * on all host threads, LDPC_HOST_THREADS to cap them; the same bit-exact
 * results as the GPU kernels), the device-buffer entry points return
 * LDPC_EUNSUPPORTED and ldpc_ctx_last_kernel reports 10. */
int ldpc_ctx_create(const ldpc_code *h, int device, int max_batch, ldpc_ctx **out);
void ldpc_ctx_destroy(ldpc_ctx *ctx);
int ldpc_ctx_stream(ldpc_ctx *ctx, void **hip_stream);
/* Kernel families (ldpc_ctx_set_kernel / get_kernel / last_kernel /
 * last_skipped; the functions take and return plain int).  4 and 6 (windowed2
 * S = 32, coop2) were superseded: the values stay reserved and are rejected
 * with LDPC_EUNSUPPORTED. */
typedef enum ldpc_kernel {
    LDPC_KERNEL_AUTO = 0,       /* set_kernel: automatic choice; last_kernel: no decode yet */
    LDPC_KERNEL_GENERIC = 1,    /* per-edge messages, any code */
    LDPC_KERNEL_WINDOWED = 2,   /* windowed layered kernel (compressed messages) */
    LDPC_KERNEL_WINDOWED2 = 3,  /* windowed2 (S = 16) */
    LDPC_KERNEL_COOP = 5,       /* workgroup-cooperative DVB-S2 kernel */
    LDPC_KERNEL_LDS = 7,        /* LDS-resident short-code kernel (whole state in LDS; int8 and float) */
    LDPC_KERNEL_COOP3 = 8,      /* DVB-S2 first-group degree 7: slab waves doing pre + post, i16 chain */
    LDPC_KERNEL_LDSEP = 9,      /* float, short QC codes: one wave per codeword, one lane per edge;
                                   the automatic choice for float decodes of the codes it fits; binary16
                                   and int8 after ldpc_ctx_set_f16_edge_parallel / _i8_edge_parallel; the
                                   longer QC codes after ldpc_ctx_set_ep_wide (float) / _i8_ep_wide (int8) */
    LDPC_KERNEL_HOST = 10,      /* last_kernel of a device -1 context (the host decoder); not selectable */
    LDPC_KERNEL_STAIRF = 11     /* float, DVB-S2 staircase codes: S consecutive checks of 64/S codewords
                                   per wave, the staircase chain by DPP; the automatic choice for float
                                   decodes of those codes, early termination by one launch per
                                   iteration + a syndrome pass.  Min-sum (OMS / NMS / MS) always;
                                   LDPC_ALGO_BP after ldpc_ctx_set_bp_staircase(ctx, 1) */
} ldpc_kernel;
/* Select the kernel family (an ldpc_kernel value): LDPC_KERNEL_AUTO .. LDPC_KERNEL_LDSEP
 * or LDPC_KERNEL_STAIRF.  A value outside 0 .. 11, or LDPC_KERNEL_HOST, is
 * LDPC_EINVAL; a family that cannot schedule the context's code (the reserved
 * 4 and 6 included) is LDPC_EUNSUPPORTED and leaves the selection as it was. */
int ldpc_ctx_set_kernel(ldpc_ctx *ctx, int kernel);
int ldpc_ctx_get_kernel(ldpc_ctx *ctx, int *kernel);
/* Belief propagation on the staircase kernel (off by default).  On: an
 * LDPC_ALGO_BP decode of a float staircase code runs on LDPC_KERNEL_STAIRF --
 * the automatic choice wherever that family takes the batch (last_skipped 0),
 * and what a forced LDPC_KERNEL_STAIRF runs.  A batch too large for the family
 * ((n + 1) * stride * 4 >= 2^32, stride = the batch rounded up to 64) decodes
 * on LDPC_KERNEL_GENERIC under the automatic choice, and last_skipped names
 * LDPC_KERNEL_STAIRF (with the switch off it stays 0 for such a batch, as
 * before); forced LDPC_KERNEL_STAIRF is then LDPC_EUNSUPPORTED.  Forced LDPC_KERNEL_GENERIC / LDPC_KERNEL_LDS and
 * every other algorithm are unchanged.  Results equal the host decoder's bit
 * for bit on either kernel.  Off: BP never runs on LDPC_KERNEL_STAIRF (forced:
 * LDPC_EUNSUPPORTED).  set: LDPC_EUNSUPPORTED on a host context or a code
 * without a staircase table (ldpc_ctx_set_kernel(ctx, LDPC_KERNEL_STAIRF) fails
 * on the same codes), the setting stays as it was; LDPC_EINVAL for a NULL ctx. */
int ldpc_ctx_set_bp_staircase(ldpc_ctx *ctx, int enable);
int ldpc_ctx_get_bp_staircase(ldpc_ctx *ctx, int *enable);
/* The group width S (checks per wave group: 2, 4, 8 or 16) that a BP decode on
 * LDPC_KERNEL_STAIRF picks when LDPC_STAIRF_S does not force one: x information
 * edges per check, m checks, stride = the batch rounded up to 64, widths = the
 * widths the code has a table for (bit S set).  The least modelled cost
 * (m / S) * (3x - 1 + S) * f(w), w = stride * S / 64 / 256 waves per CU,
 * f = 1 up to two waves and (w / 2)^(5/8) beyond (fitted to measurement,
 * DESIGN.md section 7), the wider on a tie; 0 when no width in the mask divides m.
 * (Introspection for tests; needs no context and no GPU.  Unstable: the model
 * is fitted to one code and may change, or the entry go, in any release.) */
int ldpc_bp_staircase_width_model(int x, int m, int stride, unsigned widths);
/* Kernel family the last decode actually ran (an ldpc_kernel value;
 * LDPC_KERNEL_HOST on a device -1 context, 0 before the first decode). */
int ldpc_ctx_last_kernel(ldpc_ctx *ctx, int *kernel);
/* The fastest kernel of this code that the last automatic selection could
 * not use for the call's parameters (LDPC_KERNEL_COOP3, LDPC_KERNEL_COOP -- they take OMS / MS
 * with msg_max <= 63 and var range +-127), 0 when none was skipped. */
int ldpc_ctx_last_skipped(ldpc_ctx *ctx, int *kernel);
/* Early termination of the last decode on coop3 (kernel 8): the iterations of
 * its first stage when it ran staged (batches >= LDPC_COOP3_ET_STAGE_MIN, default
 * 8192 codewords: the codewords still decoding compacted every
 * LDPC_COOP3_ET_STEP iterations), 0 when it ran as one launch. */
int ldpc_ctx_last_et_stage(ldpc_ctx *ctx, int *first_stage_iters);
/* Launch shape of the last decode on the LDS-resident kernel (7): lanes per
 * codeword (64 / codewords per wave; it grows at small batches, which spread
 * over more waves) and whether two lanes shared a check (split = 1); 0 / 0
 * when the last decode ran another kernel.  (Introspection for tests.) */
int ldpc_ctx_last_lds_shape(ldpc_ctx *ctx, int *lanes_per_codeword, int *split);
/* The edge-parallel float kernel spread over several waves (`ldsepw`, a second
 * kernel of LDPC_KERNEL_LDSEP; off by default).  LDPC_KERNEL_LDSEP proper puts
 * one wave on a codeword and holds at most 77 (layer, pass) slots of 8 checks,
 * which is 648x324 and 576x288.  `ldsepw` puts one workgroup of W = 2 or 4
 * waves on a codeword, V in the workgroup's LDS, the passes of a layer dealt to
 * the waves, one workgroup barrier per layer: it takes a table whose layer
 * plan (ldpc_code_layer_info) has 11 or 12 layers, check degree <= 8 and at
 * most 24 passes (11 layers) or 12 passes (12 layers) of 8 checks in its widest
 * layer, and that LDPC_KERNEL_LDSEP proper does not take -- 1944x972, 1248x624
 * and 2304x1152 among the shipped ones.  Same float contract as
 * LDPC_KERNEL_LDSEP: bit for bit the serial float decode of the LLRs with
 * every zero made +0.0.
 *
 * ldpc_code_ep_wide_info (no context, no GPU): *n_layers / *n_passes of the
 * plan, *waves_mask with bit W set for every W compiled for the table (0: the
 * table does not qualify; then layers and passes are 0 too), *waves_auto the
 * W the automatic choice launches at `batch`, 0 where the table does not
 * qualify or the rule -- fitted to measured times, DESIGN.md section 7 --
 * leaves that batch to the family it ran on before.  Any pointer may be NULL.
 *
 * ldpc_ctx_set_ep_wide(ctx, 1): a float min-sum decode (OMS / NMS / MS) of a
 * qualifying table then accepts ldpc_ctx_set_kernel(ctx, LDPC_KERNEL_LDSEP)
 * and runs `ldsepw`; LDPC_KERNEL_AUTO runs it where waves_auto != 0;
 * ldpc_ctx_last_kernel reports LDPC_KERNEL_LDSEP and ldpc_ctx_last_ep_waves
 * the W launched (0 after any launch that was not `ldsepw`).  The
 * environment variable LDPC_EPW_WAVES = 2 or 4 forces W whenever `ldsepw`
 * runs; a W outside the table's mask is LDPC_EUNSUPPORTED before any launch.
 * LDPC_ALGO_BP, the binary16 and the int8 decodes, and every table that does
 * not qualify are decided exactly as with the switch off, and with it off
 * every call behaves as if it did not exist.  Setting it is accepted on any
 * GPU context (it changes nothing for a table that does not qualify) and
 * LDPC_EUNSUPPORTED on a host context. */
int ldpc_code_ep_wide_info(const ldpc_code *h, int batch, int *n_layers, int *n_passes, int *waves_mask,
                           int *waves_auto);
int ldpc_ctx_set_ep_wide(ldpc_ctx *ctx, int enable);
int ldpc_ctx_get_ep_wide(ldpc_ctx *ctx, int *enable);
int ldpc_ctx_last_ep_waves(ldpc_ctx *ctx, int *waves);
/* The edge-parallel kernel in int8 (`ldsepi`, the int8 element type of
 * LDPC_KERNEL_LDSEP; off by default).  It takes the tables LDPC_KERNEL_LDSEP
 * proper takes (802.11n 648x324, 576x288 and tables of their shape), two
 * codewords per lane as 16-bit halves, one wave per pair, and computes the
 * reference's fixed-point decode bit for bit: hard decisions, int8 soft output
 * and iters_used equal those of LDPC_KERNEL_LDS and of the host decoder.
 *
 * Its parameter domain is what ldpc_ldsepi_params_ok reports (no context, no
 * GPU): OMS / NMS / MS, var_max 127, var_min in -127 .. 0, msg_max in
 * 0 .. 127, offset in 0 .. 255, every NMS factor, early termination on or off.
 * var_min = -128 is outside it (the var range +-127 that LDPC_KERNEL_COOP and
 * LDPC_KERNEL_COOP3 also keep to).
 *
 * ldpc_ctx_set_i8_edge_parallel(ctx, 1): LDPC_EUNSUPPORTED, with the setting
 * left as it was, on a host context and on a code for which
 * ldpc_ctx_set_kernel(ctx, LDPC_KERNEL_LDSEP) fails with ldpc_ctx_set_ep_wide
 * off (200x100, the DVB-S2 codes, 1944x972 whatever ldpc_ctx_set_ep_wide says).
 * With it on, an int8 decode (device or host buffers, frame- or node-major) is
 * decided as follows:
 *   LDPC_KERNEL_AUTO, parameters inside   LDPC_KERNEL_LDSEP, checked first as for
 *                                         float32: last_kernel LDPC_KERNEL_LDSEP,
 *                                         last_skipped 0, last_lds_shape 0 / 0,
 *                                         last_ep_waves 0;
 *   LDPC_KERNEL_AUTO, parameters outside  the choice with the switch off
 *                                         (LDPC_KERNEL_LDS); last_skipped names
 *                                         LDPC_KERNEL_LDSEP;
 *   forced 9, parameters inside           `ldsepi`;
 *   forced 9, parameters outside          LDPC_EUNSUPPORTED, "not applicable";
 *   every other forced family, float32, binary16, LDPC_ALGO_BP and the mixed
 *   decoder                               as with the switch off.
 * The decode allocates no scratch (node-major input: the transpose buffer
 * LDPC_KERNEL_LDS uses).  The switch is independent of ldpc_ctx_set_ep_wide,
 * ldpc_ctx_set_f16_edge_parallel and ldpc_ctx_set_f16_all_codes, and with it
 * off every call behaves as if it did not exist: a forced 9 of an int8 decode
 * is LDPC_EUNSUPPORTED as before. */
int ldpc_ctx_set_i8_edge_parallel(ldpc_ctx *ctx, int enable);
int ldpc_ctx_get_i8_edge_parallel(ldpc_ctx *ctx, int *enable);
int ldpc_ldsepi_params_ok(const ldpc_params *p, int *ok);
/* The int8 edge-parallel kernel spread over several waves (`ldsepwi`, the int8
 * element type of `ldsepw`; off by default).  It takes the tables `ldsepw`
 * takes (1944x972, 1248x624, 2304x1152 and tables of their shape): one
 * workgroup of W = 2 or 4 waves decodes one pair of codewords, each lane
 * holding the two as 16-bit halves, and computes the reference's fixed-point
 * decode bit for bit, as `ldsepi` does: hard decisions, int8 soft output and
 * iters_used equal those of LDPC_KERNEL_LDS and of the host decoder.  Its
 * parameter domain is ldpc_ldsepi_params_ok's (var_min = -128 is outside).
 *
 * ldpc_code_i8_ep_wide_info (no context, no GPU): as ldpc_code_ep_wide_info,
 * with *waves_mask the W compiled for the table in int8 and *waves_auto the W
 * the int8 rule launches at `batch`, 0 where the table does not qualify or the
 * rule -- fitted to measured times, DESIGN.md section 7 -- leaves that batch
 * to LDPC_KERNEL_LDS.
 *
 * ldpc_ctx_set_i8_ep_wide(ctx, 1): LDPC_EUNSUPPORTED, with the setting left as
 * it was, on a host context and on a code without a several-wave plan
 * (648x324, 200x100, the DVB-S2 codes).  With it on,
 * ldpc_ctx_set_kernel(ctx, LDPC_KERNEL_LDSEP) is accepted on the code, and an
 * int8 decode (device or host buffers, frame- or node-major, with or without
 * the error counter) is decided as follows:
 *   LDPC_KERNEL_AUTO, parameters inside,  LDPC_KERNEL_LDSEP: last_kernel
 *   waves_auto != 0 at this batch         LDPC_KERNEL_LDSEP, last_skipped 0,
 *                                         last_lds_shape 0 / 0, last_ep_waves W;
 *   LDPC_KERNEL_AUTO, parameters outside  the choice with the switch off;
 *                                         last_skipped names LDPC_KERNEL_LDSEP;
 *   LDPC_KERNEL_AUTO, waves_auto == 0     the choice with the switch off;
 *   forced 9, parameters inside           `ldsepwi`, whatever the rule says;
 *   forced 9, parameters outside          LDPC_EUNSUPPORTED, "not applicable";
 *   every other forced family, float32 (a float decode forced to 9 with only
 *   this switch on stays "not applicable"), binary16, LDPC_ALGO_BP and the
 *   mixed decoder                         as with the switch off.
 * LDPC_EPW_WAVES = 2 or 4 forces W as for `ldsepw`; a W outside the int8 mask
 * is LDPC_EUNSUPPORTED before any launch.  The decode allocates no scratch
 * (node-major input: the transpose buffer LDPC_KERNEL_LDS uses).  The switch
 * is independent of ldpc_ctx_set_ep_wide, ldpc_ctx_set_i8_edge_parallel,
 * ldpc_ctx_set_f16_edge_parallel and ldpc_ctx_set_f16_all_codes, and with it
 * off every call behaves as if it did not exist. */
int ldpc_code_i8_ep_wide_info(const ldpc_code *h, int batch, int *n_layers, int *n_passes, int *waves_mask,
                              int *waves_auto);
int ldpc_ctx_set_i8_ep_wide(ldpc_ctx *ctx, int enable);
int ldpc_ctx_get_i8_ep_wide(ldpc_ctx *ctx, int *enable);
/* Kernel timing (bench / profiling): when enabled, every decode records HIP
 * events around the decode kernel on the stream it is launched on;
 * ldpc_ctx_kernel_time returns the summed kernel time and launch count since
 * the last reset (it waits for the recorded events). */
int ldpc_ctx_profile(ldpc_ctx *ctx, int enable);
int ldpc_ctx_kernel_time(ldpc_ctx *ctx, double *total_ms, int *launches, int reset);

/* Host buffers, synchronous, frame-major [batch][N]; hard = (V > 0).
 * A large batch (>= 64 MB of LLRs) is decoded in chunks (LDPC_HOST_CHUNKS,
 * default 2, >= 256 codewords each) on the context's copy/decode lanes, so
 * the PCIe copies of one chunk overlap the decode of the other (decode_stream's streams,
 * code/gpu_fixed/decoder_ms/CGPU_Decoder_MS_SIMD.cu:219-275).  With buffers
 * from ldpc_host_alloc the copies are asynchronous DMA. */
int ldpc_decode_i8(ldpc_ctx *ctx, const int8_t *llr, uint8_t *hard, int batch, int n_iter,
                   const ldpc_params *p);
int ldpc_decode_f32(ldpc_ctx *ctx, const float *llr, uint8_t *hard, int batch, int n_iter,
                    const ldpc_params *p);
/* ldpc_decode_f32 on a host context (device -1) with the two further outputs
 * of the device entry points: soft [batch][N], the final V per bit, and
 * iters_used [batch] (either may be NULL).  It is what the GPU kernels' soft
 * output and iteration counts are compared to, bit for bit, without a GPU in
 * the reference.  A GPU context is LDPC_EUNSUPPORTED: ldpc_decode_f32_async
 * returns both there.  (Replaces no reference interface.) */
int ldpc_decode_f32_soft(ldpc_ctx *ctx, const float *llr, uint8_t *hard, float *soft, int32_t *iters_used,
                         int batch, int n_iter, const ldpc_params *p);

/* Host buffers, asynchronous: enqueue H2D(llr) -> decode -> D2H(hard) on
 * hip_stream (NULL: the null stream) and return -- the reference's "W streams
 * x F frames in flight" model (paper/ldpcGpuTegra.tex:279-289;
 * CGPU_Decoder_MS_SIMD::decode_stream, code/gpu_fixed/decoder_ms/
 * CGPU_Decoder_MS_SIMD.cu:219-275, without its blocking copies).  llr / hard
 * should be page-locked (ldpc_host_alloc): pageable buffers make the copies
 * synchronous.  The context's device staging and scratch are reused by its
 * next call: each call records an event of the context's own after its D2H
 * copy, and the next call's stream waits for that event before reusing them
 * (so calls on one context may use different streams, but they serialise);
 * two contexts keep two batches in flight (H2D of batch k+1 and D2H of batch
 * k-1 under the decode of batch k).  ldpc_ctx_synchronize (and
 * ldpc_ctx_destroy) wait on that event, never on the caller's stream; hard is
 * valid after it. */
int ldpc_decode_i8_host_async(ldpc_ctx *ctx, void *hip_stream, const int8_t *llr, uint8_t *hard, int batch,
                              int n_iter, const ldpc_params *p);
int ldpc_decode_f32_host_async(ldpc_ctx *ctx, void *hip_stream, const float *llr, uint8_t *hard, int batch,
                               int n_iter, const ldpc_params *p);
int ldpc_ctx_synchronize(ldpc_ctx *ctx);

/* Page-locked host memory for the host-buffer API, replacing the
 * reference's CUDA_MALLOC_HOST (code/gpu_fixed/custom_api/custom_cuda.cu:33). */
int ldpc_host_alloc(void **ptr, size_t bytes);
void ldpc_host_free(void *ptr);

/* Device buffers, asynchronous on `hip_stream`.  NULL means HIP's null
 * stream, i.e. the legacy default stream, ordered with all blocking streams
 * (the reference's decode_stream callers, code/gpu_fixed/test.cpp:347-393, and
 * torch's default stream); the context's own non-blocking stream
 * (ldpc_ctx_stream) is used only when passed explicitly.
 * soft (optional): final V per bit; iters_used (optional): per codeword.
 *
 * Buffer contract of every device-pointer entry point (decode, mixed decode,
 * channel, quantiser, bit source, encoders, error count):
 *  - a device buffer needs only the natural alignment of its element type:
 *    1 byte for int8 / uint8, 2 for binary16, 4 for float / int32, 8 for the
 *    error counters.
 *    A contiguous slice of a larger allocation is a valid argument; wider
 *    alignment (16 bytes) only selects faster load / store paths, never
 *    another result;
 *  - outputs are [batch][N] (iters_used: [batch]): rows beyond `batch` and
 *    bytes outside that range are never written, whatever group size the
 *    kernel works in; batch 0 writes nothing;
 *  - node-major input: columns batch .. ld-1 of a row are never read as data
 *    (they may hold anything). */
int ldpc_decode_i8_async(ldpc_ctx *ctx, void *hip_stream, const int8_t *d_llr, uint8_t *d_hard,
                         int8_t *d_soft, int32_t *d_iters_used, int batch, int n_iter,
                         const ldpc_params *p);
int ldpc_decode_f32_async(ldpc_ctx *ctx, void *hip_stream, const float *d_llr, uint8_t *d_hard,
                          float *d_soft, int32_t *d_iters_used, int batch, int n_iter,
                          const ldpc_params *p);
/* Node-major device input: the LLR of bit i of codeword b at d_llr[i * ld + b]
 * (ld >= batch), the interleaved layout the reference's kernels run on
 * (Interleaver_uint8, code/gpu_fixed/transpose/GPU_Transpose_uint8.cu:80-130)
 * and that CGPU_Decoder_MS_SIMD_v2::decode takes from its caller
 * (code/gpu_fixed/decoder_oms_v2/CGPU_Decoder_MS_SIMD_v2.cu:120-251).  Same
 * results as ldpc_decode_i8_async on the transposed input; d_hard / d_soft
 * are frame-major [batch][N], as that decoder returns them. */
int ldpc_decode_i8_nm_async(ldpc_ctx *ctx, void *hip_stream, const int8_t *d_llr, size_t ld, uint8_t *d_hard,
                            int8_t *d_soft, int32_t *d_iters_used, int batch, int n_iter,
                            const ldpc_params *p);

/* out[i] = a[i] [+] b[i], the box-plus of LDPC_ALGO_BP alone (csrc/bp_math.h):
 * the only way to look at it outside a decode.  _host runs on the CPU and
 * needs no context; _async on the device of a GPU context, asynchronous on
 * hip_stream (NULL: the null stream), device buffers of `count` floats, bit for
 * bit the host's results.  count = 0 is LDPC_OK and touches nothing (the
 * pointers may then be NULL, as for the quantiser), a NULL pointer with
 * count > 0 or a negative count LDPC_EINVAL, a host context LDPC_EUNSUPPORTED
 * for _async.  Finite inputs only.  (Introspection for tests; replaces no
 * reference interface.) */
int ldpc_boxplus_f32_host(const float *a, const float *b, float *out, long count);
int ldpc_boxplus_f32_async(ldpc_ctx *ctx, void *hip_stream, const float *d_a, const float *d_b, float *d_out,
                           long count);

/* ---- binary16 ("f16") decode --------------------------------------------- */
/* Layered min-sum in IEEE binary16, between the int8 and the float32 decode:
 * half the bytes of float32 per LLR, per V and per message.  binary16 values
 * travel as uint16_t bit patterns.  The half contract defines
 * the results bit for bit: every + - x rounded to nearest even to binary16,
 * min / max / abs exact, subnormals kept; V saturates at +-1024 (on load and
 * after every update, +-inf included), the messages a check sends at 256; the
 * sign of a contribution is its sign bit (-0.0 counts as negative); the hard
 * decision V > 0 is a comparison (+-0 give 0).  NaN input is outside the
 * contract.  Parameters: algo OMS / NMS / MS with beta (rounded to binary16)
 * and early_term; LDPC_ALGO_BP is LDPC_EUNSUPPORTED; a beta that is negative,
 * not finite or rounds to binary16 infinity is LDPC_EINVAL (MS ignores beta);
 * the int8 fields are ignored.
 *
 * ldpc_decode_f16_async: device buffers, the conventions and buffer contract
 * of ldpc_decode_f32_async with 2-byte element alignment; rows beyond `batch`
 * are never written although the kernel packs codewords in pairs.  On the GPU
 * it decodes the staircase codes (every DVB-S2 table and the shaped ones) on
 * the packed half-precision element type of LDPC_KERNEL_STAIRF, which
 * ldpc_ctx_last_kernel then reports: two codewords per lane as one 32-bit
 * pair.  Any other code is LDPC_EUNSUPPORTED on a GPU context, and so are a
 * family other than AUTO / LDPC_KERNEL_STAIRF forced by ldpc_ctx_set_kernel
 * and a batch beyond the kernel's 32-bit V offsets, (n + 1) * stride * 2 <
 * 2^32 with stride = batch rounded up to 64 (33088 codewords at n = 64800,
 * twice float32's limit).  LDPC_STAIRF_S forces the group width as for float32.
 *
 * ldpc_ctx_set_f16_all_codes(ctx, 1) (off by default; ldpc_ctx_get_f16_all_codes
 * reads it back; both work on GPU and host contexts, and a host context
 * decodes every code either way) opens the GPU decode to every code, on two
 * more kernels of the same contract and the same two-codewords-per-lane
 * packing.  With the switch on:
 *   LDPC_KERNEL_AUTO  a staircase code runs on LDPC_KERNEL_STAIRF as before; any
 *                     other code on LDPC_KERNEL_LDS where the float32 decode
 *                     would prefer it (the pairs' state fits LDS and the layers
 *                     are wide enough), else on LDPC_KERNEL_GENERIC;
 *   forced 7          the packed LDS-resident kernel (`ldsh`) where the state
 *                     fits LDS (lds_f32 of ldpc_code_layer_info), else
 *                     LDPC_EUNSUPPORTED;
 *   forced 1          the packed any-H kernel (`generich`), on any code;
 *   forced 11         as with the switch off;
 *   any other family  LDPC_EUNSUPPORTED, "not applicable".
 * ldpc_ctx_last_kernel reports the family that ran, ldpc_ctx_last_skipped 0.
 * On LDPC_KERNEL_LDS ldpc_ctx_last_lds_shape reports lanes per PAIR of
 * codewords and two lanes per check or not; the environment variable
 * LDPC_LDSH_LANES (8, 16, 32 or 64) forces the lanes per pair, and a value the
 * code cannot run (fewer lanes than its widest layer needs, or a wave's pairs
 * passing 64 KB of LDS) is LDPC_EUNSUPPORTED before any launch.  With the switch
 * off every call behaves as if it did not exist.
 *
 * ldpc_ctx_set_f16_edge_parallel(ctx, 1) (off by default;
 * ldpc_ctx_get_f16_edge_parallel reads it back) is a second, independent
 * switch: it lets the binary16 decode run LDPC_KERNEL_LDSEP, the edge-parallel
 * kernel of the short quasi-cyclic codes (802.11n 648x324, 576x288 and tables
 * of their shape) in binary16 (`ldseph`: one wave per pair of codewords, one
 * lane per edge, the same contract, equal to the host decoder bit for bit, the
 * sign of zero soft values included).  Setting it is LDPC_EUNSUPPORTED, with
 * the setting left as it was, on a host context and on a code for which
 * ldpc_ctx_set_kernel(ctx, LDPC_KERNEL_LDSEP) fails.  With it on, where the
 * float32 decode could run LDPC_KERNEL_LDSEP (the pairs of a workgroup fit
 * LDS), LDPC_KERNEL_AUTO and a forced 9 run it -- it is checked first, as for
 * float32 -- and ldpc_ctx_last_kernel reports LDPC_KERNEL_LDSEP,
 * ldpc_ctx_last_skipped 0, ldpc_ctx_last_lds_shape 0 / 0; the decode allocates
 * nothing.  Every other setting is decided exactly as with this switch off,
 * whatever ldpc_ctx_set_f16_all_codes says.  With the switch off a forced 9 is
 * LDPC_EUNSUPPORTED as before.
 *
 * ldpc_decode_f16: host buffers, synchronous: copy in, decode, copy out on a
 * GPU context; the host decoder, which takes every code, on a device -1
 * context (last_kernel LDPC_KERNEL_HOST).
 * ldpc_decode_f16_soft: host context only, the twin of ldpc_decode_f32_soft:
 * the definition the kernel is compared with. */
int ldpc_decode_f16_async(ldpc_ctx *ctx, void *hip_stream, const uint16_t *d_llr, uint8_t *d_hard,
                          uint16_t *d_soft, int32_t *d_iters_used, int batch, int n_iter,
                          const ldpc_params *p);
int ldpc_decode_f16(ldpc_ctx *ctx, const uint16_t *llr, uint8_t *hard, int batch, int n_iter,
                    const ldpc_params *p);
int ldpc_decode_f16_soft(ldpc_ctx *ctx, const uint16_t *llr, uint8_t *hard, uint16_t *soft, int32_t *iters_used,
                         int batch, int n_iter, const ldpc_params *p);
int ldpc_ctx_set_f16_all_codes(ldpc_ctx *ctx, int enable);
int ldpc_ctx_get_f16_all_codes(ldpc_ctx *ctx, int *enable);
int ldpc_ctx_set_f16_edge_parallel(ldpc_ctx *ctx, int enable);
int ldpc_ctx_get_f16_edge_parallel(ldpc_ctx *ctx, int *enable);
/* float32 -> binary16 LLRs: h = RNE16(min(max(y, -1024), 1024)).  _host needs
 * no context; _async runs on the device of a GPU context (a host context is
 * LDPC_EUNSUPPORTED), bit for bit the host's results.  count = 0 touches
 * nothing; a NULL pointer with count > 0 or a negative count is LDPC_EINVAL. */
int ldpc_convert_f32_f16_host(const float *y, uint16_t *h, long count);
int ldpc_convert_f32_f16_async(ldpc_ctx *ctx, void *hip_stream, const float *d_y, uint16_t *d_h, long count);
/* The group width S (2, 4, 8 or 16 checks of 128 / S codewords per wave) the
 * binary16 kernel's rule picks at `stride` (the batch rounded up to 64) among
 * `widths` (bit S set: the code has that table; 0: none).  Introspection for
 * tools/f16_rate.py, which holds the rule against measured times. */
int ldpc_f16_staircase_width_rule(int stride, unsigned widths);
/* log2 of the lanes per pair (3 .. 6) the binary16 LDS-resident kernel's rule
 * picks for `pairs` pairs of codewords ((batch + 1) / 2) of a code with n
 * variables, e edges and max_width checks in its widest layer: a cost model
 * fitted to measured runs.  Introspection for
 * tools/f16_short_rate.py and the tests, which restate it. */
int ldpc_f16_lds_shape_rule(int n, int e, int max_width, int pairs);

/* ---- mixed-rate batches (BASELINE config 5) ---------------------------- */
/* A batch whose codewords use different codes of equal length N (e.g. the
 * DVB-S2 normal-frame rates).  One decoder context per code; a decode groups
 * the codewords by code id, runs the per-code decodes concurrently on their
 * own streams (forked from / joined back to the caller's stream) and writes
 * hard decisions (and iterations used) back in batch order.  The reference
 * has one compile-time code per binary (code/x86/Constantes/constantes_sse.h). */
typedef struct ldpc_mixed ldpc_mixed;
int ldpc_mixed_create(const ldpc_code *const *codes, int n_codes, int device, int max_batch, ldpc_mixed **out);
void ldpc_mixed_destroy(ldpc_mixed *mx);
/* code_id: HOST array [batch] of indices into `codes`; d_llr/d_hard [batch][N]. */
int ldpc_decode_i8_mixed_async(ldpc_mixed *mx, void *hip_stream, const int8_t *d_llr, uint8_t *d_hard,
                               int32_t *d_iters_used, const int32_t *code_id, int batch, int n_iter,
                               const ldpc_params *p);
/* Kernel family the last mixed decode ran for code `code_index` (numbering of
 * ldpc_ctx_last_kernel; 0 if that code had no codewords in any decode yet). */
int ldpc_mixed_last_kernel(ldpc_mixed *mx, int code_index, int *kernel);
/* ldpc_ctx_last_et_stage of code `code_index`'s context. */
int ldpc_mixed_last_et_stage(ldpc_mixed *mx, int code_index, int *first_stage_iters);
/* Per-code decode-kernel timing (ldpc_ctx_profile / ldpc_ctx_kernel_time of
 * the code's context): the decode launches only, not the gather / scatter. */
int ldpc_mixed_profile(ldpc_mixed *mx, int enable);
int ldpc_mixed_kernel_time(ldpc_mixed *mx, int code_index, double *total_ms, int *launches, int reset);

/* DVB-S2 IRA encoder (codes built from an Annex-B table), as the
 * reference's GenericEncoder::encode (code/x86/CEncoder/GenericEncoder.cpp:38-78):
 * info [batch][K] 0/1 -> codeword [batch][N] = [info, parity]. */
int ldpc_dvbs2_encode(const ldpc_code *h, const uint8_t *info, uint8_t *codeword, int batch);
/* Device twin of ldpc_dvbs2_encode, asynchronous on hip_stream (NULL: the null
 * stream): d_info [batch][K] -> d_codeword [batch][N] = [info & 1, parity],
 * byte-equal to the host encoder.  One workgroup per codeword, the codeword
 * held in LDS: no scratch, no allocation, no synchronisation, and batch is not
 * limited by the context's max_batch.  d_info and d_codeword must not overlap.
 * LDPC_EUNSUPPORTED for a code not built from an Annex-B table, or one whose
 * N bytes do not fit a workgroup's 64 KiB of LDS. */
int ldpc_dvbs2_encode_async(ldpc_ctx *ctx, void *hip_stream, const uint8_t *d_info,
                            uint8_t *d_codeword, int batch);

/* ---- general encoder ---------------------------------------------------- */
/* An encoder for any ldpc_code (the reference has none for codes that are not
 * IRA).  ldpc_encoder_create reduces H over GF(2), bit-packed; the result is
 * canonical, whatever the order of elimination:
 *   parity positions: scanning columns N-1 .. 0, a column is a parity position
 *     iff it is linearly independent of the parity columns chosen before it;
 *     their count is rank (<= M);
 *   information positions: the K = N - M lowest remaining columns, ascending;
 *   forced zeros: the other M - rank remaining columns (only when rank < M);
 *   systematic = 1 iff the information positions are 0 .. K-1: the codeword
 *     is then [info, parity], the layout of ldpc_dvbs2_encode;
 *   the parity bits are the unique solution of H x = 0 given the others.
 * A code built from an Annex-B table has its staircase columns K .. N-1 as
 * parity positions: no elimination, ldpc_encode / ldpc_encode_async run the
 * IRA encoders above and are byte-equal to them.  For any other code the
 * dense M x N bit matrix (M * ceil(N / 64) * 8 bytes) must fit 64 MiB, else
 * LDPC_EUNSUPPORTED -- every shipped table does (20000x10000: 25 MB; its
 * elimination takes seconds).
 * The encoder is immutable and may be shared by contexts and threads; the code
 * it was built from must outlive it. */
typedef struct ldpc_encoder ldpc_encoder;
int ldpc_encoder_create(const ldpc_code *h, ldpc_encoder **out);
void ldpc_encoder_destroy(ldpc_encoder *e);
/* any of n, k, rank, systematic may be NULL */
int ldpc_encoder_info(const ldpc_encoder *e, int *n, int *k, int *rank, int *systematic);
/* info_pos [k], parity_pos [rank], ascending; either may be NULL */
int ldpc_encoder_positions(const ldpc_encoder *e, int32_t *info_pos, int32_t *parity_pos);
/* Host: info [batch][K] (info & 1 is taken) -> codeword [batch][N], every byte
 * written 0 / 1: codeword[info_pos[i]] = info[i], the parity bits at
 * parity_pos, 0 at the forced positions. */
int ldpc_encode(const ldpc_encoder *e, const uint8_t *info, uint8_t *codeword, int batch);
/* Attach an encoder of the context's code to a GPU context: uploads its
 * matrix (synchronous, allocates device memory; replaces an earlier one after
 * waiting for the device).  LDPC_EINVAL for an encoder of another code,
 * LDPC_EUNSUPPORTED for a host context. */
int ldpc_ctx_set_encoder(ldpc_ctx *ctx, const ldpc_encoder *e);
/* Device twin of ldpc_encode with the conventions of ldpc_dvbs2_encode_async:
 * asynchronous on hip_stream (NULL: the null stream), byte-equal to the host
 * encoder, no allocation, no synchronisation, batch not limited by max_batch,
 * batch = 0 is LDPC_OK, overlapping buffers LDPC_EINVAL, a host context
 * LDPC_EUNSUPPORTED, a context without an attached encoder LDPC_EINVAL. */
int ldpc_encode_async(ldpc_ctx *ctx, void *hip_stream, const uint8_t *d_info, uint8_t *d_codeword, int batch);

/* ---- bit source ----------------------------------------------------------- */
/* info[b][i] = bit 63 of splitmix64(((first_cw + b) * K + i) ^ (seed * 0xA0761D6478BD642FULL)),
 * the splitmix64 of the channel below under another key multiplier, so the
 * bits and the noise of one seed are separate streams.  Indexed per codeword
 * like the channel: any shard, any first_cw draws the same bits.
 * _async: K = n - m of ctx's code, device buffer [batch][K]. */
int ldpc_info_bits_host (int k, int batch, uint64_t first_cw, uint64_t seed, uint8_t *info);
int ldpc_info_bits_async(ldpc_ctx *ctx, void *hip_stream, uint8_t *d_info, int batch,
                         uint64_t first_cw, uint64_t seed);

/* ---- synthetic channel -------------------------------------------------- */
/* sigma = sqrt(10^(-(EbN0 + 10 log10(rate))/10) / 2)  (CChanelAWGN_MKL.cpp:102-105) */
double ldpc_awgn_sigma(double ebn0_db, double rate);
/* the same with the reference's es_n0 option (:97-104): es_n0 != 0 reads
 * snr_db as Es/N0 of a 2-bit (QPSK) symbol, Eb/N0 = Es/N0 - 10 log10(2 rate) */
double ldpc_awgn_sigma_ex(double snr_db, double rate, int es_n0);
/* Threshold table (63 entries) for the integer-exact quantised AWGN generator:
 * q = clamp(trunc(factor*y), -sat, sat), y = -1 + sigma*z (bit 0). */
int ldpc_awgn_i8_table(double sigma, int factor, int sat, uint32_t *table /*[64]*/);
/* General channel of CChanelAWGN_MKL::generate (:127-143): y = +-amp + sigma*z
 * (amp 1 for BPSK, 0.707106781 for QPSK, one bit per real dimension) scaled by
 * norm (1, or 2 / sigma^2 with the reference's normalize option, :114-121),
 * then q = clamp(trunc(factor * y), -sat, sat); the same generators
 * (ldpc_awgn_i8_host / _async) draw from it. */
int ldpc_awgn_i8_table_ex(double sigma, double amp, double norm, int factor, int sat, uint32_t *table /*[64]*/);
/* llr[b][i] for codewords first_cw .. first_cw+batch-1; codeword bits
 * (0/1, [batch][N]) or NULL for the all-zero codeword. */
int ldpc_awgn_i8_host(int n, int batch, uint64_t first_cw, uint64_t seed, const uint32_t *table,
                      const uint8_t *codeword, int8_t *llr);
int ldpc_awgn_i8_async(ldpc_ctx *ctx, void *hip_stream, int8_t *d_llr, int batch,
                       uint64_t first_cw, uint64_t seed, const uint32_t *table,
                       const uint8_t *d_codeword);
/* The float channel, replacing CChanelAWGN_MKL::generate
 * (code/x86/CChanel/CChanelAWGN_MKL.cpp:127-143): the unquantised form of the
 * noise the int8 channel draws.  For element i of codeword first_cw + b:
 *   u = splitmix64(((first_cw + b) * N + i) ^ (seed * 0xD1B54A32D192ED03)) >> 32
 *   z = Phi^-1((u + 0.5) * 2^-32)            (double; |z| <= 6.34: 32 bits of u
 *                                             cut off 2^-32 of the mass)
 *   y = (float)(norm * (-amp + sigma * z)),  negated where the codeword bit is 1
 * with sigma, amp and norm as in ldpc_awgn_i8_table_ex (all > 0).  Host and
 * device give the same bits.  u is the int8 channel's for the same (seed,
 * first_cw), so ldpc_quantize_f32_i8(y, factor, -sat, sat) reproduces
 * ldpc_awgn_i8_* except at the edges of a quantisation cell (about 2e-6 of
 * the samples), and float and int8 decoders can be compared on paired noise.
 * y is [batch][N] floats, 4-byte aligned; codeword bits (0/1, [batch][N]) or
 * NULL for the all-zero codeword.  LDPC_EINVAL for a NULL y, a negative batch
 * or a non-positive sigma, amp or norm; batch 0 writes nothing. */
int ldpc_awgn_f32_host(int n, int batch, uint64_t first_cw, uint64_t seed, double sigma, double amp, double norm,
                       const uint8_t *codeword, float *y);
int ldpc_awgn_f32_async(ldpc_ctx *ctx, void *hip_stream, float *d_y, int batch, uint64_t first_cw, uint64_t seed,
                        double sigma, double amp, double norm, const uint8_t *d_codeword);
/* float -> int8 LLR conversion, replacing CFastFixConversion::generate
 * (code/x86/CFixPointConversion/CFastFixConversion.cpp:55-65) and the GPU
 * converter (code/gpu_fixed/decoder_template/GPU_Scheduled_functions.cu:54-62):
 *   q[i] = clamp((int)((float)factor * y[i]), sat_neg, sat_pos)
 * (int) truncates toward zero; NaN and |product| >= 2^31 give sat_neg, as
 * x86 cvttss2si does.  factor >= 1, -128 <= sat_neg <= sat_pos <= 127
 * (the reference runs factor 8, saturation -31 / +31).
 * _async: device buffers on hip_stream; the plain form: host buffers,
 * synchronous, on the context's stream. */
int ldpc_quantize_f32_i8_async(ldpc_ctx *ctx, void *hip_stream, const float *d_y, int8_t *d_q, long count,
                               int factor, int sat_neg, int sat_pos);
int ldpc_quantize_f32_i8(ldpc_ctx *ctx, const float *y, int8_t *q, long count, int factor, int sat_neg,
                         int sat_pos);
/* Count bit errors over the first k positions of each codeword vs d_ref
 * (NULL = all-zero); d_counts[0] += bit errors, d_counts[1] += frame errors.
 * A position is an error when bit 0 of d_hard and bit 0 of d_ref differ: the
 * other bits of a d_ref byte are ignored, as the encoders take info & 1 (the
 * same holds for the counting decodes below). */
int ldpc_count_errors_async(ldpc_ctx *ctx, void *hip_stream, const uint8_t *d_hard, int batch,
                           int k, const uint8_t *d_ref, unsigned long long *d_counts);
/* Decode and count in one call: ldpc_decode_*_async followed by
 * ldpc_count_errors_async over d_hard (required) -- the reference's
 * decode + CErrorAnalyzer::generate pair (code/x86/main_p.cpp:511-540,
 * CErrorAnalyzer.cpp:123-154).  The edge-parallel float kernel (9) counts in
 * its own epilogue (no second launch); the others launch the count after. */
int ldpc_decode_i8_count_async(ldpc_ctx *ctx, void *hip_stream, const int8_t *d_llr, uint8_t *d_hard,
                               int8_t *d_soft, int32_t *d_iters_used, int batch, int n_iter, const ldpc_params *p,
                               int k, const uint8_t *d_ref, unsigned long long *d_counts);
int ldpc_decode_f32_count_async(ldpc_ctx *ctx, void *hip_stream, const float *d_llr, uint8_t *d_hard,
                                float *d_soft, int32_t *d_iters_used, int batch, int n_iter, const ldpc_params *p,
                                int k, const uint8_t *d_ref, unsigned long long *d_counts);

#ifdef __cplusplus
}
#endif
#endif /* LDPC_MI355X_H */
