// ldpc_sim.cpp -- native Monte-Carlo BER/FER driver over the C-ABI.
//
// The caller side of the boundary, re-designed from the reference's simulator
// loop (code/x86/main_p.cpp:404-656: SNR sweep, frame-error limit, per-SNR
// report line of code/x86/CTerminal/CTerminal.cpp:78-90, error counting of
// code/x86/CErrorAnalyzer/CErrorAnalyzer.cpp:123-194).  Differences by
// design: the channel runs on the GPU (integer-exact generator), one host
// thread drives each GPU with batches of thousands of codewords, and the
// output is one text line plus one JSON line per SNR.
//
//   ldpc_sim -code dvbs2_r1_2 -min 0.8 -max 1.2 -pas 0.1 -iter 50 -fer 100
//            [-batch 4096] [-frames 1000000] [-OMS 1 | -NMS 29 | -MS]
//            [-encoder [-fresh] | -gencoder [-fresh]] [-et] [-gpus N] [-seed S]
//            [-kernel K] [-f32 [-beta B] [-epwide] | -f32q | -BP [-bpstair] | -f16 [-f16all] [-f16ep] [-beta B]]
//            [-i8ep] [-i8epw]
//
// Three chains see the same noise (one u per element, the same first_cw and
// seed scheme): the default draws the quantised int8 LLRs directly
// (ldpc_awgn_i8_async -> int8 decode); -f32 draws float samples
// (ldpc_awgn_f32_async, in place of CChanelAWGN_MKL::generate) and runs the
// float decoders with the fused error count (ldpc_decode_f32_count_async;
// -beta B is the float OMS offset or NMS factor, -OMS / -NMS / -MS choose the
// algorithm, their int8 value is not used); -f32q is the reference's chain
// stage by stage: float channel -> ldpc_quantize_f32_i8_async (8, +-31) -> the
// int8 decode.  The JSON line names the chain ("i8", "f32", "f32q") and the
// algorithm.  -BP is the f32 chain with belief propagation (LDPC_ALGO_BP): the
// yardstick curve of the three min-sum algorithms.  BP is not scale-invariant,
// so its channel is drawn with norm = 2 / sigma^2 (true LLRs) where the other
// -f32 runs keep 1.0; there is no int8 BP, so -BP with -f32q is a usage error.
// -bpstair (with -BP only) lets BP run on the staircase kernel of the DVB-S2
// codes (ldpc_ctx_set_bp_staircase): the same counts, many times the frames per
// second; the JSON line names it ("bp_staircase").  -f16 is the binary16 chain:
// float channel -> ldpc_convert_f32_f16_async -> ldpc_decode_f16_async -> error
// count, with -beta / -OMS / -NMS / -MS / -et as for -f32 (chain "f16"); a usage
// error together with -f32, -f32q or -BP.  On its own -f16 takes the staircase
// codes (DVB-S2 and like-shaped tables); -f16all (with -f16 only) opens it to
// every code (ldpc_ctx_set_f16_all_codes: the packed LDS-resident and any-H
// kernels, -kernel 7 / 1 force them); the JSON line names it ("f16_all_codes").
// -f16ep (with -f16 only, freely with -f16all) lets the short QC codes run on the
// edge-parallel binary16 kernel (ldpc_ctx_set_f16_edge_parallel, -kernel 9
// forces it); the JSON line names it ("f16_edge_parallel").
// -epwide (with -f32 only) lets the float min-sum decode of the longer QC codes
// (1944x972, 1248x624, 2304x1152) run on the edge-parallel kernel spread over
// several waves (ldpc_ctx_set_ep_wide, -kernel 9 forces it); the JSON line names
// it ("ep_wide").
// -i8ep (on the default int8 chain and with -f32q; a usage error with -f32, -f16
// or -BP) lets the int8 decode of the short QC codes run on the edge-parallel int8
// kernel (ldpc_ctx_set_i8_edge_parallel, -kernel 9 forces it); the JSON line names
// it ("i8_edge_parallel").
// -i8epw (on the same chains, the same usage errors) lets the int8 decode of the
// longer QC codes (1944x972, 1248x624, 2304x1152) run on the edge-parallel int8
// kernel spread over several waves (ldpc_ctx_set_i8_ep_wide, -kernel 9 forces it);
// the JSON line names it ("i8_ep_wide").
//
// -encoder alone draws 64 codewords once on the host and replicates them over
// every batch; -encoder -fresh draws new information bits and encodes them on
// the GPU for every frame, as the reference's chain does per frame
// (code/x86/main_p.cpp:431-445, 490-498).  -encoder is the DVB-S2 IRA encoder
// (Annex-B codes only); -gencoder does the same through the general encoder
// (ldpc_encoder_create / ldpc_encode / ldpc_encode_async), so it takes any
// code.  Errors are counted over the first K codeword positions either way:
// the information bits of a systematic code; for a code whose encoder is not
// systematic (ldpc_encoder_info) they are K code bits, some of them parity.
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <thread>
#include <vector>

#include <hip/hip_runtime.h>

#include "../../include/ldpc_mi355x.h"

namespace {

struct Opt {
    std::string code = "dvbs2_r1_2";
    double min = 0.5, max = 3.0, pas = 0.1;
    int iter = 30, fer = 100, batch = 4096, gpus = 1, kernel = LDPC_KERNEL_AUTO;
    long frames = 1 << 20;
    bool encoder = false, gencoder = false, fresh = false, f32 = false, f32q = false, bp = false, bpstair = false;
    bool f16 = false, f16all = false, f16ep = false, epwide = false, i8ep = false, i8epw = false;
    ldpc_params p{};
    uint64_t seed = 1;
};

#define CHECK(x)                                                                              \
    do {                                                                                      \
        int _r = (x);                                                                         \
        if (_r != LDPC_OK) {                                                                  \
            fprintf(stderr, "%s failed: %s (%s)\n", #x, ldpc_strerror(_r), ldpc_last_error()); \
            exit(1);                                                                          \
        }                                                                                     \
    } while (0)

std::string code_path(const std::string &name, const char *argv0)
{
    if (name.find('/') != std::string::npos) return name;
    std::string dir(argv0);
    dir = dir.substr(0, dir.rfind('/') + 1);   // .../ldpcgputegra_amd/bin/
    for (const char *ext : {".ldpc", ".txt"}) {
        std::string p = dir + "../codes/" + name + ext;
        if (FILE *f = fopen(p.c_str(), "rb")) {
            fclose(f);
            return p;
        }
    }
    return name;
}

struct Totals {
    std::atomic<long> frames{0}, fe{0}, be{0};
};

void worker(int dev, const ldpc_code *h, const Opt &o, double sigma, Totals &tot, int n, int k,
            const std::vector<uint8_t> &pool, int pool_n, const ldpc_encoder *genc)
{
    ldpc_ctx *ctx;
    CHECK(ldpc_ctx_create(h, dev, o.batch, &ctx));
    if (genc && o.fresh) CHECK(ldpc_ctx_set_encoder(ctx, genc));
    if (o.epwide) CHECK(ldpc_ctx_set_ep_wide(ctx, 1));   // first: -kernel 9 takes the longer QC codes only with it on
    if (o.i8epw) CHECK(ldpc_ctx_set_i8_ep_wide(ctx, 1));   // first, for the same reason
    if (o.kernel) CHECK(ldpc_ctx_set_kernel(ctx, o.kernel));
    if (o.bpstair) CHECK(ldpc_ctx_set_bp_staircase(ctx, 1));
    if (o.f16all) CHECK(ldpc_ctx_set_f16_all_codes(ctx, 1));
    if (o.f16ep) CHECK(ldpc_ctx_set_f16_edge_parallel(ctx, 1));
    if (o.i8ep) CHECK(ldpc_ctx_set_i8_edge_parallel(ctx, 1));
    void *stream;
    CHECK(ldpc_ctx_stream(ctx, &stream));
    uint32_t table[64];
    CHECK(ldpc_awgn_i8_table(sigma, 8, 31, table));
    int8_t *d_llr;
    float *d_y = nullptr;   // the float chains' channel output
    uint8_t *d_hard, *d_cw = nullptr;
    uint16_t *d_h = nullptr;   // the binary16 chain's LLRs
    unsigned long long *d_cnt;
    (void)hipSetDevice(dev);
    if (hipMalloc(&d_llr, (size_t)o.batch * n) || hipMalloc(&d_hard, (size_t)o.batch * n) ||
        hipMalloc(&d_cnt, 16) ||
        ((o.f32 || o.f32q || o.f16) && hipMalloc(&d_y, (size_t)o.batch * n * sizeof(float))) ||
        (o.f16 && hipMalloc(&d_h, (size_t)o.batch * n * sizeof(uint16_t)))) {
        fprintf(stderr, "hipMalloc failed\n");
        exit(1);
    }
    uint8_t *d_info = nullptr;
    if (o.fresh) {
        // bits and codewords are drawn on the device per batch: no pool, no upload
        if (hipMalloc(&d_info, (size_t)o.batch * k) || hipMalloc(&d_cw, (size_t)o.batch * n)) {
            fprintf(stderr, "hipMalloc failed\n");
            exit(1);
        }
    } else if (o.encoder || o.gencoder) {
        // the codeword pool replicated over the batch (noise differs per codeword)
        std::vector<uint8_t> rep((size_t)o.batch * n);
        for (int b = 0; b < o.batch; b++) memcpy(&rep[(size_t)b * n], &pool[(size_t)(b % pool_n) * n], n);
        if (hipMalloc(&d_cw, rep.size()) || hipMemcpy(d_cw, rep.data(), rep.size(), hipMemcpyHostToDevice)) {
            fprintf(stderr, "codeword upload failed\n");
            exit(1);
        }
    }
    for (long batch_no = dev;; batch_no += o.gpus) {
        if (tot.fe.load() >= o.fer || tot.frames.load() >= o.frames) break;
        const uint64_t first = (uint64_t)batch_no * o.batch;
        (void)hipMemsetAsync(d_cnt, 0, 16, (hipStream_t)stream);
        if (o.fresh) {
            CHECK(ldpc_info_bits_async(ctx, stream, d_info, o.batch, first, o.seed));
            if (genc) CHECK(ldpc_encode_async(ctx, stream, d_info, d_cw, o.batch));
            else CHECK(ldpc_dvbs2_encode_async(ctx, stream, d_info, d_cw, o.batch));
        }
        if (o.f32) {
            const double norm = o.p.algo == LDPC_ALGO_BP ? 2.0 / (sigma * sigma) : 1.0;
            CHECK(ldpc_awgn_f32_async(ctx, stream, d_y, o.batch, first, o.seed, sigma, 1.0, norm, d_cw));
            CHECK(ldpc_decode_f32_count_async(ctx, stream, d_y, d_hard, nullptr, nullptr, o.batch, o.iter, &o.p, k,
                                              d_cw, d_cnt));
        } else if (o.f16) {
            CHECK(ldpc_awgn_f32_async(ctx, stream, d_y, o.batch, first, o.seed, sigma, 1.0, 1.0, d_cw));
            CHECK(ldpc_convert_f32_f16_async(ctx, stream, d_y, d_h, (long)o.batch * n));
            CHECK(ldpc_decode_f16_async(ctx, stream, d_h, d_hard, nullptr, nullptr, o.batch, o.iter, &o.p));
            CHECK(ldpc_count_errors_async(ctx, stream, d_hard, o.batch, k, d_cw, d_cnt));
        } else {
            if (o.f32q) {
                CHECK(ldpc_awgn_f32_async(ctx, stream, d_y, o.batch, first, o.seed, sigma, 1.0, 1.0, d_cw));
                CHECK(ldpc_quantize_f32_i8_async(ctx, stream, d_y, d_llr, (long)o.batch * n, 8, -31, 31));
            } else {
                CHECK(ldpc_awgn_i8_async(ctx, stream, d_llr, o.batch, first, o.seed, table, d_cw));
            }
            CHECK(ldpc_decode_i8_async(ctx, stream, d_llr, d_hard, nullptr, nullptr, o.batch, o.iter, &o.p));
            CHECK(ldpc_count_errors_async(ctx, stream, d_hard, o.batch, k, d_cw, d_cnt));
        }
        unsigned long long c[2];
        if (hipMemcpyAsync(c, d_cnt, 16, hipMemcpyDeviceToHost, (hipStream_t)stream) != hipSuccess ||
            hipStreamSynchronize((hipStream_t)stream) != hipSuccess) {
            fprintf(stderr, "device error: %s\n", hipGetErrorString(hipGetLastError()));
            exit(1);
        }
        tot.be += (long)c[0];
        tot.fe += (long)c[1];
        tot.frames += o.batch;
    }
    (void)hipFree(d_llr);
    if (d_y) (void)hipFree(d_y);
    if (d_h) (void)hipFree(d_h);
    (void)hipFree(d_hard);
    (void)hipFree(d_cnt);
    if (d_cw) (void)hipFree(d_cw);
    if (d_info) (void)hipFree(d_info);
    ldpc_ctx_destroy(ctx);
}

}  // namespace

int main(int argc, char **argv)
{
    Opt o;
    ldpc_params_default(&o.p);
    for (int i = 1; i < argc; i++) {
        std::string a = argv[i];
        auto nxt = [&]() { return (i + 1 < argc) ? argv[++i] : (fprintf(stderr, "missing value\n"), exit(2), ""); };
        if (a == "-code") o.code = nxt();
        else if (a == "-min") o.min = atof(nxt());
        else if (a == "-max") o.max = atof(nxt());
        else if (a == "-pas") o.pas = atof(nxt());
        else if (a == "-iter") o.iter = atoi(nxt());
        else if (a == "-fer") o.fer = atoi(nxt());
        else if (a == "-frames") o.frames = atol(nxt());
        else if (a == "-batch") o.batch = atoi(nxt());
        else if (a == "-gpus") o.gpus = atoi(nxt());
        else if (a == "-kernel") o.kernel = atoi(nxt());
        else if (a == "-seed") o.seed = strtoull(nxt(), nullptr, 10);
        else if (a == "-OMS") { o.p.algo = LDPC_ALGO_OMS; o.p.offset = atoi(nxt()); }
        else if (a == "-NMS") { o.p.algo = LDPC_ALGO_NMS; o.p.factor = atoi(nxt()); }
        else if (a == "-MS") o.p.algo = LDPC_ALGO_MS;
        else if (a == "-BP") o.bp = true;
        else if (a == "-bpstair") o.bpstair = true;
        else if (a == "-encoder") o.encoder = true;
        else if (a == "-gencoder") o.gencoder = true;
        else if (a == "-fresh") o.fresh = true;
        else if (a == "-et") o.p.early_term = 1;
        else if (a == "-f32") o.f32 = true;
        else if (a == "-f32q") o.f32q = true;
        else if (a == "-f16") o.f16 = true;
        else if (a == "-f16all") o.f16all = true;
        else if (a == "-f16ep") o.f16ep = true;
        else if (a == "-epwide") o.epwide = true;
        else if (a == "-i8ep") o.i8ep = true;
        else if (a == "-i8epw") o.i8epw = true;
        else if (a == "-beta") o.p.beta = (float)atof(nxt());
        else {
            fprintf(stderr, "unknown option %s\n", a.c_str());
            return 2;
        }
    }
    if (o.encoder && o.gencoder) {
        fprintf(stderr, "usage: -encoder (DVB-S2 IRA encoder) and -gencoder (general encoder, any code) exclude "
                        "each other\n");
        return 2;
    }
    if (o.f32 && o.f32q) {
        fprintf(stderr, "usage: -f32 (float channel -> float decode) and -f32q (float channel -> quantise -> int8 "
                        "decode) exclude each other\n");
        return 2;
    }
    if (o.f16 && (o.f32 || o.f32q || o.bp)) {
        fprintf(stderr, "usage: -f16 (float channel -> binary16 conversion -> binary16 decode) excludes -f32, -f32q "
                        "and -BP\n");
        return 2;
    }
    if (o.f16all && !o.f16) {
        fprintf(stderr, "usage: -f16all (the binary16 decode on every code) needs -f16\n");
        return 2;
    }
    if (o.f16ep && !o.f16) {
        fprintf(stderr, "usage: -f16ep (the binary16 decode on the edge-parallel kernel) needs -f16\n");
        return 2;
    }
    if (o.epwide && (!o.f32 || o.bp)) {
        fprintf(stderr, "usage: -epwide (the float min-sum decode on the edge-parallel kernel over several waves) needs "
                        "-f32 and excludes -BP\n");
        return 2;
    }
    if (o.i8ep && (o.f32 || o.f16 || o.bp)) {
        fprintf(stderr, "usage: -i8ep (the int8 decode on the edge-parallel kernel) runs on the int8 chains (the "
                        "default and -f32q) and excludes %s\n", o.f32 ? "-f32" : o.f16 ? "-f16" : "-BP");
        return 2;
    }
    if (o.i8epw && (o.f32 || o.f16 || o.bp)) {
        fprintf(stderr, "usage: -i8epw (the int8 decode on the edge-parallel kernel over several waves) runs on the int8 "
                        "chains (the default and -f32q) and excludes %s\n", o.f32 ? "-f32" : o.f16 ? "-f16" : "-BP");
        return 2;
    }
    if (o.bp) {   // belief propagation: the float chain, whatever -OMS / -NMS / -MS said
        if (o.f32q) {
            fprintf(stderr, "usage: -BP (belief propagation) is a float decode: it runs the -f32 chain and excludes "
                            "-f32q and the int8 chain\n");
            return 2;
        }
        o.f32 = true;
        o.p.algo = LDPC_ALGO_BP;
    }
    if (o.bpstair && !o.bp) {
        fprintf(stderr, "usage: -bpstair (belief propagation on the staircase kernel) needs -BP\n");
        return 2;
    }
    if (o.fresh && !o.encoder && !o.gencoder) {
        fprintf(stderr, "usage: -fresh (new codewords every frame) needs -encoder\n");
        return 2;
    }
    ldpc_code *h;
    CHECK(ldpc_code_load(code_path(o.code, argv[0]).c_str(), &h));
    int n, m, e, ng, md;
    CHECK(ldpc_code_info(h, &n, &m, &e, &ng, &md));
    const int k = n - m;
    int ndev = 0;
    ldpc_device_count(&ndev);
    if (ndev < o.gpus) {
        fprintf(stderr, "need %d GPUs, %d visible\n", o.gpus, ndev);
        return 1;
    }
    std::vector<uint8_t> pool;
    int pool_n = 0;
    ldpc_encoder *genc = nullptr;
    if (o.gencoder) CHECK(ldpc_encoder_create(h, &genc));
    if (o.fresh) {
        // the library's verdict on the code, before any GPU work
        if (!genc) CHECK(ldpc_dvbs2_encode(h, nullptr, nullptr, 0));
    } else if (o.encoder || o.gencoder) {
        pool_n = 64;
        std::vector<uint8_t> info((size_t)pool_n * k);
        std::mt19937_64 rng(o.seed);
        for (auto &b : info) b = rng() & 1;
        pool.resize((size_t)pool_n * n);
        if (genc) CHECK(ldpc_encode(genc, info.data(), pool.data(), pool_n));
        else CHECK(ldpc_dvbs2_encode(h, info.data(), pool.data(), pool_n));
    }
    const char *chain = o.f16 ? "f16" : o.f32 ? "f32" : (o.f32q ? "f32q" : "i8");
    const char *algo = o.p.algo == LDPC_ALGO_BP    ? "BP"
                       : o.p.algo == LDPC_ALGO_NMS ? "NMS"
                                                   : (o.p.algo == LDPC_ALGO_MS ? "MS" : "OMS");
    printf("(II) code %s N=%d K=%d E=%d | %s | chain %s | iters %d | batch %d x %d GPU(s)\n", o.code.c_str(), n, k, e,
           algo, chain, o.iter, o.batch, o.gpus);
    for (double eb = o.min; eb <= o.max + 1e-9; eb += o.pas) {
        const double sigma = ldpc_awgn_sigma(eb, (double)k / n);
        Totals tot;
        auto t0 = std::chrono::steady_clock::now();
        std::vector<std::thread> th;
        for (int d = 0; d < o.gpus; d++)
            th.emplace_back(worker, d, h, std::cref(o), sigma, std::ref(tot), n, k, std::cref(pool), pool_n, genc);
        for (auto &t : th) t.join();
        const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        const long fr = tot.frames, fe = tot.fe, be = tot.be;
        const double ber = (double)be / fr / k, fer = (double)fe / fr;
        const double mbps = (double)fr * n / sec / 1e6;
        // CTerminal::final_report (code/x86/CTerminal/CTerminal.cpp:78-90) format
        printf("SNR = %.2f | BER =  %2.3e | FER =  %2.3e | BPS =  %2.2f | MATRICES = %10ld| FE = %ld | BE = %ld | "
               "BE/FE = %.1f | RUNTIME = %.2fs\n",
               eb, ber, fer, (double)fr * k / sec / 1e6, fr, fe, be, fe ? (double)be / fe : 0.0, sec);
        printf("{\"ebn0\": %.3f, \"sigma\": %.6f, \"frames\": %ld, \"frame_errors\": %ld, \"bit_errors\": %ld, "
               "\"ber\": %.6e, \"fer\": %.6e, \"coded_mbps\": %.3f, \"chain\": \"%s\", \"algo\": \"%s\", \"bp_staircase\": %s, "
               "\"f16_all_codes\": %s, \"f16_edge_parallel\": %s, \"ep_wide\": %s, \"i8_edge_parallel\": %s, "
               "\"i8_ep_wide\": %s}\n",
               eb, sigma, fr, fe, be, ber, fer, mbps, chain, algo, o.bpstair ? "true" : "false",
               o.f16all ? "true" : "false", o.f16ep ? "true" : "false", o.epwide ? "true" : "false",
               o.i8ep ? "true" : "false", o.i8epw ? "true" : "false");
        fflush(stdout);
    }
    ldpc_encoder_destroy(genc);
    ldpc_code_destroy(h);
    return 0;
}
