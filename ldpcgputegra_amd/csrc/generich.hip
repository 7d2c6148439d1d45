// generich.hip -- any-H binary16 layered min-sum: generic.hip's generic_decode
// with two codewords per lane.  Another element type of kernel family 1, with
// the half contract of DESIGN.md §3 as its arithmetic (pk_f16.h).
//
// One lane = one pair: codewords 2q (low half) and 2q + 1 (high half).  Every
// lane walks the checks in schedule order, so H indices are wave-uniform
// (scalar loads) and V / message accesses are coalesced across the wave: V is
// V[node][stride] binary16 and the messages msg[edge][stride], both addressed
// as pairs, stride a multiple of 128 (generich_stride) so that a wave's piece
// of a row is one whole 256-B run.  Index arithmetic is 64-bit.  Early
// termination runs in the kernel per pair: the loop runs until both halves have
// stopped, and a stopped half is frozen by storing under a per-half mask
// (pk_f16.h put2; while no pair of the wave is half stopped, plain stores).
// With an odd batch the last pair's high half is the zero column the
// interleave wrote: it computes and the deinterleave never reads it.
#include <cstring>

#include "ldsh.h"
#include "pk_f16.h"

namespace {

using namespace pkf16;

struct GenhArgs {
    uint32_t *V;     // V[node][hs] pairs, hs = stride / 2
    uint32_t *msg;   // msg[edge][hs] pairs
    const uint32_t *ev;
    const int *gdeg;
    const int *gcnt;
    int n_groups, hs, batch, iters, early;
    uint32_t beta2;   // RNE16(beta) in both halves
    int32_t *iters_used;
};

// Vq / mp: this lane's column of V and of the check's messages
template <int D, int A, bool WHOLE>
LDPC_DEV void check(uint32_t *__restrict__ Vq, uint32_t *__restrict__ mp, const uint32_t *__restrict__ ev, size_t hs,
                    uint32_t beta2, uint32_t mask)
{
    uint32_t c[D], av[D];
    uint32_t sign = (D & 1) ? SGN2 : 0u;   // only bits 15 and 31 are ever used
    uint32_t m1 = INF2, m2 = INF2;
#pragma unroll
    for (int j = 0; j < D; j++) {
        c[j] = pk_sub(Vq[(size_t)ev[j] * hs], mp[(size_t)j * hs]);
        av[j] = c[j] & ABS2;
        sign ^= c[j];
        const uint32_t t = m1;
        m1 = pk_min(av[j], m1);
        m2 = pk_min(m2, pk_max(av[j], t));
    }
    const uint32_t sum = pk_addu(m1, m2);
#pragma unroll
    for (int j = 0; j < D; j++) {
        const uint32_t r = cst<A>(pk_subu(sum, pk_minu(av[j], m2)), beta2);
        const uint32_t m = with_sign(r, sign ^ c[j]);
        put2<WHOLE>(mp + (size_t)j * hs, m, mask);
        put2<WHOLE>(Vq + (size_t)ev[j] * hs, clamp_v(pk_add(c[j], m)), mask);
    }
}

template <int D, int A, bool WHOLE>
LDPC_DEV void run_group(uint32_t *Vq, uint32_t *mp, const uint32_t *ev, int cnt, size_t hs, uint32_t beta2,
                        uint32_t mask)
{
    for (int i = 0; i < cnt; i++) check<D, A, WHOLE>(Vq, mp + (size_t)i * D * hs, ev + (size_t)i * D, hs, beta2, mask);
}

// bit 0 / bit 1: some check of the low / high half's hard decisions fails
LDPC_DEV uint32_t syndrome_bad(const uint32_t *__restrict__ Vq, const uint32_t *__restrict__ ev, const int *gdeg,
                               const int *gcnt, int n_groups, size_t hs, uint32_t want)
{
    uint32_t bad = 0;
    for (int g = 0; g < n_groups; g++) {
        const int d = gdeg[g];
        for (int i = 0; i < gcnt[g]; i++, ev += d) {
            uint32_t par = 0;
            for (int j = 0; j < d; j++) par ^= pos2(Vq[(size_t)ev[j] * hs]);
            bad |= par;
            if ((bad & want) == want) return bad;   // every half still asked about has failed
        }
    }
    return bad;
}

#define LDPC_GENH_DEG_CASES(X) \
    X(2) X(3) X(4) X(5) X(6) X(7) X(8) X(9) X(10) X(11) X(12) X(13) X(14) X(15) X(16) X(17) X(18) X(19) \
    X(20) X(21) X(22) X(23) X(24) X(25) X(26) X(27) X(28) X(29) X(30) X(31) X(32)

template <int A>
__global__ void __launch_bounds__(64) generich_decode(GenhArgs a)
{
    const int q = blockIdx.x * 64 + threadIdx.x;
    const int b0 = 2 * q;
    if (b0 >= a.batch) return;
    const bool has1 = b0 + 1 < a.batch;
    const size_t hs = (size_t)a.hs;
    uint32_t *Vq = a.V + q;
    uint32_t *msg = a.msg + q;
    // without early termination the pair runs whole (a missing high half
    // computes on the zero column), with it a missing half counts as stopped
    bool al0 = true, al1 = a.early ? has1 : true;
    int it = 0;
    while (it < a.iters && (al0 || al1)) {
        const uint32_t mask = (al0 ? 0xFFFFu : 0u) | (al1 ? 0xFFFF0000u : 0u);
        // uniform over the lanes still in the loop: none has one half stopped, so every store is a whole pair
        const bool whole = !a.early || !__builtin_amdgcn_ballot_w64(al0 != al1);
        const uint32_t *ev = a.ev;
        uint32_t *mp = msg;
        for (int g = 0; g < a.n_groups; g++) {
            const int d = a.gdeg[g], cnt = a.gcnt[g];
            if (whole) {
                switch (d) {
#define X(DD) \
    case DD: run_group<DD, A, true>(Vq, mp, ev, cnt, hs, a.beta2, mask); break;
                    LDPC_GENH_DEG_CASES(X)
#undef X
                default: break;
                }
            } else {
                switch (d) {
#define X(DD) \
    case DD: run_group<DD, A, false>(Vq, mp, ev, cnt, hs, a.beta2, mask); break;
                    LDPC_GENH_DEG_CASES(X)
#undef X
                default: break;
                }
            }
            ev += (size_t)d * cnt;
            mp += (size_t)d * cnt * hs;
        }
        it++;
        if (a.early) {
            const uint32_t want = (al0 ? 1u : 0u) | (al1 ? 2u : 0u);
            const uint32_t bad = syndrome_bad(Vq, a.ev, a.gdeg, a.gcnt, a.n_groups, hs, want);
            if (al0 && !(bad & 1u)) {
                al0 = false;
                if (a.iters_used) a.iters_used[b0] = it;
            }
            if (al1 && !(bad & 2u)) {
                al1 = false;
                if (a.iters_used) a.iters_used[b0 + 1] = it;
            }
        }
    }
    if (a.iters_used) {   // codewords that never stopped
        if (al0) a.iters_used[b0] = it;
        if (has1 && al1) a.iters_used[b0 + 1] = it;
    }
}

uint32_t half_bits(float x)
{
    const _Float16 v = (_Float16)x;   // round to nearest even
    uint16_t u;
    memcpy(&u, &v, 2);
    return u;
}

}  // namespace

int launch_generich(const DecodeLaunch &L, hipStream_t s)
{
    if (L.stride % 128 != 0 || L.batch > L.stride || L.vpitch != L.stride) return -1;
    GenhArgs a;
    a.V = (uint32_t *)L.V;
    a.msg = (uint32_t *)L.msg;
    a.ev = L.d_edge_var;
    a.gdeg = L.d_group_deg;
    a.gcnt = L.d_group_cnt;
    a.n_groups = L.n_groups;
    a.hs = L.stride / 2;
    a.batch = L.batch;
    a.iters = L.iters;
    a.early = L.early;
    const uint32_t b16 = half_bits(L.beta) & 0x7FFFu;   // (-0.0 is +0)
    a.beta2 = b16 | (b16 << 16);
    a.iters_used = L.iters_used;
    const int pairs = (L.batch + 1) / 2;
    dim3 grid((pairs + 63) / 64), block(64);
    if (L.algo == 1)
        hipLaunchKernelGGL(generich_decode<1>, grid, block, 0, s, a);
    else if (b16 == 0)
        hipLaunchKernelGGL(generich_decode<2>, grid, block, 0, s, a);
    else
        hipLaunchKernelGGL(generich_decode<0>, grid, block, 0, s, a);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
