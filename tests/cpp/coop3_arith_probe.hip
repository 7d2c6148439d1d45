// coop3_arith_probe.hip -- libc3probe.so: the packed 16-bit arithmetic of the
// coop3 kernel (pk16.h, coop3_kernel.h, both included unchanged) run on the
// device against the scalar reference coop3_arith_ref.h over whole input
// domains (tests/test_gpu_coop3_arith.py).  Every kernel is an ordinary grid
// whose buffer indices are bounded by the launch shape; the large products
// are reduced on the device: a mismatch count and the first 16 mismatching
// tuples come back.  The two halves of a dword always carry different tuples
// (tuple i in the low half, tuple N - 1 - i in the high half).
//
// Test infrastructure only: the main library neither contains nor links it.
#include "../../ldpcgputegra_amd/csrc/coop3_kernel.h"

#include "coop3_arith_ref.h"

using namespace c3;

namespace {

struct Out {                    // what a reducing probe returns
    unsigned long long n;       // mismatches
    int t[16][8];               // the first 16: probe-specific fields
};

__device__ void report(Out *o, int a0, int a1 = 0, int a2 = 0, int a3 = 0, int a4 = 0, int a5 = 0, int a6 = 0, int a7 = 0)
{
    const unsigned long long k = atomicAdd(&o->n, 1ull);
    if (k < 16) {
        int *t = o->t[k];
        t[0] = a0, t[1] = a1, t[2] = a2, t[3] = a3, t[4] = a4, t[5] = a5, t[6] = a6, t[7] = a7;
    }
}

// ---- four pieces of Slab3::pre that could not be made functions of the
// kernel's without changing its instructions (register allocation): restated
// here line for line.  A change to the kernel's lines must be repeated here.
// copies Slab3::pre, tail branch: "the chain passes V[p_0] (the tail's last edge) on" .. "EPS = 0"
template <bool NMS>
LDPC_DEV void chain_tail(uint32_t y, uint32_t &A, uint32_t &B, uint32_t &EPS, uint32_t &COV, uint32_t &L, uint32_t &H)
{
    const uint32_t Y = pk_ashr8(y);
    A = B = COV = L = H = Y;
    if constexpr (NMS) {
        A = pk_shl5(Y);
        B = pk_add(A, 0x001F001Fu);
    }
    EPS = 0;
}
// copies Slab3::pre: the body of "if (!(meta & COOP_M_ACT))", the pass-through slot
template <bool NMS>
LDPC_DEV void chain_pass(uint32_t &A, uint32_t &B, uint32_t &EPS, uint32_t &COV, uint32_t &L, uint32_t &H)
{
    A = COV = 0;
    B = NMS ? 0x001F001Fu : 0u;
    EPS = NMS ? 0x00200020u : 0x00010001u;
    L = VNEG127;
    H = V127;
}
// copies Slab3::pre: "per codeword records: (A, B), (eps, c_o), (L, H) as i16 pairs", r0.x .. r0.w = r1.w = 0
LDPC_DEV void chain_pack(uint32_t A, uint32_t B, uint32_t EPS, uint32_t COV, uint32_t L, uint32_t H, uint4 &r0,
                         uint4 &r1)
{
    r0.x = perm(B, A, 0x05040100u);
    r1.x = perm(B, A, 0x07060302u);
    r0.y = perm(COV, EPS, 0x05040100u);
    r1.y = perm(COV, EPS, 0x07060302u);
    r0.z = perm(H, L, 0x05040100u);
    r1.z = perm(H, L, 0x07060302u);
    r0.w = r1.w = 0;
}

// copies Slab3::pre, tail branch: k1, k2 and signed_csts (later group: the clip at msg_max comes after the offset)
template <bool NMS, bool ODD>
LDPC_DEV void tail_csts(uint32_t min1, uint32_t min2, uint32_t sacc, const PkK &K, uint32_t fk, uint32_t &e1,
                        uint32_t &e2)
{
    const uint32_t k1 = NMS ? nms_c(pk_min(min2, K.rmm), fk)
                            : pk_min(pk_max(pk_sub(min2, K.coff), 0u), K.rmm) & HIBYTES;
    const uint32_t k2 = NMS ? nms_c(pk_min(min1, K.rmm), fk)
                            : pk_min(pk_max(pk_sub(min1, K.coff), 0u), K.rmm) & HIBYTES;
    signed_csts(k1, k2, sacc ^ (ODD ? SIGNS : 0u), e1, e2);
}


__device__ uint32_t Rf(int x) { return (uint32_t)(256 * x + 255) & 0xFFFFu; }   // R(x) of one half
__device__ uint32_t Cf(int m) { return (uint32_t)(256 * m) & 0xFFFFu; }         // C(m)
__device__ uint32_t pk(uint32_t lo, uint32_t hi) { return (lo & 0xFFFFu) | (hi << 16); }
__device__ int half(uint32_t x, int h) { return (int)((x >> (16 * h)) & 0xFFFFu); }
__device__ PkK make_k(int mm, int off)
{
    PkK K;
    K.neg127 = RNEG127, K.r0 = R0, K.c510 = C510;
    K.rmm = Rf(mm) * 0x10001u;
    K.coff = (Cf(off) + 255u) * 0x10001u;
    return K;
}
// (V, m) realising the difference d = V - m in -191 .. 190
__device__ void vm_of(int d, int &v, int &m)
{
    v = d < -128 ? -128 : d > 127 ? 127 : d;
    m = v - d;
}

// ---- message decode: msg_tab, old_msg<J>, old_msg2<J, NMA>
constexpr int NC = 4 * 127 * 127;   // (code, cst1, cst2)
__device__ void msg_tuple(int i, int &code, int &c1, int &c2)
{
    c2 = i % 127 - 63;
    c1 = i / 127 % 127 - 63;
    code = i / (127 * 127);
}
template <int NMA>
__global__ void k_msg(Out *o)
{
    const long long total = (long long)(8 * NMA) * 3 * NC;
    for (long long g = blockIdx.x * (long long)blockDim.x + threadIdx.x; g < total; g += (long long)gridDim.x * blockDim.x) {
        const int i = (int)(g % NC), fill = (int)(g / NC % 3), J = (int)(g / NC / 3);
        int cd[2], c1[2], c2[2];
        msg_tuple(i, cd[0], c1[0], c2[0]);
        msg_tuple(NC - 1 - i, cd[1], c1[1], c2[1]);
        uint32_t MA[NMA];
        for (int w = 0; w < NMA; w++) MA[w] = fill == 0 ? 0u : fill == 1 ? 0xFFFFFFFFu : 0x9C36E1A5u * (uint32_t)(2 * w + 1);
        const int sh = 2 * (J & 7);
        MA[J >> 3] = (MA[J >> 3] & ~((3u << sh) | (3u << (16 + sh)))) | ((uint32_t)cd[0] << sh) | ((uint32_t)cd[1] << (16 + sh));
        const uint32_t MB = (uint32_t)(c1[0] & 0xFF) | (uint32_t)(c2[0] & 0xFF) << 8 | (uint32_t)(c1[1] & 0xFF) << 16 |
                            (uint32_t)(c2[1] & 0xFF) << 24;
        const MsgTab t = msg_tab(MB);
        PkK K = make_k(31, 1);
        uint32_t got = 0, got1 = 0;
        static_for<0, 8 * NMA>([&](auto jc) {
            constexpr int JJ = decltype(jc)::value;
            if (J == JJ) {
                got = old_msg2<JJ>(MA, t, K);
                got1 = NMA == 1 ? old_msg<JJ & 7>(MA[0], t) : got;
            }
        });
        const uint32_t exp = pk(Cf(c3ref::msg_of_code(cd[0], c1[0], c2[0])), Cf(c3ref::msg_of_code(cd[1], c1[1], c2[1])));
        if (got != exp || got1 != exp) report(o, J, fill, cd[0], c1[0], c2[0], (int)got, (int)exp, (int)got1);
    }
}

// ---- contribution and magnitude: every V x every message, values copied back
constexpr int NVM = 256 * 127;
__global__ void k_contrib(uint32_t *c_out, uint32_t *as_out, uint32_t *ar_out, Out *o)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= NVM) return;
    int v[2], m[2];
    v[0] = i / 127 - 128, m[0] = i % 127 - 63;
    v[1] = (NVM - 1 - i) / 127 - 128, m[1] = (NVM - 1 - i) % 127 - 63;
    const uint32_t c = pk_sub_sat(pk(Rf(v[0]), Rf(v[1])), pk(Cf(m[0]), Cf(m[1])));
    const uint32_t as = abs_sat(c, C510);
    const uint32_t cc = pk_max(c, RNEG127);
    const uint32_t ar = abs_r(cc, C510);
    c_out[i] = c, as_out[i] = as, ar_out[i] = ar;
    for (int h = 0; h < 2; h++) {
        const int d = v[h] - m[h], cr = c3ref::contrib(v[h], m[h]);
        const int ec = d < -128 ? 0x8000 : (int)Rf(c3ref::sat8(d));
        const int ea = (int)Rf(c3ref::iabs(cr));
        if (half(c, h) != ec) report(o, 0, h, v[h], m[h], half(c, h), ec);
        if (half(as, h) != ea) report(o, 1, h, v[h], m[h], half(as, h), ea);
        if (half(cc, h) != (int)Rf(cr)) report(o, 2, h, v[h], m[h], half(cc, h), (int)Rf(cr));
        if (half(ar, h) != ea) report(o, 3, h, v[h], m[h], half(ar, h), ea);
    }
}
// unpack_v / pack_v: every u16 pair in either half of a V dword (the other half its complement)
__global__ void k_vpack(uint32_t *un_out, uint32_t *pk_out, Out *o)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= 2 * 65536) return;
    const uint32_t r = (uint32_t)i & 0xFFFFu, hi = (uint32_t)i >> 16;
    const uint32_t raw = hi ? (r << 16) | (~r & 0xFFFFu) : r | (~r << 16);
    const uint32_t u = unpack_v(raw, 0x010d000du + hi * 0x02000200u);
    const uint32_t p = pack_v(u);
    un_out[i] = u, pk_out[i] = p;
    const uint32_t eu = pk(Rf((int)(int8_t)(r & 0xFF)), Rf((int)(int8_t)(r >> 8)));
    if (u != eu) report(o, 0, (int)hi, (int)r, 0, (int)u, (int)eu);
    if (p != r) report(o, 1, (int)hi, (int)r, 0, (int)p, (int)r);
    if (hi == 0) {   // the chain inputs' form: two values' low bytes -> R pair
        const uint32_t x = Slab3<7, 6, 2>::x_of(make_uint2(r & 0xFFu, r >> 8));
        if (x != eu) report(o, 2, 0, (int)r, 0, (int)x, (int)eu);
    }
}

// ---- constants: signed_csts, nms_v, nms_c, post_finish, tail_csts
// tuple: (min, msg_max, param, parity, form); form 0 .. 2: where the minimum enters post_finish
template <bool NMS, bool ODD>
__global__ void k_consts(Out *o)
{
    const int NP_ = NMS ? 65 : 64;
    const int total = 128 * 64 * NP_ * 2 * 3;
    for (int g = blockIdx.x * blockDim.x + threadIdx.x; g < total; g += gridDim.x * blockDim.x) {
        int mn[2], par[2], form[2], sgn[2];
        const int par_ = g / (128 * 64) / NP_;   // (parity, form): shared by both halves except the mirrored ones below
        const int mm = g / 128 % 64, prm = g / (128 * 64) % NP_;
        mn[0] = g % 128, mn[1] = 127 - mn[0];
        par[0] = par_ & 1, par[1] = !par[0];
        form[0] = par_ >> 1, form[1] = (form[0] + 1) % 3;
        sgn[0] = (g >> 3) & 1, sgn[1] = !sgn[0];
        const PkK K = make_k(mm, NMS ? 0 : prm);
        const uint32_t fk = (uint32_t)prm * 0x10001u;
        const c3ref::Params P{NMS, prm, mm};
        // form 0: |c_x| = min, the others 127; form 1: mn1 = min, |c_x| = 127; form 2: mn1 = 0, mn2 = min, |c_x| = 127
        int y[2], m1[2], m2[2];
        for (int h = 0; h < 2; h++) {
            y[h] = (form[h] == 0 ? mn[h] : 127) * (sgn[h] ? -1 : 1);
            m1[h] = form[h] == 0 ? 127 : form[h] == 1 ? mn[h] : 0;
            m2[h] = form[h] == 2 ? mn[h] : 127;
        }
        uint32_t cx, ax, min1, min2, k1, k2, e1, e2;
        post_finish<NMS, ODD>(pk(Rf(y[0]), Rf(y[1])), 0u, pk(Rf(m1[0]), Rf(m1[1])), pk(Rf(m2[0]), Rf(m2[1])),
                              pk(par[0] ? 0x8000u : 0u, par[1] ? 0x8000u : 0u), K, fk, cx, ax, min1, min2, k1, k2, e1, e2);
        uint32_t t1, t2;
        tail_csts<NMS, ODD>(pk(Rf(m1[0]), Rf(m1[1])), pk(Rf(m2[0]), Rf(m2[1])), pk(par[0] ? 0x8000u : 0u, par[1] ? 0x8000u : 0u),
                            K, fk, t1, t2);
        const uint32_t nv = nms_v(pk(Rf(c3ref::imin(mn[0], mm)), Rf(c3ref::imin(mn[1], mm))), fk);
        const uint32_t nc = nms_c(pk(Rf(c3ref::imin(mn[0], mm)), Rf(c3ref::imin(mn[1], mm))), fk);
        for (int h = 0; h < 2; h++) {
            const int a = c3ref::iabs(y[h]);
            const int r1 = c3ref::imin(a, m1[h]), r2 = c3ref::imax(m1[h], c3ref::imin(a, m2[h]));
            const int q1 = c3ref::cst(P, c3ref::imin(r2, mm)), q2 = c3ref::cst(P, c3ref::imin(r1, mm));   // first group: a clipped
            const int neg = par[h] ^ (y[h] < 0) ^ (ODD ? 1 : 0);
            const bool ok = half(cx, h) == (int)Rf(y[h]) && half(ax, h) == (int)Rf(a) && half(min1, h) == (int)Rf(r1) &&
                            half(min2, h) == (int)Rf(r2) && half(k1, h) == (int)Cf(q1) && half(k2, h) == (int)Cf(q2) &&
                            half(e1, h) == (int)Cf(neg ? -q1 : q1) && half(e2, h) == (int)Cf(neg ? -q2 : q2);
            if (!ok) report(o, 0, h, mn[h], mm, prm, par[h] | form[h] << 1 | sgn[h] << 3, (int)(e1 >> (16 * h) & 0xFFFF) | (int)(e2 >> (16 * h)) << 16,
                            (int)Cf(neg ? -q1 : q1) | (int)Cf(neg ? -q2 : q2) << 16);
            // the tail check: later group, the magnitudes are clipped by mag(), the constants after the offset
            const int u1 = c3ref::cst(P, NMS ? c3ref::imin(m2[h], mm) : m2[h]), u2 = c3ref::cst(P, NMS ? c3ref::imin(m1[h], mm) : m1[h]);
            const int tn = par[h] ^ (ODD ? 1 : 0);
            if (half(t1, h) != (int)Cf(tn ? -u1 : u1) || half(t2, h) != (int)Cf(tn ? -u2 : u2))
                report(o, 1, h, mn[h], mm, prm, par[h] | form[h] << 1, (int)(t1 >> (16 * h) & 0xFFFF) | (int)(t2 >> (16 * h)) << 16,
                       (int)Cf(tn ? -u1 : u1) | (int)Cf(tn ? -u2 : u2) << 16);
            if (NMS) {
                const int e = (c3ref::imin(mn[h], mm) * prm) >> 5;
                if (half(nv, h) != e) report(o, 2, h, mn[h], mm, prm, 0, half(nv, h), e);
                if (half(nc, h) != (int)Cf(e)) report(o, 3, h, mn[h], mm, prm, 0, half(nc, h), (int)Cf(e));
            }
        }
    }
}
// signed_csts alone: every k1, k2 in 0 .. 127 (C form) x both parities
__global__ void k_signed(uint32_t *e_out, Out *o)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int N = 128 * 128 * 2;
    if (i >= N) return;
    int k1[2], k2[2], p[2];
    for (int h = 0; h < 2; h++) {
        const int j = h ? N - 1 - i : i;
        k1[h] = j % 128, k2[h] = j / 128 % 128, p[h] = j / (128 * 128);
    }
    uint32_t e1, e2;
    signed_csts(pk(Cf(k1[0]), Cf(k1[1])), pk(Cf(k2[0]), Cf(k2[1])), pk(p[0] ? 0x8000u : 0x7FFFu, p[1] ? 0xFFFFu : 0u), e1, e2);
    e_out[2 * i] = e1, e_out[2 * i + 1] = e2;
    for (int h = 0; h < 2; h++)
        if (half(e1, h) != (int)Cf(p[h] ? -k1[h] : k1[h]) || half(e2, h) != (int)Cf(p[h] ? -k2[h] : k2[h]))
            report(o, h, k1[h], k2[h], p[h], half(e1, h), half(e2, h));
}

// ---- new V and codes: new_v<J>, msg_code<J>, new_v_later<J>, add_code<J>
// tuple: (d = V - m, min1 <= a, cst2 <= cst1 <= 63, eps); mm < 0: first group
constexpr int NCS = 64 * 65 / 2;   // (cst1, cst2) pairs
constexpr long long NNV = 382ll * 128 * NCS * 2;
__device__ void nv_tuple(long long i, int &d, int &mn, int &c1, int &c2, int &eps)
{
    eps = (int)(i & 1) ? -1 : 1;
    int cs = (int)(i / 2 % NCS);
    c1 = 0;
    while (cs > c1) cs -= ++c1;   // cs-th pair (c1, c2 <= c1)
    c2 = cs;
    mn = (int)(i / 2 / NCS % 128);
    d = (int)(i / 2 / NCS / 128) - 191;
}
template <bool LATER>
__global__ void k_newv(int mm, int fill, Out *o)
{
    for (long long g = blockIdx.x * (long long)blockDim.x + threadIdx.x; g < 8 * NNV; g += (long long)gridDim.x * blockDim.x) {
        const int J = (int)(g / NNV);
        const long long i = g % NNV;
        int d[2], mn[2], c1[2], c2[2], eps[2], v[2], m[2], cr[2], a[2];
        nv_tuple(i, d[0], mn[0], c1[0], c2[0], eps[0]);
        nv_tuple(NNV - 1 - i, d[1], mn[1], c1[1], c2[1], eps[1]);
        for (int h = 0; h < 2; h++) {
            vm_of(d[h], v[h], m[h]);
            cr[h] = c3ref::contrib(v[h], m[h]);
            a[h] = c3ref::mag(!LATER, cr[h], LATER ? mm : 127);
            if (mn[h] > a[h]) mn[h] = a[h] - (mn[h] - a[h] - 1) % (a[h] + 1);   // min1 <= a: fold the rest back into 0 .. a
        }
        const PkK K = make_k(LATER ? mm : 63, 0);
        uint32_t c = pk_sub_sat(pk(Rf(v[0]), Rf(v[1])), pk(Cf(m[0]), Cf(m[1])));
        uint32_t av;
        if (LATER) {
            c = pk_max(c, K.neg127);
            av = abs_r(pk_min(c, K.rmm), K.c510);
        } else
            av = abs_sat(c, K.c510);
        const uint32_t min1 = pk(Rf(mn[0]), Rf(mn[1]));
        const uint32_t e1 = pk(Cf(eps[0] * c1[0]), Cf(eps[1] * c1[1])), e2 = pk(Cf(eps[0] * c2[0]), Cf(eps[1] * c2[1]));
        const uint32_t slot = 0x00030003u << (2 * J);
        const uint32_t MA0 = fill ? ~slot : 0u;
        uint32_t MA = MA0, MC = MA0, MD = MA0, nv = 0;
        static_for<0, 8>([&](auto jc) {
            constexpr int JJ = decltype(jc)::value;
            if (J == JJ) {
                if constexpr (LATER)
                    nv = new_v_later<JJ>(c, av, min1, e1, e2, MA, K.neg127);
                else
                    nv = new_v<JJ>(c, av, min1, e1, e2, MA, K.c510);
                msg_code<JJ>(c, av, min1, MC);
                MD = add_code<JJ>(MD, pk_sra15(c), pk_sra15(pk_sub(min1, av)));
            }
        });
        uint32_t ev = 0, ema = MA0;
        for (int h = 0; h < 2; h++) {
            const int r = a[h] == mn[h] ? c1[h] : c2[h];
            const int msg = c3ref::message(cr[h], r, eps[h] < 0);
            ev |= Rf(c3ref::new_v(cr[h], msg)) << (16 * h);
            ema |= (uint32_t)((cr[h] < 0) | (a[h] > mn[h]) << 1) << (2 * J + 16 * h);
        }
        if (nv != ev || MA != ema || MC != ema || MD != ema)
            for (int h = 0; h < 2; h++)
                if (half(nv, h) != half(ev, h) || half(MA, h) != half(ema, h) || half(MC, h) != half(ema, h) || half(MD, h) != half(ema, h))
                    report(o, J, d[h], mn[h], c1[h] | c2[h] << 8, eps[h], half(nv, h) | half(MA, h) << 16, half(ev, h) | half(ema, h) << 16,
                           half(MC, h) | half(MD, h) << 16);
    }
}

// ---- min tracking: min_track / min_merge2 as the pre runs them, Slab3::merge
// One tuple per lane pair: the smallest s1 at edge p1, the second smallest s2
// at p2, every other edge `oth` (>= s2); signs from the tuple index.
// D0 < 22: both lanes of a pair compute the whole check (two tuples per dword);
// HALF: lane h reduces edges [h XH, h XH + XH), sinks (c = R(127), no sign) past X.
template <int D0>
__global__ void k_min(const int *tup, int ntup, Out *o)
{
    using G = G3<D0>;
    constexpr int X = G::X, XL = G::XH;
    const int lane = threadIdx.x;
    const int nwork = (ntup + 31) / 32 * 32;   // every lane of a wave runs the same count: merge is a DPP exchange
    for (int w0 = blockIdx.x * 32; w0 < nwork; w0 += gridDim.x * 32) {
        const int wi = w0 + (lane >> 1);
        const bool live = wi < ntup;
        const int hh = G::HALF ? (lane & 1) : 0;
        int ti[2] = {live ? wi : 0, live ? ntup - 1 - wi : 0};
        uint32_t a[XL], sg[XL];
        int e1v[2], e2v[2], es[2];
        for (int h = 0; h < 2; h++) {
            const int *t = tup + 5 * ti[h];   // p1, p2, s1, s2, oth
            e1v[h] = t[2], e2v[h] = t[3], es[h] = 0;
            for (int j = 0; j < X; j++) es[h] ^= (int)(((unsigned)ti[h] * 2654435761u >> (j & 31)) & 1u);
        }
#pragma unroll
        for (int j = 0; j < XL; j++) {
            const int e = hh * XL + j;
            uint32_t av = 0, sv_ = 0;
            for (int h = 0; h < 2; h++) {
                const int *t = tup + 5 * ti[h];
                const int val = e >= X ? 127 : e == t[0] ? t[2] : e == t[1] ? t[3] : t[4];
                const uint32_t s = e >= X ? 0u : ((unsigned)ti[h] * 2654435761u >> (e & 31)) & 1u;
                av |= Rf(val) << (16 * h);
                sv_ |= (s ? 0x8000u : 0u) << (16 * h);
            }
            a[j] = av, sg[j] = sv_;
        }
        uint32_t min1 = R127, min2 = R127, sacc = 0;
        if constexpr (XL < LDPC_C3_PRE_CHUNK_X) {
            static_for<0, XL>([&](auto jc) {
                constexpr int J = decltype(jc)::value;
                sacc ^= sg[J];
                min_track<J>(min1, min2, a[J]);
            });
        } else {
            uint32_t m1[2] = {R127, R127}, m2[2] = {R127, R127};
            static_for<0, XL>([&](auto jc) {
                constexpr int J = decltype(jc)::value;
                sacc ^= sg[J];
                min_track<2>(m1[J & 1], m2[J & 1], a[J]);
            });
            min_merge2(m1, m2, min1, min2);
        }
        if constexpr (G::HALF) Slab3<D0, G::WS, 2>::merge(min1, min2, sacc);
        if (live)
            for (int h = 0; h < 2; h++)
                if (half(min1, h) != (int)Rf(e1v[h]) || half(min2, h) != (int)Rf(e2v[h]) || (half(sacc, h) >> 15) != es[h])
                    report(o, D0, ti[h], hh, half(min1, h), half(min2, h), half(sacc, h) >> 15, (int)Rf(e1v[h]) | (int)Rf(e2v[h]) << 16, es[h]);
    }
}

// ---- the chain step: chain_consts -> chain_pack -> chain_window3 -> xo and w
constexpr int CS = 16;   // steps of the probe's window: two blocks of 8
struct ChainSm {
    uint4 cst[2][CS][2][NP];
    uint4 xo[2][CS / 8][CW];
};
// kind 0: first-group record; 1: the tail record (output = the tail's V); 2:
// pass-through only; 3: first-group record with the FZ override (output = the
// o edge's V as read).  tuple: (Y, m_x, c_o, eps, tmin index, param index)
__constant__ int c_set[9] = {0, 1, 2, 30, 31, 32, 62, 63, 64};
template <bool NMS, bool PF2>
__global__ void __launch_bounds__(64) k_chain(int pos, int mm, int kind, int full, Out *o)
{
    __shared__ ChainSm smg[4];
    const int lane = threadIdx.x & 15, grp = threadIdx.x >> 4;
    ChainSm &sm = smg[grp];
    const int NS = NMS ? 9 : 8;
    // full: clipped-min x param over their whole range at c_o in {-127, -1, 0, 1, 127}
    const long long nt = full ? 255ll * 127 * 5 * 2 * 64 * (NMS ? 65 : 64) : 255ll * 127 * 255 * 2 * 8 * NS;
    const long long nit = (nt + 7) / 8;   // 8 tuples and their mirrors per 16 lanes
    auto tuple = [&](long long i, int &y, int &mx, int &co, int &eps, int &tm, int &prm) {
        eps = (i & 1) ? -1 : 1, i >>= 1;
        if (full) {
            const int cov[5] = {-127, -1, 0, 1, 127};
            tm = (int)(i % 64), i /= 64;
            prm = (int)(i % (NMS ? 65 : 64)), i /= (NMS ? 65 : 64);
            co = cov[i % 5], i /= 5;
        } else {
            tm = c_set[i % 8], i /= 8;
            prm = c_set[i % NS], i /= NS;
            co = (int)(i % 255) - 127, i /= 255;
        }
        mx = (int)(i % 127) - 63, i /= 127;
        y = (int)(i % 255) - 127;
    };
    // every step a pass-through record (a production record)
    if (lane < NP) {
        uint32_t A, B, EPS, COV, L, H;
        chain_pass<NMS>(A, B, EPS, COV, L, H);
        uint4 r0, r1;
        chain_pack(A, B, EPS, COV, L, H, r0, r1);
        for (int s = 0; s < CS; s++) sm.cst[0][s][0][lane] = r0, sm.cst[0][s][1][lane] = r1;
    }
    const long long stride = (long long)gridDim.x * 4;
    for (long long it = blockIdx.x * 4ll + grp; it < (nit + stride - 1) / stride * stride; it += stride) {
        const bool live = it < nit;
        const long long base = live ? it * 8 : 0;
        __syncthreads();
        if (lane < NP && kind != 2) {   // the pre's lane of pair q = lane: codewords 2q (tuple), 2q + 1 (its mirror)
            int y[2], mx[2], co[2], eps[2], tm[2], prm[2];
            const long long i0 = base + lane < nt ? base + lane : nt - 1;
            tuple(i0, y[0], mx[0], co[0], eps[0], tm[0], prm[0]);
            tuple(nt - 1 - i0, y[1], mx[1], co[1], eps[1], tm[1], prm[1]);
            // one parameter per record pair: the low half's
            const PkK K = make_k(mm, NMS ? 0 : prm[0]);
            const uint32_t fk = (uint32_t)prm[0] * 0x10001u, offp = NMS ? 0u : (uint32_t)prm[0] * 0x10001u;
            uint32_t A, B, EPS, COV, L, H;
            if (kind == 1)
                chain_tail<NMS>(pk(Rf(co[0]), Rf(co[1])), A, B, EPS, COV, L, H);
            else {
                chain_consts<NMS>(pk(Rf(co[0]), Rf(co[1])), pk(Cf(mx[0]), Cf(mx[1])), pk(Rf(tm[0]), Rf(tm[1])),
                                  pk(eps[0] < 0 ? 0x8000u : 0u, eps[1] < 0 ? 0x8000u : 0u), K, fk, offp, A, B, EPS, COV, L, H);
                if (kind == 3) chain_freeze(0xFFFFFFFFu, pk(Rf(mx[0]), Rf(mx[1])), L, H);   // V[p_i] as read: m_x's value here
            }
            uint4 r0, r1;
            chain_pack(A, B, EPS, COV, L, H, r0, r1);
            sm.cst[0][pos][0][lane] = r0, sm.cst[0][pos][1][lane] = r1;
        }
        __syncthreads();
        int y, mx, co, eps, tm, prm, prm0, d0, d1, d2, d3, d4;
        const long long il = base + (lane >> 1) < nt ? base + (lane >> 1) : nt - 1;
        const long long ii = (lane & 1) ? nt - 1 - il : il;
        tuple(ii, y, mx, co, eps, tm, prm);
        tuple(il, d0, d1, d2, d3, d4, prm0);
        uint32_t w[4] = {(uint32_t)y & 0xFFFFu, 0, 0, 0};
        chain_window3<4, 2, 0, CS / 8, NMS, PF2>(sm, 0, lane, w);
        const c3ref::Params P{NMS, prm0, mm};
        const int exp = kind == 0 ? c3ref::chain_step(P, y, mx, co, tm, eps) : kind == 1 ? co : kind == 2 ? y : mx;
        const int got = (int)(short)(w[0] & 0xFFFFu);
        // xo: the inputs of the 16 steps: Y up to the record's position, its output after it
        const unsigned short *xs = (const unsigned short *)&sm.xo[0][0][lane];
        const unsigned short *xs1 = (const unsigned short *)&sm.xo[0][1][lane];
        bool ok = got == exp;
        for (int s = 0; s < CS; s++) {
            const int xv = (int)(short)(s < 8 ? xs[s] : xs1[s - 8]);
            ok = ok && xv == (s <= pos ? y : exp);
        }
        if (live && base + (lane >> 1) < nt && !ok) report(o, y, mx, co, eps, tm, prm0, got, exp);
    }
}

// ---- ET bit helpers
__global__ void k_bits(const uint4 *in, int n, uint32_t *pb, uint32_t *hb, uint32_t *rb, Out *o)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint4 x = in[i];
    const unsigned xa[4] = {x.x, x.y, x.z, x.w};
    pb[i] = pos_bits(x.x), hb[i] = high_bits16(x), rb[i] = row_hbits(x);
    if (pb[i] != c3ref::pos_bits(x.x)) report(o, 0, i, (int)x.x, 0, 0, 0, (int)pb[i], (int)c3ref::pos_bits(x.x));
    if (hb[i] != c3ref::high_bits16(xa)) report(o, 1, i, (int)x.x, (int)x.y, (int)x.z, (int)x.w, (int)hb[i], (int)c3ref::high_bits16(xa));
    if (rb[i] != c3ref::row_hbits(xa)) report(o, 2, i, (int)x.x, (int)x.y, (int)x.z, (int)x.w, (int)rb[i], (int)c3ref::row_hbits(xa));
}

// ---- host side
struct DevOut {
    Out *d = nullptr;
    hipError_t e;
    DevOut()
    {
        e = hipMalloc(&d, sizeof(Out));
        if (e == hipSuccess) e = hipMemset(d, 0, sizeof(Out));
    }
    int finish(unsigned long long *count, int *tuples)
    {
        if (e == hipSuccess) e = hipGetLastError();
        if (e == hipSuccess) e = hipDeviceSynchronize();
        Out h{};
        if (e == hipSuccess) e = hipMemcpy(&h, d, sizeof(Out), hipMemcpyDeviceToHost);
        if (d) (void)hipFree(d);
        *count = h.n;
        for (int i = 0; i < 16 * 8; i++) tuples[i] = h.t[i / 8][i % 8];
        return (int)e;
    }
};
template <typename T>
struct DevBuf {
    T *d = nullptr;
    size_t n;
    hipError_t e;
    explicit DevBuf(size_t n_, const T *src = nullptr) : n(n_)
    {
        e = hipMalloc(&d, n * sizeof(T));
        if (e == hipSuccess) e = src ? hipMemcpy(d, src, n * sizeof(T), hipMemcpyHostToDevice) : hipMemset(d, 0, n * sizeof(T));
    }
    hipError_t get(T *dst) { return hipMemcpy(dst, d, n * sizeof(T), hipMemcpyDeviceToHost); }
    ~DevBuf()
    {
        if (d) (void)hipFree(d);
    }
};
constexpr int GRID = 2048, TPB = 256;

}  // namespace

extern "C" {

int c3p_msg(int nma, unsigned long long *count, int *tuples)
{
    DevOut o;
    if (o.e == hipSuccess) {
        if (nma == 1) k_msg<1><<<GRID, TPB>>>(o.d);
        else if (nma == 2) k_msg<2><<<GRID, TPB>>>(o.d);
        else if (nma == 4) k_msg<4><<<GRID, TPB>>>(o.d);
        else o.e = hipErrorInvalidValue;
    }
    return o.finish(count, tuples);
}

// c, abs_sat, abs_r: NVM dwords each (tuple i = (V, m) in the low half, NVM - 1 - i in the high half)
int c3p_contrib(uint32_t *c, uint32_t *as, uint32_t *ar, unsigned long long *count, int *tuples)
{
    DevOut o;
    DevBuf<uint32_t> dc(NVM), da(NVM), dr(NVM);
    if (o.e == hipSuccess && dc.e == hipSuccess && da.e == hipSuccess && dr.e == hipSuccess) k_contrib<<<(NVM + TPB - 1) / TPB, TPB>>>(dc.d, da.d, dr.d, o.d);
    else if (o.e == hipSuccess) o.e = hipErrorOutOfMemory;
    const int rc = o.finish(count, tuples);
    if (rc) return rc;
    hipError_t e = dc.get(c);
    if (e == hipSuccess) e = da.get(as);
    if (e == hipSuccess) e = dr.get(ar);
    return (int)e;
}

// unpack_v / pack_v of every u16 pair in the low (i < 65536) and the high half of a V dword: 2 * 65536 dwords each
int c3p_vpack(uint32_t *un, uint32_t *pkd, unsigned long long *count, int *tuples)
{
    DevOut o;
    DevBuf<uint32_t> du(2 * 65536), dp(2 * 65536);
    if (o.e == hipSuccess && du.e == hipSuccess && dp.e == hipSuccess) k_vpack<<<2 * 65536 / TPB, TPB>>>(du.d, dp.d, o.d);
    else if (o.e == hipSuccess) o.e = hipErrorOutOfMemory;
    const int rc = o.finish(count, tuples);
    if (rc) return rc;
    hipError_t e = du.get(un);
    if (e == hipSuccess) e = dp.get(pkd);
    return (int)e;
}

int c3p_consts(int nms, int odd, unsigned long long *count, int *tuples)
{
    DevOut o;
    if (o.e == hipSuccess) {
        if (nms && odd) k_consts<true, true><<<GRID, TPB>>>(o.d);
        else if (nms) k_consts<true, false><<<GRID, TPB>>>(o.d);
        else if (odd) k_consts<false, true><<<GRID, TPB>>>(o.d);
        else k_consts<false, false><<<GRID, TPB>>>(o.d);
    }
    return o.finish(count, tuples);
}

// e: 2 * 128 * 128 * 2 dwords (e1, e2 per tuple (k1, k2, parity))
int c3p_signed(uint32_t *e_out, unsigned long long *count, int *tuples)
{
    const int N = 128 * 128 * 2;
    DevOut o;
    DevBuf<uint32_t> de(2 * N);
    if (o.e == hipSuccess && de.e == hipSuccess) k_signed<<<N / TPB, TPB>>>(de.d, o.d);
    else if (o.e == hipSuccess) o.e = hipErrorOutOfMemory;
    const int rc = o.finish(count, tuples);
    return rc ? rc : (int)de.get(e_out);
}

// mm < 0: new_v / msg_code / add_code (first group); else new_v_later with a = |min(c, mm)|
int c3p_newv(int mm, int fill, unsigned long long *count, int *tuples)
{
    DevOut o;
    if (mm > 63) o.e = hipErrorInvalidValue;
    if (o.e == hipSuccess) {
        if (mm < 0) k_newv<false><<<4 * GRID, TPB>>>(63, fill, o.d);
        else k_newv<true><<<4 * GRID, TPB>>>(mm, fill, o.d);
    }
    return o.finish(count, tuples);
}

// tup: ntup x (p1, p2, s1, s2, oth), every position < the degree's X
int c3p_min(int d0, const int *tup, int ntup, unsigned long long *count, int *tuples)
{
    DevOut o;
    if (ntup <= 0) return (int)hipErrorInvalidValue;
    DevBuf<int> dt(5 * (size_t)ntup, tup);
    if (o.e == hipSuccess && dt.e != hipSuccess) o.e = dt.e;
    if (o.e == hipSuccess) {
        const int g = (ntup + 31) / 32 < 1024 ? (ntup + 31) / 32 : 1024;
        switch (d0) {
        case 7: k_min<7><<<g, 64>>>(dt.d, ntup, o.d); break;
        case 10: k_min<10><<<g, 64>>>(dt.d, ntup, o.d); break;
        case 14: k_min<14><<<g, 64>>>(dt.d, ntup, o.d); break;
        case 22: k_min<22><<<g, 64>>>(dt.d, ntup, o.d); break;
        case 27: k_min<27><<<g, 64>>>(dt.d, ntup, o.d); break;
        case 30: k_min<30><<<g, 64>>>(dt.d, ntup, o.d); break;
        default: o.e = hipErrorInvalidValue;
        }
    }
    return o.finish(count, tuples);
}

int c3p_chain(int nms, int pf2, int pos, int mm, int kind, int full, unsigned long long *count, int *tuples)
{
    DevOut o;
    if (pos < 0 || pos >= CS || mm < 0 || mm > 63 || kind < 0 || kind > 3) o.e = hipErrorInvalidValue;
    if (o.e == hipSuccess) {
        const int g = 4096;
        if (nms && pf2) k_chain<true, true><<<g, 64>>>(pos, mm, kind, full, o.d);
        else if (nms) k_chain<true, false><<<g, 64>>>(pos, mm, kind, full, o.d);
        else if (pf2) k_chain<false, true><<<g, 64>>>(pos, mm, kind, full, o.d);
        else k_chain<false, false><<<g, 64>>>(pos, mm, kind, full, o.d);
    }
    return o.finish(count, tuples);
}

// in: n x 4 dwords; pos_bits of the first dword, high_bits16 and row_hbits of each
int c3p_bits(const uint32_t *in, int n, uint32_t *pb, uint32_t *hb, uint32_t *rb, unsigned long long *count, int *tuples)
{
    DevOut o;
    if (n <= 0) return (int)hipErrorInvalidValue;
    DevBuf<uint4> di((size_t)n, (const uint4 *)in);
    DevBuf<uint32_t> dp(n), dh(n), dr(n);
    if (o.e == hipSuccess && (di.e != hipSuccess || dp.e != hipSuccess || dh.e != hipSuccess || dr.e != hipSuccess)) o.e = hipErrorOutOfMemory;
    if (o.e == hipSuccess) k_bits<<<(n + TPB - 1) / TPB, TPB>>>(di.d, n, dp.d, dh.d, dr.d, o.d);
    const int rc = o.finish(count, tuples);
    if (rc) return rc;
    hipError_t e = dp.get(pb);
    if (e == hipSuccess) e = dh.get(hb);
    if (e == hipSuccess) e = dr.get(rb);
    return (int)e;
}

int c3p_device_count()
{
    int n = 0;
    return hipGetDeviceCount(&n) == hipSuccess ? n : 0;
}
}
