// coop3_arith_ref.h -- scalar reference of the check arithmetic that
// coop3_kernel.h / pk16.h evaluate in packed 16-bit form: plain ints holding
// int8 values, the per-check recurrence of SURVEY.md 8(a) written out.  No
// packed forms, no tables.  Compiled for the device beside the production
// functions (coop3_arith_probe.hip) and for the host (coop3_arith_ref_host.cpp),
// where tests/test_coop3_arith_ref_cpu.py pins it against the oracle.
#pragma once

#if defined(__HIPCC__)
#define C3REF __host__ __device__ inline
#else
#define C3REF inline
#endif

namespace c3ref {

constexpr int MAXD = 32;   // edges per check

struct Params {
    int nms;       // 0: OMS / MS (param = offset), 1: NMS (param = factor)
    int param;
    int msg_max;
};

C3REF int imin(int a, int b) { return a < b ? a : b; }
C3REF int imax(int a, int b) { return a > b ? a : b; }
C3REF int iabs(int a) { return a < 0 ? -a : a; }
C3REF int sat8(int x) { return imax(-128, imin(x, 127)); }

// contribution of an edge: V - old message, saturated, clamped at -127
C3REF int contrib(int v, int m) { return imax(sat8(v - m), -127); }
// its magnitude: first group min(|c|, msg_max), later groups |min(c, msg_max)|
// (NMS: the first form in every group)
C3REF int mag(bool first, int c, int msg_max) { return first ? imin(iabs(c), msg_max) : iabs(imin(c, msg_max)); }
// the constant a check sends back for a minimum
C3REF int cst(const Params &p, int mn)
{
    if (p.nms) return (mn * p.param) >> 5;
    return imin(imax(mn - p.param, 0), p.msg_max);
}
// new V of an edge: max(sat(c + m), -127)
C3REF int new_v(int c, int m) { return imax(sat8(c + m), -127); }
// the message: magnitude r, sign = (c < 0) xor parity
C3REF int message(int c, int r, int par) { return ((c < 0) != (par != 0)) ? -r : r; }

struct Check {
    int c[MAXD], a[MAXD];   // contributions, magnitudes
    int min1, min2, cst1, cst2, par;
    int m[MAXD], v[MAXD];   // new messages, new V
};

// one check of degree d: v / m = V and old message per edge
C3REF void check(const Params &p, bool first, int d, const int *v, const int *m, Check &k)
{
    int neg = 0;
    k.min1 = k.min2 = 127;
    for (int j = 0; j < d; j++) {
        const int c = contrib(v[j], m[j]);
        const int a = mag(first || p.nms, c, p.msg_max);
        k.c[j] = c;
        k.a[j] = a;
        neg ^= (c < 0);
        k.min2 = imin(k.min2, imax(a, k.min1));
        k.min1 = imin(k.min1, a);
    }
    k.cst1 = cst(p, k.min2);
    k.cst2 = cst(p, k.min1);
    k.par = neg ^ (d & 1);
    for (int j = 0; j < d; j++) {
        const int r = k.a[j] == k.min1 ? k.cst1 : k.cst2;
        k.m[j] = message(k.c[j], r, k.par);
        k.v[j] = new_v(k.c[j], k.m[j]);
    }
}

// ---- the pieces the kernel's functions compute, each from the definitions above

// the message record: a 2-bit code per edge (bit 0: c < 0, bit 1: the edge got
// cst2) and the signed constants eps * cst1, eps * cst2 (eps = -1: odd parity)
C3REF int msg_of_code(int code, int ec1, int ec2) { return (code & 1) ? -((code & 2) ? ec2 : ec1) : ((code & 2) ? ec2 : ec1); }

// the staircase chain step of a first-group check, as the o edge's new V of
// the whole check: y = the x edge's V (the chain input), mx / co = the x
// edge's old message / the o edge's contribution, tmin = the clipped smallest
// magnitude of the information edges (so that the minimum over the edges
// other than o is min(tmin, a_x)), eps = +1 / -1: the sign parity of the
// information edges with the odd-degree flip
C3REF int chain_step(const Params &p, int y, int mx, int co, int tmin, int eps)
{
    const int cx = contrib(y, mx);
    const int ax = imin(iabs(cx), p.msg_max);
    const int r = cst(p, imin(imin(tmin, p.msg_max), ax));   // o excluded: the minimum of the others
    // parity of the whole check without o's own sign = eps's * sign(c_x)
    const int others_neg = (eps < 0) != (cx < 0);
    return new_v(co, others_neg ? -r : r);
}

// hard-decision bit helpers of the early-termination kernels
C3REF unsigned pos_bits(unsigned d)
{
    unsigned o = 0;
    for (int j = 0; j < 4; j++) {
        const int b = (int)(signed char)((d >> (8 * j)) & 0xFF);
        if (b > 0) o |= 0x80u << (8 * j);
    }
    return o;
}
C3REF unsigned high_bits16(const unsigned (&x)[4])
{
    unsigned o = 0;
    for (int j = 0; j < 16; j++) o |= ((x[j >> 2] >> (8 * (j & 3) + 7)) & 1u) << j;
    return o;
}
C3REF unsigned row_hbits(const unsigned (&y)[4])
{
    unsigned o = 0;
    for (int j = 0; j < 16; j++) o |= (unsigned)((int)(signed char)((y[j >> 2] >> (8 * (j & 3))) & 0xFF) > 0) << j;
    return o;
}

}  // namespace c3ref
