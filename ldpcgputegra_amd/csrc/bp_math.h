// bp_math.h -- the arithmetic of layered belief propagation (sum-product), one
// definition for the host decoder (host.cpp), the device kernels (bp.hip) and
// the introspection entries ldpc_boxplus_f32_host / _async.
//
//   g(x)   ~ ln(1 + e^-x), x >= 0
//   a [+] b = -2 atanh(tanh(a/2) tanh(b/2)) up to this project's sign rule,
//            through the identity
//              | a [+] b | = min(|a|, |b|) + g(|a| + |b|) - g(| |a| - |b| |)
//
// Host and device must agree bit for bit, so nothing here calls
// libm / ocml: g is written out in float +, -, *, comparisons, one float -> int
// conversion and one exponent built from bits, each correctly rounded on both
// sides.  There is no division and no table.  Nothing may be contracted: both
// builds pass -ffp-contract=off.
//
// g: x is cut at BP_G_CUT (from there on g is exactly +0: e^-18 = 1.5e-8 is a
// sixteenth of the error allowed), then
//   k = trunc(x / ln 2 + 0.5)                  0 <= k <= 26
//   r = (x - k * LN2_HI) - k * LN2_LO          |r| <= ln 2 / 2 (+ rounding);
//                                              LN2_HI has 15 significant bits, so
//                                              k * LN2_HI is exact
//   p = E(r) ~ e^-r                            degree 7, Horner
//   u = p * 2^-k = e^-x                        0 < u <= 1 (+ rounding), exact scaling
//   g = u * L(u), L(u) ~ ln(1 + u) / u         degree 8 (degree 9 in all), Horner
// E and L interpolate at the Chebyshev nodes of [-ln 2 / 2, ln 2 / 2] and
// [0, 1] (both widened by rounding slack), coefficients rounded to float.
// The product form makes g follow e^-x with a relative error towards the
// cutoff.  Measured error and the bound it is held to: DESIGN.md §3,
// tests/test_bp_cpu.py.
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define BP_HD __host__ __device__ inline
#else
#define BP_HD inline
#endif

// the loops of bp_check unroll on the device, where the degree is a constant
#if defined(__HIP_DEVICE_COMPILE__)
#define BP_UNROLL _Pragma("unroll")
#else
#define BP_UNROLL
#endif

#define BP_G_CUT 18.0f                 // g(x) = +0 for x >= BP_G_CUT
#define BP_INV_LN2 0x1.715476p+0f      // 1 / ln 2
#define BP_LN2_HI 0x1.62e4p-1f         // ln 2 = HI + LO, HI in 15 bits
#define BP_LN2_LO 0x1.7f7d1cp-20f

BP_HD float bp_from_bits(uint32_t b)
{
    float f;
    __builtin_memcpy(&f, &b, 4);
    return f;
}

BP_HD uint32_t bp_bits(float f)
{
    uint32_t b;
    __builtin_memcpy(&b, &f, 4);
    return b;
}

BP_HD float bp_abs(float x) { return bp_from_bits(bp_bits(x) & 0x7FFFFFFFu); }

// ln(1 + e^-x) for x >= 0 (-0.0 counts as 0)
BP_HD float bp_g(float x)
{
    const float xc = x < BP_G_CUT ? x : BP_G_CUT;
    const int k = (int)(xc * BP_INV_LN2 + 0.5f);
    const float kf = (float)k;
    const float r = (xc - kf * BP_LN2_HI) - kf * BP_LN2_LO;
    float p = -0x1.a18p-13f;
    p = p * r + 0x1.6da9a4p-10f;
    p = p * r + -0x1.1110a4p-7f;
    p = p * r + 0x1.555462p-5f;
    p = p * r + -0x1.555556p-3f;
    p = p * r + 0.5f;
    p = p * r + -1.0f;
    p = p * r + 1.0f;
    const float u = p * bp_from_bits((uint32_t)(127 - k) << 23);
    float q = 0x1.4ff184p-8f;
    q = q * u + -0x1.dc5944p-6f;
    q = q * u + 0x1.3d816ep-4f;
    q = q * u + -0x1.1692ecp-3f;
    q = q * u + 0x1.86b1c8p-3f;
    q = q * u + -0x1.fca104p-3f;
    q = q * u + 0x1.552d74p-2f;
    q = q * u + -0x1.fffe8cp-2f;
    q = q * u + 0x1.fffffep-1f;
    return x < BP_G_CUT ? q * u : 0.0f;
}

// a [+] b.  The sign is this project's: hard = V > 0 reads as bit 1, so every
// combination negates -- chained over the D - 1 other edges of a check it gives
// the odd-degree flip of the min-sum kernels (sign = D & 1).  Zero and -0.0
// count as non-negative, as in check_f32.
BP_HD float bp_boxplus(float a, float b)
{
    const float x = bp_abs(a), y = bp_abs(b);
    const float mn = x < y ? x : y;
    const float d = (mn + bp_g(x + y)) - bp_g(bp_abs(x - y));
    const float r = d > 0.0f ? d : 0.0f;
    return ((a < 0.0f) == (b < 0.0f)) ? -r : r;
}

// One check of degree d (2 .. 32), in place: fm[j] = t_j = V[v_j] - m_j on entry,
// the new message m'_j = [+] of the other edges' t on return, by the forward /
// backward recursion of the definition:
//   F_0 = t_0, F_j = F_{j-1} [+] t_j;  B_{d-1} = t_{d-1}, B_j = t_j [+] B_{j+1};
//   m'_0 = B_1, m'_{d-1} = F_{d-2}, m'_j = F_{j-1} [+] B_{j+1}
// t is left as it was.  With d a compile-time constant after inlining, both
// loops unroll and the arrays live in registers.
__attribute__((always_inline)) BP_HD void bp_check(int d, const float *t, float *fm)
{
    // forward: fm[j] = F_j, j = 0 .. d-2 (fm[0] = t_0 already)
    BP_UNROLL
    for (int j = 1; j < d - 1; j++) fm[j] = bp_boxplus(fm[j - 1], t[j]);
    float B = t[d - 1];
    fm[d - 1] = fm[d - 2];
    BP_UNROLL
    for (int j = d - 2; j >= 1; j--) {
        fm[j] = bp_boxplus(fm[j - 1], B);
        B = bp_boxplus(t[j], B);
    }
    fm[0] = B;
}
