// awgn_f32.h -- the float AWGN channel's generator, one definition for the host
// twin (code.cpp: ldpc_awgn_f32_host) and the device kernel (awgn_f32_k,
// layout.hip).  It stands where the reference draws its noise with MKL
// (CChanelAWGN_MKL::generate, code/x86/CChanel/CChanelAWGN_MKL.cpp:127-143).
//
// Element i of codeword cw of an N-bit code:
//   idx = cw * N + i                                           (64-bit)
//   u   = splitmix64(idx ^ (seed * 0xD1B54A32D192ED03)) >> 32  (the int8 channel's u)
//   z   = Phi^-1((u + 0.5) * 2^-32)
//   t   = norm * (-amp + sigma * z)                            (double, this order)
//   y   = (float)t, negated where the codeword bit is 1
//
// Phi^-1 is Wichura's AS241 (PPND16; Applied Statistics 37 (3), 1988), relative
// error about 1e-16.  p >= 2^-33 keeps sqrt(-log p) <= 4.79, so its far-tail
// region (r > 5) is never reached: there are two regions, |p - 0.5| <= 0.425
// and the tail.  32 bits of u bound |z| at 6.34 (the mass cut off is 2^-32).
//
// Host and device must agree bit for bit, so the function calls no libm / ocml
// transcendental: the logarithm is written out (exponent bits + an atanh series
// in the mantissa), and what remains is integer work and IEEE double + - * /
// and sqrt, each correctly rounded on both sides.  Nothing may be contracted:
// both builds pass -ffp-contract=off.
//
// Both regions are computed for every sample and the result selected: 15 % of
// the samples are in the tail, so a 64-lane wave practically always holds both
// kinds (0.85^64 = 3e-5) and a branch would run both bodies anyway, each under
// a partial mask; straight-line code lets the compiler interleave the two
// Horner chains and the samples of one lane.  One division serves both regions
// (the numerator and denominator are selected, then divided).
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define LDPC_HD __host__ __device__ inline
#else
#define LDPC_HD inline
#endif

#define AWGN_KEY_MUL 0xD1B54A32D192ED03ull
#define AWGN_F32_SPLIT 0.425   // |p - 0.5| <= SPLIT: central region, else tail

// u values where the method changes region (tests probe around them): the
// last tail u below the centre, and its mirror image, the last central u
#define AWGN_F32_U_LO 322122546u    // (u + 0.5) * 2^-32 - 0.5 < -0.425 up to here
#define AWGN_F32_U_HI 3972844748u   // 2^32 - 1 - (U_LO + 1)

LDPC_HD uint64_t awgn_splitmix64(uint64_t x)
{
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

LDPC_HD uint32_t awgn_u(uint64_t idx, uint64_t key) { return (uint32_t)(awgn_splitmix64(idx ^ key) >> 32); }

// natural logarithm of a normal positive double, to about 1e-16 relative:
// x = m * 2^e with m in [sqrt(1/2), sqrt(2)), log m = 2 atanh(s), s = (m-1)/(m+1),
// |s| <= 0.1716: the series is cut after s^23 / 23 (next term < 4e-20)
LDPC_HD double awgn_log(double x)
{
    uint64_t b;
    memcpy(&b, &x, 8);
    int e = (int)(b >> 52) - 1023;
    uint64_t frac = b & 0x000FFFFFFFFFFFFFull;
    const int up = frac > 0x0006A09E667F3BCDull;   // m > sqrt(2): halve it
    e += up;
    b = frac | ((uint64_t)(1023 - up) << 52);
    double m;
    memcpy(&m, &b, 8);
    const double s = (m - 1.0) / (m + 1.0), w = s * s;
    double h = 1.0 / 23.0;
    h = h * w + 1.0 / 21.0;
    h = h * w + 1.0 / 19.0;
    h = h * w + 1.0 / 17.0;
    h = h * w + 1.0 / 15.0;
    h = h * w + 1.0 / 13.0;
    h = h * w + 1.0 / 11.0;
    h = h * w + 1.0 / 9.0;
    h = h * w + 1.0 / 7.0;
    h = h * w + 1.0 / 5.0;
    h = h * w + 1.0 / 3.0;
    h = h * w + 1.0;
    return (double)e * 0.69314718055994530942 + 2.0 * s * h;
}

// z = Phi^-1((u + 0.5) * 2^-32); exactly antisymmetric in u <-> 2^32 - 1 - u
// (p - 0.5 and min(p, 1 - p) are exact), non-decreasing in u
LDPC_HD double awgn_normal(uint32_t u)
{
    const double p = ((double)u + 0.5) * (1.0 / 4294967296.0);
    const double q = p - 0.5;
    const double aq = q < 0.0 ? -q : q;
    // central region
    const double rc = 0.180625 - q * q;
    double nc = 2.5090809287301226727e+3;
    nc = nc * rc + 3.3430575583588128105e+4;
    nc = nc * rc + 6.7265770927008700853e+4;
    nc = nc * rc + 4.5921953931549871457e+4;
    nc = nc * rc + 1.3731693765509461125e+4;
    nc = nc * rc + 1.9715909503065514427e+3;
    nc = nc * rc + 1.3314166789178437745e+2;
    nc = nc * rc + 3.3871328727963666080e+0;
    nc = nc * q;
    double dc = 5.2264952788528545610e+3;
    dc = dc * rc + 2.8729085735721942674e+4;
    dc = dc * rc + 3.9307895800092710610e+4;
    dc = dc * rc + 2.1213794301586595867e+4;
    dc = dc * rc + 5.3941960214247511077e+3;
    dc = dc * rc + 6.8718700749205790830e+2;
    dc = dc * rc + 4.2313330701600911252e+1;
    dc = dc * rc + 1.0;
    // tail: r = sqrt(-log(min(p, 1 - p))) - 1.6, r + 1.6 in (0.83, 4.79)
    const double pm = q < 0.0 ? p : 1.0 - p;
    const double rt = sqrt(-awgn_log(pm)) - 1.6;
    double nt = 7.74545014278341407640e-4;
    nt = nt * rt + 2.27238449892691845833e-2;
    nt = nt * rt + 2.41780725177450611770e-1;
    nt = nt * rt + 1.27045825245236838258e+0;
    nt = nt * rt + 3.64784832476320460504e+0;
    nt = nt * rt + 5.76949722146069140550e+0;
    nt = nt * rt + 4.63033784615654529590e+0;
    nt = nt * rt + 1.42343711074968357734e+0;
    nt = q < 0.0 ? -nt : nt;
    double dt = 1.05075007164441684324e-9;
    dt = dt * rt + 5.47593808499534494600e-4;
    dt = dt * rt + 1.51986665636164571966e-2;
    dt = dt * rt + 1.48103976427480074590e-1;
    dt = dt * rt + 6.89767334985100004550e-1;
    dt = dt * rt + 1.67638483018380384940e+0;
    dt = dt * rt + 2.05319162663775882187e+0;
    dt = dt * rt + 1.0;
    const bool central = aq <= AWGN_F32_SPLIT;
    return (central ? nc : nt) / (central ? dc : dt);
}

// the sample for bit 0 (sent as -amp); a codeword bit of 1 negates it
LDPC_HD float awgn_f32_sample(uint64_t idx, uint64_t key, double sigma, double amp, double norm)
{
    const double z = awgn_normal(awgn_u(idx, key));
    return (float)(norm * (-amp + sigma * z));
}
