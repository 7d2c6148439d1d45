// pk_i8.h -- the int8 contract (lds.hip lds_check_i8, kernels_common.h
// check_constants) on a 32-bit pair of codewords: the per-edge functions of the
// edge-parallel int8 kernel (ldsepi.hip).  A pair holds two codewords, the even
// one in the low half, each value as a plain sign-extended i16.
//
// Every function is __host__ __device__: the device compiles the vector
// operations to v_pk_*_i16 / _u16, the host to two scalar lanes, and
// tests/cpp/ldsepi_arith_probe.cpp holds the host form to the reference's
// sat8 / abs8 / subs_u8 / nms_scale over whole domains (tests/test_i8_ep_cpu.py).
//
// Why the int8 operations are exact in i16, inside the kernel's domain
// (var_min in -127 .. 0, msg_max in 0 .. 127, offset in 0 .. 255):
// * V in -128 .. 127, m in -127 .. 127: V - m and c + m lie in -255 .. 254, so
//   the i16 difference / sum never wraps and sat8 is min(., 127) and max(., -128);
//   the lower clamp is absorbed by max(., var_min) since var_min >= -127;
// * c >= -127, so abs8 never meets -128 and |t| = max(t, 0 - t);
// * a magnitude e is 0 .. 127: subs_u8(e, offset) is the saturating u16
//   difference, as_i8 of it is the identity, and (e * factor mod 2^16) >> 5 is
//   at most 2047 -- nms_scale's int16 reinterpretation never sees a sign bit, so
//   its clamp is min(., 127).
#pragma once
#include <stdint.h>

#if defined(__HIP__) || defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define PKI8_FN __host__ __device__ __forceinline__
#else
#define PKI8_FN inline
#endif

namespace pki8 {

typedef short s2_t __attribute__((ext_vector_type(2)));
typedef unsigned short u2_t __attribute__((ext_vector_type(2)));

constexpr uint32_t K127 = 0x007F007Fu;     // 127 per half
constexpr uint32_t KN127 = 0xFF81FF81u;    // -127 per half

PKI8_FN s2_t as_s2(uint32_t u) { return __builtin_bit_cast(s2_t, u); }
PKI8_FN uint32_t s2_u(s2_t v) { return __builtin_bit_cast(uint32_t, v); }
PKI8_FN u2_t as_u2(uint32_t u) { return __builtin_bit_cast(u2_t, u); }
PKI8_FN uint32_t u2_u(u2_t v) { return __builtin_bit_cast(uint32_t, v); }

PKI8_FN uint32_t pk_add(uint32_t a, uint32_t b) { return s2_u(as_s2(a) + as_s2(b)); }
PKI8_FN uint32_t pk_sub(uint32_t a, uint32_t b) { return s2_u(as_s2(a) - as_s2(b)); }
PKI8_FN uint32_t pk_min(uint32_t a, uint32_t b) { return s2_u(__builtin_elementwise_min(as_s2(a), as_s2(b))); }
PKI8_FN uint32_t pk_max(uint32_t a, uint32_t b) { return s2_u(__builtin_elementwise_max(as_s2(a), as_s2(b))); }
PKI8_FN uint32_t pk_sra15(uint32_t a) { return s2_u(as_s2(a) >> (short)15); }
PKI8_FN uint32_t pk_subs_u(uint32_t a, uint32_t b) { return u2_u(__builtin_elementwise_sub_sat(as_u2(a), as_u2(b))); }
PKI8_FN uint32_t pk_mul_lo(uint32_t a, uint32_t b) { return u2_u(as_u2(a) * as_u2(b)); }
PKI8_FN uint32_t pk_lshr5(uint32_t a) { return u2_u(as_u2(a) >> (unsigned short)5); }

// the same i16 value x in both halves
PKI8_FN uint32_t splat(int x) { return ((uint32_t)x & 0xFFFFu) * 0x00010001u; }
// two int8 values as a pair
PKI8_FN uint32_t pair(int lo, int hi) { return ((uint32_t)lo & 0xFFFFu) | ((uint32_t)hi << 16); }
PKI8_FN int half_lo(uint32_t x) { return (int)(int16_t)(uint16_t)x; }
PKI8_FN int half_hi(uint32_t x) { return (int)(int16_t)(uint16_t)(x >> 16); }

// contribution c = max(sat8(V - m), var_min): hi = 127, lo = var_min per half.
// (The kernel's padding lanes pass hi = lo = -127: a constant negative
// contribution of magnitude 127, whatever they load.)
PKI8_FN uint32_t contribution(uint32_t v, uint32_t m, uint32_t hi, uint32_t lo)
{
    return pk_max(pk_min(pk_sub(v, m), hi), lo);
}

// magnitude under both rules as one expression, a = min(|min(c, x)|, y):
//   first degree group  a = min(|c|, msg_max):  x = 127 (no-op, c <= 127), y = msg_max
//   later groups        a = |min(c, msg_max)|:  x = msg_max, y = 127 (no-op, c >= -127)
PKI8_FN uint32_t mag_x(bool later, uint32_t msg_max2) { return later ? msg_max2 : K127; }
PKI8_FN uint32_t mag_y(bool later, uint32_t msg_max2) { return later ? K127 : msg_max2; }
PKI8_FN uint32_t magnitude(uint32_t c, uint32_t x, uint32_t y)
{
    const uint32_t t = pk_min(c, x);
    return pk_min(pk_max(t, pk_sub(0u, t)), y);
}

// the constant from an exclusive minimum e (0 .. 127 per half)
// OMS / MS: min(subs_u8(e, offset), msg_max), offset 0 .. 255 per half of off2
PKI8_FN uint32_t cst_oms(uint32_t e, uint32_t off2, uint32_t msg_max2) { return pk_min(pk_subs_u(e, off2), msg_max2); }
// NMS: nms_scale(e, factor), factor mod 2^16 per half of f2; clamped at 127, not at msg_max
PKI8_FN uint32_t cst_nms(uint32_t e, uint32_t f2) { return pk_min(pk_lshr5(pk_mul_lo(e, f2)), K127); }

// message: -r where the sign bit (15 / 31) of sx is set, else r
PKI8_FN uint32_t message(uint32_t r, uint32_t sx)
{
    const uint32_t s = pk_sra15(sx);
    return pk_sub(r ^ s, s);
}

// V' = max(sat8(c + m'), var_min)
PKI8_FN uint32_t new_v(uint32_t c, uint32_t m, uint32_t lo) { return pk_max(pk_min(pk_add(c, m), K127), lo); }

// hard decisions V > 0: bit 0 the low half, bit 1 the high
PKI8_FN uint32_t pos2(uint32_t x) { return (half_lo(x) > 0 ? 1u : 0u) | (half_hi(x) > 0 ? 2u : 0u); }

}  // namespace pki8
