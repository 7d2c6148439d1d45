// pk_f16.h -- the half contract on a 32-bit pair of binary16
// values: what the packed binary16 kernels share (stairh_kernel.h,
// ldsh_kernel.h, generich.hip).  A pair holds two codewords, the even one in
// the low half.
// * + and - are v_pk_add_f16 (neg modifiers), NMS's product v_pk_mul_f16, each
//   rounded to nearest even per half -- the contract's (+) (-) (x);
// * min / max of magnitudes and the clamps are v_pk_min_f16 / v_pk_max_f16
//   (exact; the operands are never NaN inside the contract);
// * |c| clears bits 15 and 31; the sign of a contribution IS its sign bit, so
//   the parity of a check is the XOR of the pairs and a message gets its sign by
//   a bit-field insert -- no per-half compare anywhere;
// * non-negative binary16 orders as u16, so with M1 <= M2 the two smallest
//   magnitudes of a check, (M1 + M2) - min_u16(a_j, M2) in packed u16
//   arithmetic is M2 where a_j == M1 and M1 elsewhere (a_j > M1 implies
//   a_j >= M2) -- what the serial decode's "a_j == min1 ? min2 : min1" picks.
#pragma once
#include "kernels_common.h"

namespace pkf16 {

typedef _Float16 h2_t __attribute__((ext_vector_type(2)));
typedef unsigned short u2_t __attribute__((ext_vector_type(2)));

constexpr uint32_t ABS2 = 0x7FFF7FFFu, SGN2 = 0x80008000u;
constexpr uint32_t INF2 = 0x7C007C00u, NINF2 = 0xFC00FC00u;
constexpr uint32_t VSAT2 = 0x64006400u, NVSAT2 = 0xE400E400u;   // +-1024
constexpr uint32_t MSAT2 = 0x5C005C00u;                         // 256

LDPC_DEV h2_t as_h2(uint32_t u) { return __builtin_bit_cast(h2_t, u); }
LDPC_DEV uint32_t h2_u(h2_t h) { return __builtin_bit_cast(uint32_t, h); }
LDPC_DEV u2_t as_u2(uint32_t u) { return __builtin_bit_cast(u2_t, u); }
LDPC_DEV uint32_t u2_u(u2_t h) { return __builtin_bit_cast(uint32_t, h); }

LDPC_DEV uint32_t pk_add(uint32_t a, uint32_t b) { return h2_u(as_h2(a) + as_h2(b)); }
LDPC_DEV uint32_t pk_sub(uint32_t a, uint32_t b) { return h2_u(as_h2(a) - as_h2(b)); }
LDPC_DEV uint32_t pk_mul(uint32_t a, uint32_t b) { return h2_u(as_h2(a) * as_h2(b)); }
LDPC_DEV uint32_t pk_min(uint32_t a, uint32_t b) { return h2_u(__builtin_elementwise_min(as_h2(a), as_h2(b))); }
LDPC_DEV uint32_t pk_max(uint32_t a, uint32_t b) { return h2_u(__builtin_elementwise_max(as_h2(a), as_h2(b))); }
LDPC_DEV uint32_t pk_abs(uint32_t a) { return h2_u(__builtin_elementwise_abs(as_h2(a))); }   // clears bits 15 and 31
LDPC_DEV uint32_t pk_addu(uint32_t a, uint32_t b) { return u2_u(as_u2(a) + as_u2(b)); }
LDPC_DEV uint32_t pk_subu(uint32_t a, uint32_t b) { return u2_u(as_u2(a) - as_u2(b)); }
LDPC_DEV uint32_t pk_minu(uint32_t a, uint32_t b) { return u2_u(__builtin_elementwise_min(as_u2(a), as_u2(b))); }

// V's saturation: min(max(x, -VSAT), VSAT)
LDPC_DEV uint32_t clamp_v(uint32_t x) { return pk_min(pk_max(x, NVSAT2), VSAT2); }
// magnitude r (sign bits clear) with the sign bits of s
LDPC_DEV uint32_t with_sign(uint32_t r, uint32_t s) { return (r & ABS2) | (s & SGN2); }

// A: 0 OMS, 1 NMS, 2 plain min-sum (beta16 = 0: max(x - 0, +0) = x for x >= +0)
template <int A>
LDPC_DEV uint32_t cst(uint32_t x, uint32_t beta2)
{
    if constexpr (A == 1)
        return pk_min(pk_mul(x, beta2), MSAT2);
    else if constexpr (A == 2)
        return pk_min(x, MSAT2);
    else
        return pk_min(pk_max(pk_sub(x, beta2), 0u), MSAT2);
}

// ---- what the kernels with early termination inside the wave add (ldsh, generich)

// hard decisions of the two halves, V > 0 as binary16 comparisons (+-0 give 0): bit 0 the low half, bit 1 the high
LDPC_DEV uint32_t pos2(uint32_t x)
{
    const h2_t v = as_h2(x);
    return (v[0] > (_Float16)0.0f ? 1u : 0u) | (v[1] > (_Float16)0.0f ? 2u : 0u);
}

// store the pair under a per-half mask (0xFFFF per live half; a lane with no live half does not get here):
// the whole pair, or the one live half as a 16-bit store, so a stopped codeword's state stays frozen.
// WHOLE: the caller knows (wave-uniformly) that every lane's mask is full, and the store is a plain one
template <bool WHOLE>
LDPC_DEV void put2(uint32_t *p, uint32_t x, uint32_t mask)
{
    if (WHOLE || mask == 0xFFFFFFFFu)
        *p = x;
    else if (mask & 1u)
        *(uint16_t *)p = (uint16_t)x;
    else
        ((uint16_t *)p)[1] = (uint16_t)(x >> 16);
}

}  // namespace pkf16
