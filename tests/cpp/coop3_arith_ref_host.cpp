// coop3_arith_ref_host.cpp -- libc3ref_host.so: the scalar reference of
// coop3_arith_ref.h compiled for the host, so that
// tests/test_coop3_arith_ref_cpu.py can pin it against the oracle without a GPU
#include <stdint.h>

#include "coop3_arith_ref.h"

extern "C" {

// n checks of degree d: v, m, v_new, m_new are [n][d] int8
int c3ref_check(int nms, int param, int msg_max, int first, int d, int n, const int8_t *v, const int8_t *m, int8_t *v_new,
                int8_t *m_new)
{
    if (d < 1 || d > c3ref::MAXD) return 1;
    const c3ref::Params p{nms, param, msg_max};
    for (int i = 0; i < n; i++) {
        int vi[c3ref::MAXD], mi[c3ref::MAXD];
        for (int j = 0; j < d; j++) vi[j] = v[(long)i * d + j], mi[j] = m[(long)i * d + j];
        c3ref::Check k;
        c3ref::check(p, first != 0, d, vi, mi, k);
        for (int j = 0; j < d; j++) v_new[(long)i * d + j] = (int8_t)k.v[j], m_new[(long)i * d + j] = (int8_t)k.m[j];
    }
    return 0;
}

// n chain steps: out = the o edge's new V
int c3ref_chain_step(int nms, int param, int msg_max, int n, const int *y, const int *mx, const int *co, const int *tmin,
                     const int *eps, int *out)
{
    const c3ref::Params p{nms, param, msg_max};
    for (int i = 0; i < n; i++) out[i] = c3ref::chain_step(p, y[i], mx[i], co[i], tmin[i], eps[i]);
    return 0;
}

int c3ref_msg_of_code(int code, int ec1, int ec2) { return c3ref::msg_of_code(code, ec1, ec2); }

// n rows of 4 dwords
void c3ref_bits(const uint32_t *in, int n, uint32_t *pb, uint32_t *hb, uint32_t *rb)
{
    for (int i = 0; i < n; i++) {
        const unsigned x[4] = {in[4 * i], in[4 * i + 1], in[4 * i + 2], in[4 * i + 3]};
        pb[i] = c3ref::pos_bits(x[0]);
        hb[i] = c3ref::high_bits16(x);
        rb[i] = c3ref::row_hbits(x);
    }
}
}
