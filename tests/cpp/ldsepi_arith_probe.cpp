// ldsepi_arith_probe.cpp -- libldsepi_probe.so: the per-edge functions of the
// edge-parallel int8 kernel (csrc/pk_i8.h) compiled for the host and exposed on
// arrays of 32-bit pairs (two codewords: int8 values as sign-extended i16
// halves).  tests/test_i8_ep_cpu.py compares them with a numpy restatement of the
// reference's sat8 / abs8 / subs_u8 / nms_scale over whole domains.  Built by
// csrc/Makefile; not linked into the library.  Constants (var_min, msg_max,
// offset, factor) come as pairs too, so the two halves may differ.
#include "../../ldpcgputegra_amd/csrc/pk_i8.h"

extern "C" {

// c = max(sat8(V - m), var_min); hi: 127 per half, lo: var_min per half
void pki8_contribution(const uint32_t *v, const uint32_t *m, uint32_t hi, uint32_t lo, uint32_t *out, long n)
{
    for (long i = 0; i < n; i++) out[i] = pki8::contribution(v[i], m[i], hi, lo);
}

// later = 0: min(|c|, msg_max); later = 1: |min(c, msg_max)|
void pki8_magnitude(const uint32_t *c, int later, uint32_t msg_max2, uint32_t *out, long n)
{
    const uint32_t x = pki8::mag_x(later != 0, msg_max2), y = pki8::mag_y(later != 0, msg_max2);
    for (long i = 0; i < n; i++) out[i] = pki8::magnitude(c[i], x, y);
}

// the same with the two bounds given: min(|min(c, x)|, y) (a padding lane takes the rule's x and y = 127)
void pki8_magnitude_xy(const uint32_t *c, uint32_t x, uint32_t y, uint32_t *out, long n)
{
    for (long i = 0; i < n; i++) out[i] = pki8::magnitude(c[i], x, y);
}

void pki8_cst_oms(const uint32_t *e, uint32_t off2, uint32_t msg_max2, uint32_t *out, long n)
{
    for (long i = 0; i < n; i++) out[i] = pki8::cst_oms(e[i], off2, msg_max2);
}

void pki8_cst_nms(const uint32_t *e, uint32_t f2, uint32_t *out, long n)
{
    for (long i = 0; i < n; i++) out[i] = pki8::cst_nms(e[i], f2);
}

// -r where bit 15 / 31 of sx is set, else r
void pki8_message(const uint32_t *r, const uint32_t *sx, uint32_t *out, long n)
{
    for (long i = 0; i < n; i++) out[i] = pki8::message(r[i], sx[i]);
}

void pki8_new_v(const uint32_t *c, const uint32_t *m, uint32_t lo, uint32_t *out, long n)
{
    for (long i = 0; i < n; i++) out[i] = pki8::new_v(c[i], m[i], lo);
}

void pki8_pos2(const uint32_t *x, uint32_t *out, long n)
{
    for (long i = 0; i < n; i++) out[i] = pki8::pos2(x[i]);
}

}  // extern "C"
