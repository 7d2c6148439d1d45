"""coop3's packed 16-bit arithmetic on the device, over whole input domains.

libc3probe.so (tests/cpp/coop3_arith_probe.hip, built by csrc/Makefile from
the kernel's own headers) calls the production device functions of pk16.h and
coop3_kernel.h and compares each result, bit for bit, with the scalar
reference tests/cpp/coop3_arith_ref.h, which test_coop3_arith_ref_cpu.py pins
against the oracle.  Large products are reduced on the device (mismatch count
and the first 16 tuples); small ones also come back and are compared in numpy
with the scalar statement and with test_coop2_arith.py's instruction
emulation, which certifies that emulation against the hardware.  In every
dword the two halves carry different tuples (tuple i and tuple N - 1 - i).
"""
import ctypes as C
import os

import numpy as np
import pytest

import test_coop2_arith as A2

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
_lib = None


def probe():
    global _lib
    if _lib is None:
        _lib = C.CDLL(os.path.join(ROOT, "ldpcgputegra_amd", "libc3probe.so"))
    return _lib


def run(name, fields, *args):
    """Call a reducing probe; fail with `function, tuple, got, expected` of the first mismatches."""
    n = C.c_ulonglong(0)
    tup = np.zeros((16, 8), np.int32)
    rc = getattr(probe(), name)(*args, C.byref(n), C.c_void_p(tup.ctypes.data))
    assert rc == 0, "%s: HIP error %d" % (name, rc)
    if n.value:
        rows = ["  " + ", ".join("%s=%s" % (f, hex(int(v) & 0xFFFFFFFF) if f.startswith(("got", "exp")) else int(v))
                                 for f, v in zip(fields, t)) for t in tup[:min(16, n.value)]]
        pytest.fail("%s%s: %d mismatches; the first:\n%s" % (name, args, n.value, "\n".join(rows)))


def ptr(a):
    return C.c_void_p(a.ctypes.data)


def halves(x):
    x = np.asarray(x, np.int64)
    return x & 0xFFFF, (x >> 16) & 0xFFFF


def R(x):
    return (256 * np.asarray(x, np.int64) + 255) & 0xFFFF


def Cf(m):
    return (256 * np.asarray(m, np.int64)) & 0xFFFF


# ---- message decode ---------------------------------------------------------
@pytest.mark.parametrize("nma", [1, 2, 4])
def test_message_decode(nma):
    """msg_tab, old_msg<J> (J = 0 .. 7, with NMA = 1) and old_msg2<J, NMA> for
    every slot J < 8 NMA (degrees 7 .. 30 use slots 0 .. 13; the HALF records
    14 / 15): all 4 codes of slot J in both halves x every (cst1, cst2) in
    -63 .. 63, the other slots all-zero, all-ones and a fixed pattern.  The
    result is C(+-cst), low byte 0."""
    run("c3p_msg", ("J", "fill", "code", "cst1", "cst2", "got", "exp", "got_old_msg"), nma)


# ---- contribution, magnitude -------------------------------------------------
def test_contribution_and_magnitude():
    """pk_sub_sat, abs_sat, abs_r (of the contribution clamped at R(-127)):
    every V -128 .. 127 x every message -63 .. 63, the 0x8000 result
    included; the values come back and are compared with the scalar statement
    and with test_coop2_arith's instruction emulation."""
    n = 256 * 127
    c, a_s, a_r = (np.zeros(n, np.uint32) for _ in range(3))
    run("c3p_contrib", ("function(0 c,1 abs_sat,2 max,3 abs_r)", "half", "V", "m", "got", "exp"), ptr(c), ptr(a_s), ptr(a_r))
    i = np.arange(n)
    v, m = i // 127 - 128, i % 127 - 63
    d = v - m
    for h, (vv, mm, dd) in enumerate(((v, m, d), (v[::-1], m[::-1], d[::-1]))):
        ec = np.where(dd < -128, 0x8000, R(np.clip(dd, -128, 127)))
        ea = R(np.minimum(np.abs(dd), 127))
        for name, got, exp in (("pk_sub_sat", c, ec), ("abs_sat", a_s, ea), ("abs_r", a_r, ea)):
            g = halves(got)[h]
            bad = np.flatnonzero(g != exp)
            assert bad.size == 0, "%s half %d (V, m) = (%d, %d): got %#x, expected %#x" % (
                name, h, vv[bad[0]], mm[bad[0]], g[bad[0]], exp[bad[0]])
    Rp, Cp = A2.join(R(v), R(v[::-1])), A2.join(Cf(m), Cf(m[::-1]))
    ce = A2.pk_sub_sat(Rp, Cp)
    assert np.array_equal(ce, c), "emulated pk_sub_sat differs from the device"
    assert np.array_equal(A2.abs_sat(ce), a_s), "emulated abs_sat differs from the device"
    assert np.array_equal(A2.abs_r(A2.pk_max(ce, A2.RNEG127)), a_r), "emulated abs_r differs from the device"


def test_v_pairs_round_trip():
    """unpack_v with both selectors (the pair in the low / high u16 of a V
    dword, the other u16 its complement), pack_v of the result, Slab3::x_of:
    all 65536 pairs."""
    un, pk = np.zeros(2 * 65536, np.uint32), np.zeros(2 * 65536, np.uint32)
    run("c3p_vpack", ("function(0 unpack_v,1 pack_v,2 x_of)", "dword_half", "raw", "-", "got", "exp"), ptr(un), ptr(pk))
    raw = np.arange(65536)
    b0, b1 = ((raw & 0xFF) ^ 0x80) - 0x80, ((raw >> 8) ^ 0x80) - 0x80
    exp = R(b0) | (R(b1) << 16)
    for hi in (0, 1):
        assert np.array_equal(un[hi * 65536:][:65536], exp), "unpack_v, pair in u16 %d" % hi
        assert np.array_equal(pk[hi * 65536:][:65536], raw), "pack_v(unpack_v), pair in u16 %d" % hi
    assert np.array_equal(A2.unpack_v(raw), un[:65536]), "emulated unpack_v differs from the device"
    assert np.array_equal(A2.pack_v(un[:65536].astype(np.int64)), pk[:65536]), "emulated pack_v differs from the device"


# ---- constants ------------------------------------------------------------
@pytest.mark.parametrize("odd", [0, 1], ids=["even", "odd"])
@pytest.mark.parametrize("nms", [0, 1], ids=["oms", "nms"])
def test_constants(nms, odd):
    """post_finish (cx, ax, min1, min2, k1, k2, e1, e2), the tail check's k1 /
    k2 / signed_csts form, nms_v, nms_c: every min 0 .. 127 (entering as |c_x|,
    as mn1 and as mn2) x msg_max 0 .. 63 x offset 0 .. 63 (offset 0 = MS) or
    factor 0 .. 64 x both parities x both signs of c_x."""
    run("c3p_consts", ("function(0 post_finish,1 tail,2 nms_v,3 nms_c)", "half", "min", "msg_max", "param",
                       "parity|form<<1|sign<<3", "got_e1|e2<<16", "exp_e1|e2<<16"), nms, odd)


def test_signed_csts():
    """signed_csts: every k1, k2 in 0 .. 127 x both parities (other bits of
    the parity word set or clear); also against the emulation's multiply form."""
    n = 128 * 128 * 2
    e = np.zeros(2 * n, np.uint32)
    run("c3p_signed", ("half", "k1", "k2", "parity", "got_e1", "got_e2"), ptr(e))
    i = np.arange(n)
    k1, k2, p = i % 128, i // 128 % 128, i // (128 * 128)
    par = A2.join(np.where(p == 1, 0x8000, 0x7FFF), np.where(p[::-1] == 1, 0xFFFF, 0))
    e1, e2 = A2.signed_csts(A2.join(Cf(k1), Cf(k1[::-1])), A2.join(Cf(k2), Cf(k2[::-1])), par, 0)
    assert np.array_equal(e1, e[0::2]) and np.array_equal(e2, e[1::2]), "emulated signed_csts differs from the device"
    assert np.array_equal(halves(e[0::2])[0], Cf(np.where(p == 1, -k1, k1)))
    assert np.array_equal(halves(e[1::2])[1], Cf(np.where(p == 1, -k2, k2))[::-1])


# ---- new V and codes ----------------------------------------------------
@pytest.mark.parametrize("fill", [0, 1], ids=["ma0", "ma1"])
@pytest.mark.parametrize("mm", [-1, 0, 1, 31, 62, 63], ids=["first", "later0", "later1", "later31", "later62", "later63"])
def test_new_v_and_codes(mm, fill):
    """new_v<J>, msg_code<J>, add_code<J> (first group) and new_v_later<J>
    (a = |min(c, msg_max)|), J = 0 .. 7: every contribution x every min1 <= a x
    every cst2 <= cst1 <= 63 x eps +-1, MA starting from zero and from all-ones
    in the other slots.  The contribution is enumerated by V - m = -191 .. 190,
    every value pk_sub_sat can see, each realised by one (V, m) with V at its
    clamp; test_contribution_and_magnitude covers every (V, m) that leads to
    it.  Nothing else is thinned."""
    run("c3p_newv", ("J", "V-m", "min1", "cst1|cst2<<8", "eps", "got_v|ma<<16", "exp_v|ma<<16", "got_msg_code|add_code<<16"),
        mm, fill)


# ---- min tracking ---------------------------------------------------------
def min_tuples(X):
    vals = [0, 1, 62, 63, 64, 126, 127]
    rows = [(p1, p2, s1, s2, oth) for p1 in range(X) for p2 in range(X) if p1 != p2
            for s1 in vals for s2 in vals if s2 >= s1 for oth in sorted({s2, min(s2 + 1, 127), 127})]
    return np.ascontiguousarray(rows, np.int32)


@pytest.mark.parametrize("d0", [7, 10, 14, 22, 27, 30])
def test_min_tracking(d0):
    """min_track / min_merge2 as the pre runs them (one chain below 8 edges,
    two interleaved chains from 8) and Slab3::merge (degrees 22 .. 30: the
    edges split over two lanes as G3::XH, sinks at R(127), r8/9's three
    included): the two smallest at every ordered pair of positions, equal and
    unequal, equal to R(127), every other edge tied with the second, one
    above it, or R(127); signs from a hash of the tuple.  Expected: the exact
    two smallest and the xor of the signs."""
    t = min_tuples(d0 - 2)
    run("c3p_min", ("degree", "tuple", "lane_half", "got_min1", "got_min2", "got_sign", "exp_min1|min2<<16", "exp_sign"),
        d0, ptr(t), len(t))


# ---- the chain step -----------------------------------------------------
CHAIN_FIELDS = ("Y", "m_x", "c_o", "eps", "tmin", "param", "got", "exp")


@pytest.mark.parametrize("full", [0, 1], ids=["set", "fullrange"])
@pytest.mark.parametrize("pos", range(8))
@pytest.mark.parametrize("pf2", [0, 1], ids=["pf1", "pf2"])
@pytest.mark.parametrize("nms", [0, 1], ids=["oms", "nms"])
def test_chain_step(nms, pf2, pos, full):
    """chain_consts -> the record packing -> chain_window3 (16 steps, both
    prefetch forms) -> xo and the final w, with the record at position `pos`
    of the first block and pass-through records elsewhere: every Y -127 .. 127
    x m_x -63 .. 63 x c_o -127 .. 127 x eps +-1 x clipped-min and offset /
    factor over {0, 1, 2, 30, 31, 32, 62, 63(, 64)} (set), or c_o in {-127,
    -1, 0, 1, 127} x every clipped-min 0 .. 63 x every offset / factor
    (fullrange); msg_max 63.  Expected: the o edge's new V of the whole check,
    Y in xo up to the position and the output after it."""
    run("c3p_chain", CHAIN_FIELDS, nms, pf2, pos, 63, 0, full)


@pytest.mark.parametrize("mm", [0, 1, 31])
@pytest.mark.parametrize("nms", [0, 1], ids=["oms", "nms"])
def test_chain_step_clips_the_minimum(nms, mm):
    """The same product with msg_max below the minimum's range: chain_consts
    clips it (second block, position 11, prefetch form of degree 10)."""
    run("c3p_chain", CHAIN_FIELDS, nms, 1, 11, mm, 0, 0)


@pytest.mark.parametrize("kind", [1, 2, 3], ids=["tail", "pass", "frozen"])
@pytest.mark.parametrize("pos", [0, 7, 8, 15])
@pytest.mark.parametrize("nms", [0, 1], ids=["oms", "nms"])
def test_chain_records(nms, pos, kind):
    """The tail record (output = the tail's V), pass-through records alone
    (output = Y) and the FZ override (output = the V as read)."""
    run("c3p_chain", CHAIN_FIELDS, nms, pos & 1, pos, 63, kind, 0)


# ---- early-termination bit helpers -------------------------------------
def test_et_bit_helpers():
    """pos_bits, high_bits16, row_hbits: every byte value in every byte
    position over zeros and over ones, then 2^16 random rows."""
    rows = []
    for bg in (0, 0xFF):
        for posn in range(16):
            r = np.full((256, 16), bg, np.uint8)
            r[:, posn] = np.arange(256)
            rows.append(r)
    rng = np.random.default_rng(3)
    rows.append(rng.integers(0, 256, (1 << 16, 16), dtype=np.uint8))
    x = np.ascontiguousarray(np.concatenate(rows)).view(np.uint32).reshape(-1, 4)
    n = len(x)
    pb, hb, rb = (np.zeros(n, np.uint32) for _ in range(3))
    run("c3p_bits", ("function(0 pos_bits,1 high_bits16,2 row_hbits)", "row", "x", "y", "z", "w", "got", "exp"),
        ptr(x), n, ptr(pb), ptr(hb), ptr(rb))
    by = x.view(np.uint8).reshape(n, 16)
    w = (1 << np.arange(16)).astype(np.int64)
    assert np.array_equal(rb, ((by.view(np.int8) > 0) * w).sum(axis=1))
    assert np.array_equal(hb, ((by >> 7) * w).sum(axis=1))
    assert np.array_equal(pb, (((by[:, :4].view(np.int8) > 0) * 0x80).astype(np.int64) << (8 * np.arange(4))).sum(axis=1))
