"""The edge-parallel int8 kernel (`ldsepi`, the int8 element type of family 9),
host side: what tests/test_gpu_i8_ep.py rests on.

* the per-edge functions of csrc/pk_i8.h, compiled for the host into
  libldsepi_probe.so (tests/cpp/ldsepi_arith_probe.cpp), against a numpy
  restatement of the reference's sat8 / abs8 / subs_u8 / nms_scale and
  check_constants (csrc/kernels_common.h) over whole domains, with different
  values (and different constants) in the two halves of every pair;
* the host decoder equals the oracle on the kernel's domain, on every table of
  ldsep_domain (hard decisions: all the host int8 entry point returns), so a GPU
  mismatch is a kernel bug;
* the early-termination input of the GPU file holds what its tests need, for
  each of the three algorithms;
* the i8_edge_parallel switch on a host context, the exports, and
  ldpc_ldsepi_params_ok against its restatement."""
import ctypes as C
import os

import numpy as np
import pytest

import ldsep_domain as ED
import oracle as O
import param_domain as PD
from ldpcgputegra_amd import ALGO_BP, ALGO_MS, ALGO_NMS, ALGO_OMS, Code, Decoder, LdpcError, _lib, channel, \
    default_params, load_table

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))

VAR_MINS = (-127, -64, -1, 0)
MSG_MAXS = (0, 1, 31, 63, 127)
OFFSETS = (0, 1, 5, 63, 64, 255)
FACTORS = (0, 1, 26, 29, 32, 33, 64, 65, 255, 65535)

# the parameter sets of the host / GPU comparison: PD.SUBSET inside the kernel's domain, plus the two var_min
# entries at which the padding-lane hazards of an int8 sink would show
DOMAIN = [p for p in PD.SUBSET if p.var_min >= -127] + [PD.Params("OMS", 1, -64, 31), PD.Params("OMS", 1, 0, 31)]
BATCH, ITERS = 17, 3

ET_CODE, ET_BATCH, ET_ITERS, ET_EBN0 = "648x324", 17, 16, 1.5
ET_PARAMS = {"OMS": PD.Params("OMS", 1, -127, 31), "MS": PD.Params("MS", 0, -127, 31),
             "NMS": PD.Params("NMS", 26, -127, 31)}
ET_ITERS_USED = {
    "OMS": [6, 12, 6, 7, 7, 15, 5, 16, 4, 3, 16, 6, 16, 4, 9, 7, 8],
    "MS": [16, 16, 16, 10, 13, 16, 10, 16, 10, 4, 16, 6, 16, 4, 11, 9, 15],
    "NMS": [8, 16, 8, 7, 7, 13, 5, 16, 4, 4, 16, 7, 16, 4, 16, 8, 8],
}
_et = []
_probe = None


def et_input():
    """int8 [17, 648], read-only: AWGN LLRs of 648x324 at 1.5 dB, seed 1"""
    if not _et:
        t = load_table(ET_CODE)
        table = channel.i8_table(channel.sigma_from_ebn0(ET_EBN0, t.k_info / t.n))
        x = channel.awgn_i8_host(t.n, ET_BATCH, seed=1, table=table)
        x.setflags(write=False)
        _et.append(x)
    return _et[0]


# ---- the reference's operations, restated (csrc/kernels_common.h) -------------------

def sat8(x):
    return np.clip(x, -128, 127)


def abs8(x):
    return np.where(x == -128, -128, np.abs(x))


def as_i8(x):
    return (np.asarray(x) & 0xFF).astype(np.uint8).view(np.int8).astype(np.int64)


def subs_u8(a, b):
    return np.maximum((a & 0xFF) - (b & 0xFF), 0)


def nms_scale(mn, factor):
    prod = ((mn & 0xFF) * (factor & 0xFFFF)) & 0xFFFF
    s = (prod >> 5).astype(np.uint16).view(np.int16).astype(np.int64)
    return np.clip(s, -128, 127)


def check_constant(algo, param, msg_max, mn):
    """cst of check_constants from the minimum `mn` it is computed from"""
    if algo == "NMS":
        return nms_scale(mn, param)
    return np.minimum(as_i8(subs_u8(mn, param)), msg_max)


# ---- pairs --------------------------------------------------------------------------

def probe():
    global _probe
    if _probe is None:
        _probe = C.CDLL(os.path.join(ROOT, "ldpcgputegra_amd", "libldsepi_probe.so"))
    return _probe


def pairs(lo, hi):
    lo, hi = np.asarray(lo, dtype=np.int64), np.asarray(hi, dtype=np.int64)
    return np.ascontiguousarray(((lo & 0xFFFF) | ((hi & 0xFFFF) << 16)).astype(np.uint32))


def pair1(lo, hi):
    return int(pairs([lo], [hi])[0])


def halves(p):
    p = np.asarray(p, dtype=np.uint32)
    return ((p & 0xFFFF).astype(np.uint16).view(np.int16).astype(np.int64),
            (p >> 16).astype(np.uint16).view(np.int16).astype(np.int64))


def other(a):
    """the high half's values: the low half's, in another order"""
    return np.roll(np.asarray(a)[::-1], 7)


def call(name, arrays, consts):
    n = arrays[0].size
    out = np.empty(n, dtype=np.uint32)
    fn = getattr(probe(), name)
    fn.restype = None
    fn(*[C.c_void_p(a.ctypes.data) for a in arrays], *consts, C.c_void_p(out.ctypes.data), C.c_long(n))
    return halves(out)


def u32(x):
    return C.c_uint32(x)


# ---- the arithmetic probe -----------------------------------------------------------

def test_probe_contribution():
    v, m = [a.ravel() for a in np.meshgrid(np.arange(-128, 128), np.arange(-127, 128), indexing="ij")]
    v1, m1 = other(v), other(m)
    for vmin in VAR_MINS:
        vmin1 = VAR_MINS[(VAR_MINS.index(vmin) + 1) % len(VAR_MINS)]
        lo, hi = call("pki8_contribution", [pairs(v, v1), pairs(m, m1)], [u32(pair1(127, 127)), u32(pair1(vmin, vmin1))])
        assert np.array_equal(lo, np.maximum(sat8(v - m), vmin)), vmin
        assert np.array_equal(hi, np.maximum(sat8(v1 - m1), vmin1)), vmin1
    # a padding lane's bounds: the constant -127 whatever it loads
    lo, hi = call("pki8_contribution", [pairs(v, v1), pairs(m, m1)], [u32(pair1(-127, -127)), u32(pair1(-127, -127))])
    assert (lo == -127).all() and (hi == -127).all()


def test_probe_magnitude():
    c = np.arange(-127, 128)
    c1 = other(c)
    for mm in MSG_MAXS:
        mm1 = MSG_MAXS[(MSG_MAXS.index(mm) + 2) % len(MSG_MAXS)]
        lo, hi = call("pki8_magnitude", [pairs(c, c1)], [C.c_int(0), u32(pair1(mm, mm1))])
        assert np.array_equal(lo, np.minimum(abs8(c), mm)) and np.array_equal(hi, np.minimum(abs8(c1), mm1)), mm
        lo, hi = call("pki8_magnitude", [pairs(c, c1)], [C.c_int(1), u32(pair1(mm, mm1))])
        assert np.array_equal(lo, abs8(np.minimum(c, mm))) and np.array_equal(hi, abs8(np.minimum(c1, mm1))), mm
        # a padding lane (contribution -127, y = 127): magnitude 127 under both rules
        pad = pairs(np.full(4, -127), np.full(4, -127))
        for x in (pair1(127, 127), pair1(mm, mm1)):      # first rule, later rule
            lo, hi = call("pki8_magnitude_xy", [pad], [u32(x), u32(pair1(127, 127))])
            assert (lo == 127).all() and (hi == 127).all(), mm


def test_probe_constants():
    e = np.arange(0, 128)
    e1 = other(e)
    for off in OFFSETS:
        off1 = OFFSETS[(OFFSETS.index(off) + 1) % len(OFFSETS)]
        for mm in MSG_MAXS:
            mm1 = MSG_MAXS[(MSG_MAXS.index(mm) + 2) % len(MSG_MAXS)]
            lo, hi = call("pki8_cst_oms", [pairs(e, e1)], [u32(pair1(off, off1)), u32(pair1(mm, mm1))])
            assert np.array_equal(lo, check_constant("OMS", off, mm, e)), (off, mm)
            assert np.array_equal(hi, check_constant("OMS", off1, mm1, e1)), (off1, mm1)
    for f in FACTORS:
        f1 = FACTORS[(FACTORS.index(f) + 3) % len(FACTORS)]
        lo, hi = call("pki8_cst_nms", [pairs(e, e1)], [u32(pair1(f, f1))])
        assert np.array_equal(lo, check_constant("NMS", f, 0, e)), f
        assert np.array_equal(hi, check_constant("NMS", f1, 0, e1)), f1
        assert lo.max() <= 127 and lo.min() >= 0


def test_probe_message_and_new_v():
    # message: (parity ^ (c < 0)) ? -r : r, a contribution of 0 counting as positive
    c, r, par = [a.ravel() for a in np.meshgrid(np.arange(-127, 128), np.arange(0, 128), np.arange(2), indexing="ij")]
    c1, r1, par1 = other(c), other(r), other(par)
    sx = pairs(c, c1) ^ pairs(par << 15, par1 << 15)
    lo, hi = call("pki8_message", [pairs(r, r1), sx], [])
    assert np.array_equal(lo, np.where(par ^ (c < 0), as_i8(-r), r))
    assert np.array_equal(hi, np.where(par1 ^ (c1 < 0), as_i8(-r1), r1))
    # new V: max(sat8(c + m'), var_min), every (c, m')
    c, m = [a.ravel() for a in np.meshgrid(np.arange(-127, 128), np.arange(-127, 128), indexing="ij")]
    c1, m1 = other(c), other(m)
    for vmin in VAR_MINS:
        vmin1 = VAR_MINS[(VAR_MINS.index(vmin) + 1) % len(VAR_MINS)]
        lo, hi = call("pki8_new_v", [pairs(c, c1), pairs(m, m1)], [u32(pair1(vmin, vmin1))])
        assert np.array_equal(lo, np.maximum(sat8(c + m), vmin)) and np.array_equal(hi, np.maximum(sat8(c1 + m1), vmin1))
    # hard decisions V > 0 per half, the raw LLR -128 included
    v = np.arange(-128, 128)
    v1 = other(v)
    lo, hi = call("pki8_pos2", [pairs(v, v1)], [])
    assert np.array_equal(lo, (v > 0) | ((v1 > 0) << 1)) and not hi.any()


# ---- host decoder and oracle on the new domain -----------------------------------------

@pytest.mark.parametrize("d,rows,Z", ED.ALL, ids=[ED.synthetic_name(*k) for k in ED.ALL])
def test_host_equals_oracle(d, rows, Z):
    t = ED.synthetic(d, rows, Z)
    name = ED.synthetic_name(d, rows, Z)
    dec = Decoder(Code(t), device=-1, max_batch=BATCH)
    for kind in PD.INPUTS:
        x = PD.make_input(kind, BATCH, t.n)
        for p in DOMAIN:
            exp = PD.oracle_decode(name, (kind, BATCH), x, p, ITERS, table=t)
            got = dec.decode_i8(x, ITERS, p.product())
            assert np.array_equal(got, exp[0]), (name, kind, p.id)
    dec.close()


# ---- the early-termination input ----------------------------------------------------------

@pytest.mark.parametrize("algo", sorted(ET_PARAMS))
def test_early_termination_input(algo):
    p = ET_PARAMS[algo]
    its = PD.oracle_decode(ET_CODE, "i8ep_et", et_input(), p, ET_ITERS, early=True)[2]
    assert its.tolist() == ET_ITERS_USED[algo]
    pr = [(int(its[2 * k]), int(its[2 * k + 1])) for k in range(ET_BATCH // 2)]
    assert any(a < ET_ITERS and b == ET_ITERS for a, b in pr), "a pair (stops, runs to the limit)"
    assert any(a == ET_ITERS and b < ET_ITERS for a, b in pr), "a pair (runs to the limit, stops)"
    assert any(a < ET_ITERS and b < ET_ITERS and a != b for a, b in pr), "a pair whose halves stop apart"
    assert its[ET_BATCH - 1] < ET_ITERS, "the lone last half stops"


# ---- the switch -------------------------------------------------------------------------

def test_switch_on_a_host_context():
    dec = Decoder(Code("648x324"), device=-1, max_batch=4)
    assert dec.i8_edge_parallel is False
    for flag in (True, False):
        with pytest.raises(LdpcError) as e:
            dec.set_i8_edge_parallel(flag)
        assert e.value.status == _lib.LDPC_EUNSUPPORTED
        assert dec.i8_edge_parallel is False
    dec.close()
    with pytest.raises(LdpcError) as e:
        Decoder(Code("648x324"), device=-1, max_batch=4, i8_edge_parallel=True)
    assert e.value.status == _lib.LDPC_EUNSUPPORTED
    L = _lib.lib()
    on = C.c_int(5)
    assert L.ldpc_ctx_set_i8_edge_parallel(None, 1) == _lib.LDPC_EINVAL
    assert L.ldpc_ctx_get_i8_edge_parallel(None, C.byref(on)) == _lib.LDPC_EINVAL and on.value == 5


def test_exports():
    L = _lib.lib()
    for name in ("ldpc_ctx_set_i8_edge_parallel", "ldpc_ctx_get_i8_edge_parallel", "ldpc_ldsepi_params_ok"):
        assert name in _lib.SIGNATURES and hasattr(L, name), name
    with open(os.path.join(ROOT, "include", "ldpc_mi355x.h")) as f:
        header = f.read()
    assert "int ldpc_ctx_set_i8_edge_parallel(ldpc_ctx *ctx, int enable);" in header
    assert "int ldpc_ctx_get_i8_edge_parallel(ldpc_ctx *ctx, int *enable);" in header
    with open(os.path.join(ROOT, "include", "ldpc_mi355x.hpp")) as f:
        assert "setI8EdgeParallel" in f.read()


def params_ok_restated(p):
    if p.algo not in (ALGO_OMS, ALGO_NMS, ALGO_MS):
        return False
    if p.var_max != 127 or not -127 <= p.var_min <= 0 or not 0 <= p.msg_max <= 127:
        return False
    return p.algo != ALGO_OMS or 0 <= p.offset <= 255


def test_params_ok():
    L = _lib.lib()
    ok = C.c_int(7)
    seen = set()
    for algo in (ALGO_OMS, ALGO_NMS, ALGO_MS, ALGO_BP):
        for var_min in (-129, -128, -127, -64, -1, 0, 1):
            for var_max in (127, 126):
                for msg_max in (-1, 0, 31, 127, 128):
                    for offset in (-1, 0, 1, 255, 256):
                        for factor in (0, 26, 65535, 70000):
                            for early in (0, 1):
                                p = default_params(algo=algo, var_min=var_min, var_max=var_max, msg_max=msg_max,
                                                   offset=offset, factor=factor, early_term=early)
                                assert L.ldpc_ldsepi_params_ok(C.byref(p), C.byref(ok)) == _lib.LDPC_OK
                                assert bool(ok.value) == params_ok_restated(p), (algo, var_min, var_max, msg_max, offset)
                                seen.add(bool(ok.value))
    assert seen == {True, False}
    for p in PD.GRID:      # var_min = -128 is the one way out of the domain among the accepted parameter sets
        assert L.ldpc_ldsepi_params_ok(C.byref(p.product()), C.byref(ok)) == _lib.LDPC_OK
        assert bool(ok.value) == (p.var_min >= -127), p.id
    assert L.ldpc_ldsepi_params_ok(None, C.byref(ok)) == _lib.LDPC_EINVAL
    assert L.ldpc_ldsepi_params_ok(C.byref(default_params()), None) == _lib.LDPC_EINVAL
