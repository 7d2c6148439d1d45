"""The binary16 decode of every code on the GPU (the f16_all_codes switch): the
packed LDS-resident kernel (family 7, `ldsh`) and the packed any-H kernel
(family 1, `generich`) against the host decoder, which defines the half contract
 and which test_f16_cpu.py / test_f16_short_cpu.py tie to its
numpy restatement.  "Equal" is always hard as uint8, soft as uint16 bit patterns
and iters_used as int32 with zero differing elements.

* every check degree 2 .. 32 on short_domain's synthetic tables, Z = 12 (two
  lanes per check, odd degrees with their padding lane) and Z = 40 (lanes
  looping and idle), on both families;
* every launch shape of ldsh (LDPC_LDSH_LANES 8 / 16 / 32 / 64) at batches 1,
  17, 65 and 130 (a lone half pair, a partly filled last wave, several waves);
  a shape the table cannot run is LDPC_EUNSUPPORTED and writes nothing;
* early termination per codeword: pairs whose halves stop apart or never;
* every shipped .ldpc table through the automatic choice;
* family 1 == family 11 == host on staircase tables;
* the buffer contract on 2-byte aligned slices, odd batches included;
* scratch shared with int8 and float32 decodes; selection and status codes."""
import ctypes as C

import numpy as np
import pytest

import f16_ref as R
import short_domain as SD
import struct_domain as ST
from ldpcgputegra_amd import ALGO_BP, ALGO_MS, ALGO_NMS, ALGO_OMS, Code, Decoder, LdpcError, _lib, default_params, \
    load_table
from test_f16_short_cpu import ET_BATCH, ET_ITERS, ET_ITERS_USED, et_input, ldsh_rule_shape

pytestmark = pytest.mark.gpu

ALGO = {"MS": (ALGO_MS, 0.0), "OMS": (ALGO_OMS, 0.375), "NMS": (ALGO_NMS, 0.8125),
        "OMS.5": (ALGO_OMS, 0.5), "NMS.75": (ALGO_NMS, 0.75)}
FAMILY = {7: "lds", 1: "generic", 11: "stairf"}
LANES = (8, 16, 32, 64)
BATCHES = (1, 17, 65, 130)
LDS_MAX = 64 * 1024
SOFT_FILL, HARD_FILL, ITS_FILL = 0x1234, 9, -7
_host_ref = {}


def _torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def _table(name):
    if isinstance(name, tuple):
        return SD.synthetic(*name)
    if name.endswith(".st"):
        return ST.table(name[:-3])
    return load_table(name)


def _params(algo, early=False):
    a, beta = ALGO[algo]
    return default_params(algo=a, beta=beta, early_term=int(early))


def host_ref(name, x, key, iters, algo, early=False):
    """(hard, soft uint16, iters_used) of the host decoder, computed once per case and read-only"""
    k = (name, key, iters, algo, early)
    if k not in _host_ref:
        dec = Decoder(Code(_table(name)), device=-1, max_batch=max(x.shape[0], 1))
        hard, soft, its = dec.decode_f16_soft(x, iters, _params(algo, early))
        dec.close()
        out = (hard, np.asarray(soft).view(np.uint16), its)
        for a in out:
            a.setflags(write=False)
        _host_ref[k] = out
    return _host_ref[k]


def as_device(x):
    torch = _torch()
    return torch.from_numpy(np.array(x).view(np.int16)).cuda().view(torch.float16)


def run_f16(dec, d_llr, iters, params, extra=2):
    """decode_f16_device with guard rows behind every output"""
    torch = _torch()
    B, n = d_llr.shape
    d_hard = torch.full((B + extra, n), HARD_FILL, dtype=torch.uint8, device="cuda")
    d_soft = torch.full((B + extra, n), SOFT_FILL, dtype=torch.int16, device="cuda")
    d_its = torch.full((B + extra,), ITS_FILL, dtype=torch.int32, device="cuda")
    dec.decode_f16_device(d_llr, d_hard, iters, params=params, soft=d_soft.view(torch.float16), iters_used=d_its)
    torch.cuda.synchronize()
    hard, soft, its = d_hard.cpu().numpy(), d_soft.cpu().numpy().view(np.uint16), d_its.cpu().numpy()
    assert (hard[B:] == HARD_FILL).all() and (soft[B:] == SOFT_FILL).all() and (its[B:] == ITS_FILL).all(), \
        "rows beyond the batch written"
    return hard[:B], soft[:B], its[:B]


def assert_bits(got, exp, where):
    for g, e, what in zip(got, exp, ("hard", "soft", "iters_used")):
        assert g.dtype == e.dtype and g.shape == e.shape, (where, what, g.dtype, e.dtype)
        bad = np.flatnonzero((g != e).ravel())
        assert bad.size == 0, "%s: %s differs in %d of %d places, first at %d: %r vs %r" % (
            where, what, bad.size, g.size, bad[0], g.ravel()[bad[0]], e.ravel()[bad[0]])


def _status(fn):
    with pytest.raises(LdpcError) as e:
        fn()
    return e.value.status, str(e.value)


def layer_info(code):
    """(layers, widest layer, float state fits LDS) of ldpc_code_layer_info"""
    nl, mw, i8, f32 = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    _lib.check(_lib.lib().ldpc_code_layer_info(code.handle, C.byref(nl), C.byref(mw), C.byref(i8), C.byref(f32)))
    return nl.value, mw.value, bool(f32.value)


def need_lanes(mw):
    return 8 if mw <= 8 else 16 if mw <= 16 else 32 if mw <= 32 else 64


def lds_bytes(t, lanes):
    """ldsh's LDS per wave: the u16 edge table in whole 16-B chunks, then 64 / lanes pairs of V[N] + msg[E] uint32"""
    e = len(t.edge_var)
    return (2 * e + 15) // 16 * 16 + (64 // lanes) * (t.n + e) * 4


def shape_legal(t, code, lanes):
    _, mw, fits = layer_info(code)
    return fits and lanes >= need_lanes(mw) and lds_bytes(t, lanes) <= LDS_MAX


def rule_shape(t, mw, batch):
    """the shape ldsh's rule takes, from its restatement (test_f16_short_cpu.ldsh_rule_shape)"""
    return ldsh_rule_shape(t.n, len(t.edge_var), mw, batch)


# ---- degrees x shapes -----------------------------------------------------------

@pytest.mark.parametrize("d", SD.DEGREES)
def test_every_degree(d):
    algos = ("OMS", "MS", "NMS") if d in (2, 3, 17, 32) else ("OMS",)
    for Z in (SD.Z_SPLIT, SD.Z_LOOP):
        t = SD.synthetic(d, Z)
        x = R.make_input(5, t.n)
        dev = as_device(x)
        dec = Decoder(Code(t), max_batch=64, f16_all_codes=True)
        for fam in (7, 1):
            dec.set_kernel(fam)
            for algo in algos:
                got = run_f16(dec, dev, 2, _params(algo))
                assert dec.last_kernel == FAMILY[fam]
                if fam == 7:    # Z = 12: 32 lanes, two per check (24 busy); Z = 40: 64 lanes, one per check
                    exp_shape = (32, True) if Z == SD.Z_SPLIT else (64, False)
                    assert dec.last_lds_shape == rule_shape(t, Z, 5) == exp_shape
                assert_bits(got, host_ref((d, Z), x, 5, 2, algo), "d %d Z %d family %d %s" % (d, Z, fam, algo))
        dec.close()


# ---- every launch shape of ldsh ---------------------------------------------------

@pytest.mark.parametrize("lanes", LANES)
@pytest.mark.parametrize("name", ("200x100", "648x324", "1024x518", (7, 12)), ids=str)
def test_launch_shapes(name, lanes, monkeypatch):
    torch = _torch()
    t = _table(name)
    code = Code(t)
    mw = layer_info(code)[1]
    dec = Decoder(code, max_batch=max(BATCHES), f16_all_codes=True)
    monkeypatch.setenv("LDPC_LDSH_LANES", str(lanes))
    dec.set_kernel(7)      # (the family has the table's plan even where the float state passes LDS at every shape)
    legal = shape_legal(t, code, lanes)
    for batch in BATCHES:
        x = R.make_input(batch, t.n)
        dev = as_device(x)
        if legal:
            got = run_f16(dec, dev, 2, _params("OMS"))
            assert dec.last_kernel == "lds" and dec.last_lds_shape == (lanes, lanes >= 2 * mw)
            assert_bits(got, host_ref(name, x, batch, 2, "OMS"), "%s lanes %d batch %d" % (name, lanes, batch))
        else:
            hard = torch.full((batch, t.n), HARD_FILL, dtype=torch.uint8, device="cuda")
            st, _ = _status(lambda: dec.decode_f16_device(dev, hard, 2, params=_params("OMS")))
            torch.cuda.synchronize()
            assert st == _lib.LDPC_EUNSUPPORTED
            assert (hard.cpu().numpy() == HARD_FILL).all(), "a refused shape launched something"
    if legal:              # and the rule's own shape, from the restatement
        monkeypatch.delenv("LDPC_LDSH_LANES")
        x = R.make_input(17, t.n)
        got = run_f16(dec, as_device(x), 2, _params("OMS"))
        assert dec.last_lds_shape == rule_shape(t, mw, 17)
        assert_bits(got, host_ref(name, x, 17, 2, "OMS"), "%s automatic shape" % (name,))
    dec.close()


# ---- early termination ------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(ET_ITERS_USED))
def test_early_termination(name, monkeypatch):
    """The inputs test_f16_short_cpu.py describes: halves of a pair that stop at
    different iterations, one half that never stops, a lone last codeword."""
    t = _table(name)
    code = Code(t)
    x = et_input(name)
    dev = as_device(x)
    exp = host_ref(name, x, "et", ET_ITERS, "MS", early=True)
    assert exp[2].tolist() == ET_ITERS_USED[name]
    dec = Decoder(code, max_batch=ET_BATCH, f16_all_codes=True)
    dec.set_kernel(7)
    shapes = [lanes for lanes in LANES if shape_legal(t, code, lanes)]
    assert len(shapes) >= 2, name
    for lanes in shapes:
        monkeypatch.setenv("LDPC_LDSH_LANES", str(lanes))
        got = run_f16(dec, dev, ET_ITERS, _params("MS", early=True))
        assert dec.last_lds_shape[0] == lanes
        assert_bits(got, exp, "%s early termination, family 7, %d lanes" % (name, lanes))
    monkeypatch.delenv("LDPC_LDSH_LANES")
    for fam in (7, 1):
        dec.set_kernel(fam)
        for algo in ("MS",) if fam == 7 else ("MS", "OMS.5", "NMS.75"):
            got = run_f16(dec, dev, ET_ITERS, _params(algo, early=True))
            assert dec.last_kernel == FAMILY[fam]
            assert_bits(got, host_ref(name, x, "et", ET_ITERS, algo, early=True),
                        "%s early termination, family %d, %s" % (name, fam, algo))
    dec.set_kernel(7)
    for algo in ("OMS.5", "NMS.75"):
        got = run_f16(dec, dev, ET_ITERS, _params(algo, early=True))
        assert_bits(got, host_ref(name, x, "et", ET_ITERS, algo, early=True),
                    "%s early termination, family 7, %s" % (name, algo))
    dec.close()


# ---- every shipped table, the automatic choice ------------------------------------

@pytest.mark.parametrize("name", SD.SHORT_CODES)
def test_shipped_tables_automatic(name):
    t = _table(name)
    code = Code(name)
    nl, _, fits = layer_info(code)
    batch = 2 if name in ("20000x10000", "16200x7560") else 3
    x = R.make_input(batch, t.n)
    dec = Decoder(code, max_batch=64, f16_all_codes=True)
    got = run_f16(dec, as_device(x), 2, _params("OMS"))
    assert dec.last_kernel == ("lds" if fits and t.m >= 8 * nl else "generic")
    assert dec.last_skipped is None
    assert_bits(got, host_ref(name, x, batch, 2, "OMS"), name)
    dec.close()


def test_automatic_takes_both_families():
    picks = set()
    for name in SD.SHORT_CODES:
        code = Code(name)
        nl, _, fits = layer_info(code)
        picks.add(fits and _table(name).m >= 8 * nl)
    assert picks == {True, False}


# ---- staircase tables: family 1 == family 11 == host ------------------------------

@pytest.mark.parametrize("name", ("dvbs2_r1_2", "x8_q5_h110.st"))
def test_staircase_cross_check(name):
    t = _table(name)
    x = R.make_input(5, t.n)
    dev = as_device(x)
    exp = host_ref(name, x, 5, 2, "OMS")
    dec = Decoder(Code(t), max_batch=64, f16_all_codes=True)
    got = {}
    for fam in (0, 1, 11):
        dec.set_kernel(fam)
        got[fam] = run_f16(dec, dev, 2, _params("OMS"))
        assert dec.last_kernel == FAMILY[fam or 11]          # the automatic choice stays the staircase kernel
        assert_bits(got[fam], exp, "%s family %d" % (name, fam))
    assert_bits(got[1], got[11], name + " family 1 against family 11")
    dec.close()


# ---- the buffer contract ----------------------------------------------------------

@pytest.mark.parametrize("batch", (0, 1, 3, 64, 65))
@pytest.mark.parametrize("name,fam", (("648x324", 7), ("2048x384", 1)))
def test_buffer_contract(name, fam, batch):
    """Inputs and outputs are slices starting 2 bytes (binary16), 1 byte (hard)
    and 4 bytes (iters_used) into larger buffers; everything outside the
    [batch] rows keeps its fill.  An odd batch leaves the last pair half empty."""
    torch = _torch()
    t = _table(name)
    n, rows = t.n, 66
    x = R.make_input(max(batch, 1), n)[:batch]
    dec = Decoder(Code(t), max_batch=rows, kernel=fam, f16_all_codes=True)
    buf_in = torch.full((rows * n + 1,), SOFT_FILL, dtype=torch.int16, device="cuda")
    buf_soft = torch.full((rows * n + 3,), SOFT_FILL, dtype=torch.int16, device="cuda")
    buf_hard = torch.full((rows * n + 3,), HARD_FILL, dtype=torch.uint8, device="cuda")
    buf_its = torch.full((rows + 2,), ITS_FILL, dtype=torch.int32, device="cuda")
    d_in = buf_in[1:1 + batch * n].view(torch.float16).view(batch, n)
    if batch:
        d_in.copy_(as_device(x))
    d_soft = buf_soft[1:1 + batch * n].view(torch.float16).view(batch, n)
    d_hard = buf_hard[1:1 + batch * n].view(batch, n)
    d_its = buf_its[1:1 + batch]
    dec.decode_f16_device(d_in, d_hard, 2, params=_params("NMS"), soft=d_soft, iters_used=d_its)
    torch.cuda.synchronize()
    soft, hard, its = buf_soft.cpu().numpy().view(np.uint16), buf_hard.cpu().numpy(), buf_its.cpu().numpy()
    assert soft[0] == SOFT_FILL and (soft[1 + batch * n:] == SOFT_FILL).all()
    assert hard[0] == HARD_FILL and (hard[1 + batch * n:] == HARD_FILL).all()
    assert its[0] == ITS_FILL and (its[1 + batch:] == ITS_FILL).all()
    assert (buf_in.cpu().numpy().view(np.uint16)[1 + batch * n:] == SOFT_FILL).all()
    if batch:
        assert dec.last_kernel == FAMILY[fam]
        exp = host_ref(name, x, ("contract", batch), 2, "NMS")
        got = (hard[1:1 + batch * n].reshape(batch, n), soft[1:1 + batch * n].reshape(batch, n), its[1:1 + batch])
        assert_bits(got, exp, "%s batch %d on unaligned slices" % (name, batch))
        # hard decisions alone: no soft output, no iteration counts
        only = torch.full((batch + 1, n), HARD_FILL, dtype=torch.uint8, device="cuda")
        dec.decode_f16_device(d_in, only[:batch], 2, params=_params("NMS", early=True))
        torch.cuda.synchronize()
        only = only.cpu().numpy()
        assert (only[batch] == HARD_FILL).all()
        assert np.array_equal(only[:batch], host_ref(name, x, ("contract", batch), 2, "NMS", early=True)[0])
    dec.close()


def test_aligned_rows_take_the_wide_loads():
    """648 * 2 bytes is a multiple of 16: a 16-byte aligned buffer goes through
    ldsh's 16-B loads, one offset by 2 bytes through the 2-byte ones; 200x100's
    rows (400 bytes) always do.  The same results either way."""
    torch = _torch()
    t = _table("648x324")
    x = R.make_input(7, t.n)
    exp = host_ref("648x324", x, 7, 2, "OMS")
    dec = Decoder(Code(t), max_batch=64, kernel=7, f16_all_codes=True)
    dev = as_device(x)
    assert dev.data_ptr() % 16 == 0 and (t.n * 2) % 16 == 0
    assert_bits(run_f16(dec, dev, 2, _params("OMS")), exp, "aligned rows")
    buf = torch.zeros((7 * t.n + 1,), dtype=torch.float16, device="cuda")
    off = buf[1:].view(7, t.n)
    off.copy_(dev)
    assert off.data_ptr() % 16 == 2
    assert_bits(run_f16(dec, off, 2, _params("OMS")), exp, "rows offset by 2 bytes")
    dec.close()


# ---- scratch shared with the other element types ----------------------------------

def test_scratch_shared_with_int8_and_float32():
    torch = _torch()
    name = "2048x384"
    t = _table(name)
    x = R.make_input(65, t.n)
    dev = as_device(x)
    exp = host_ref(name, x, 65, 2, "OMS")
    exp_et = host_ref(name, x, 65, 2, "OMS", early=True)
    dec = Decoder(Code(t), max_batch=130, kernel=1, f16_all_codes=True)
    assert_bits(run_f16(dec, dev, 2, _params("OMS")), exp, "fresh context")
    q = torch.from_numpy(np.array(ST.f32_input(130, t.n)).astype(np.int8)).cuda()
    y = torch.from_numpy(np.array(ST.f32_input(130, t.n))).cuda()
    hard = torch.zeros((130, t.n), dtype=torch.uint8, device="cuda")
    dec.decode_i8_device(q, hard, 3)
    dec.decode_f32_device(y, hard, 3, params=default_params(algo=ALGO_MS, early_term=1))
    torch.cuda.synchronize()
    assert dec.last_kernel == "generic"
    ref32 = hard.cpu().numpy().copy()
    assert_bits(run_f16(dec, dev, 2, _params("OMS")), exp, "after an int8 and a float32 decode")
    assert_bits(run_f16(dec, dev, 2, _params("OMS", early=True)), exp_et, "early termination after them")
    dec.decode_f32_device(y, hard, 3, params=default_params(algo=ALGO_MS, early_term=1))
    torch.cuda.synchronize()
    assert np.array_equal(hard.cpu().numpy(), ref32)      # and float32 after f16 is unchanged too
    dec.close()


# ---- selection and status ---------------------------------------------------------

def test_switch_off_is_the_default():
    """The regression guard for the default: a code without a staircase is refused."""
    torch = _torch()
    n = _table("648x324").n
    dev = as_device(R.make_input(2, n))
    hard = torch.full((2, n), HARD_FILL, dtype=torch.uint8, device="cuda")
    dec = Decoder(Code("648x324"), max_batch=64)
    assert dec.f16_all_codes is False
    for k in (0, 7, 1):
        dec.set_kernel(k)
        st, msg = _status(lambda: dec.decode_f16_device(dev, hard, 1))
        assert st == _lib.LDPC_EUNSUPPORTED and "staircase" in msg, (k, msg)
    dec.set_kernel(0)
    dec.set_f16_all_codes(True)
    dec.decode_f16_device(dev, hard, 1)
    assert dec.last_kernel == "lds"
    dec.set_f16_all_codes(False)
    assert _status(lambda: dec.decode_f16_device(dev, hard, 1))[0] == _lib.LDPC_EUNSUPPORTED
    dec.close()
    # on a staircase table the switch off still refuses every family but 11
    t = ST.table("x5_q1_h57")
    d5 = as_device(R.make_input(2, t.n))
    h5 = torch.zeros((2, t.n), dtype=torch.uint8, device="cuda")
    dec = Decoder(Code(t), max_batch=64, kernel=1)
    st, msg = _status(lambda: dec.decode_f16_device(d5, h5, 1))
    assert st == _lib.LDPC_EUNSUPPORTED and "not applicable" in msg
    dec.close()


def test_selection_table():
    torch = _torch()
    # a code that prefers family 7, one that fits it without preferring it, one that does not fit
    for name, auto in (("648x324", "lds"), ("200x100", "generic"), ("2048x384", "generic")):
        t = _table(name)
        code = Code(t)
        nl, _, fits = layer_info(code)
        assert auto == ("lds" if fits and t.m >= 8 * nl else "generic"), name
        x = R.make_input(4, t.n)
        dev = as_device(x)
        exp = host_ref(name, x, 4, 1, "MS")
        hard = torch.zeros((4, t.n), dtype=torch.uint8, device="cuda")
        dec = Decoder(code, max_batch=64, f16_all_codes=True)
        assert_bits(run_f16(dec, dev, 1, _params("MS")), exp, name + " automatic")
        assert dec.last_kernel == auto and dec.last_skipped is None
        dec.set_kernel(1)
        assert_bits(run_f16(dec, dev, 1, _params("MS")), exp, name + " forced 1")
        assert dec.last_kernel == "generic" and dec.last_lds_shape == (0, False)
        try:
            dec.set_kernel(7)
            forced7 = True
        except LdpcError:
            forced7 = False       # the family refuses this table altogether
        if forced7 and fits:
            assert_bits(run_f16(dec, dev, 1, _params("MS")), exp, name + " forced 7")
            assert dec.last_kernel == "lds" and dec.last_lds_shape == rule_shape(t, layer_info(code)[1], 4)
        elif forced7:
            st, msg = _status(lambda: dec.decode_f16_device(dev, hard, 1))
            assert st == _lib.LDPC_EUNSUPPORTED and "not applicable" in msg
        for k in (2, 3, 5, 8, 9, 11):
            try:
                dec.set_kernel(k)
            except LdpcError:
                continue
            st, msg = _status(lambda: dec.decode_f16_device(dev, hard, 1))
            assert st == _lib.LDPC_EUNSUPPORTED and "not applicable" in msg, (name, k, msg)
        # parameter checking is unchanged: BP, beta
        dec.set_kernel(0)
        assert _status(lambda: dec.decode_f16_device(dev, hard, 1, params=default_params(algo=ALGO_BP)))[0] == \
            _lib.LDPC_EUNSUPPORTED
        for beta in (-0.5, float("inf"), float("nan"), 65520.0):
            for algo in (ALGO_OMS, ALGO_NMS):
                st, _ = _status(lambda: dec.decode_f16_device(dev, hard, 1, params=default_params(algo=algo, beta=beta)))
                assert st == _lib.LDPC_EINVAL, beta
        # batch 0 touches nothing and takes NULL pointers
        p = default_params(algo=ALGO_MS)
        assert _lib.lib().ldpc_decode_f16_async(dec._ctx, None, None, None, None, None, 0, 1, C.byref(p)) == _lib.LDPC_OK
        dec.close()
    # a staircase code with the switch on: 11 by default and forced, 7 not applicable
    t = ST.table("x5_q1_h57")
    dev = as_device(R.make_input(4, t.n))
    hard = torch.zeros((4, t.n), dtype=torch.uint8, device="cuda")
    dec = Decoder(Code(t), max_batch=64, f16_all_codes=True)
    dec.decode_f16_device(dev, hard, 1)
    assert dec.last_kernel == "stairf"
    for k in (2, 3, 5, 7, 8):
        try:
            dec.set_kernel(k)
        except LdpcError:
            continue
        if k == 7 and layer_info(Code(t))[2]:
            continue              # (a staircase table small enough for LDS runs there when forced)
        st, msg = _status(lambda: dec.decode_f16_device(dev, hard, 1))
        assert st == _lib.LDPC_EUNSUPPORTED and "not applicable" in msg, (k, msg)
    dec.close()


@pytest.mark.parametrize("name", ("648x324", "2048x384"))
def test_host_buffer_entry_point(name):
    """ldpc_decode_f16 with host buffers on a GPU context: copy in, decode, copy out."""
    t = _table(name)
    x = R.make_input(5, t.n)
    dec = Decoder(Code(t), max_batch=64, f16_all_codes=True)
    got = run_f16(dec, as_device(x), 2, _params("OMS"))
    assert np.array_equal(dec.decode_f16(x, 2, _params("OMS")), got[0])
    assert np.array_equal(got[0], host_ref(name, x, 5, 2, "OMS")[0])
    dec.close()
