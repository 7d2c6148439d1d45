"""The edge-parallel binary16 kernel on the GPU (`ldseph`: family 9 of the f16
decode, behind the f16_edge_parallel switch) against the host decoder, which
defines the half contract and which test_f16_cpu.py /
test_f16_ep_cpu.py tie to its numpy restatement.  "Equal" is always hard as
uint8, soft as uint16 bit patterns and iters_used as int32 with zero differing
elements.

* every table of ldsep_domain (check degrees 2 .. 8: padding lanes; Z = 8, 27,
  32 in the 12 x 4 shape and Z = 41 in the 11 x 6 shape: full, ragged and empty
  passes) x MS / OMS / NMS at batches 1, 2, 7, 9 and 17: a lone half, one full
  pair, a ragged workgroup with an odd tail, a second workgroup holding only a
  lone half, several workgroups; guard rows behind every output;
* the shipped 648x324 and 576x288 tables, 20 iterations;
* early termination per codeword: pairs (stops, never), (never, stops), halves
  that stop apart, a lone last half;
* -0.0 and +0.0 LLRs on every variable of some checks: equal including the sign
  of zero soft values, which the float32 kernel of the family cannot offer;
* the buffer contract on 2-byte aligned slices of odd batches;
* selection with the switch off (the parent's answers) and on."""
import ctypes as C

import numpy as np
import pytest

import f16_ref as R
import ldsep_domain as ED
import param_domain as PD
import struct_domain as ST
from bp_ref import check_rows
from ldpcgputegra_amd import ALGO_BP, ALGO_MS, ALGO_NMS, ALGO_OMS, Code, Decoder, LdpcError, _lib, default_params, \
    load_table
from test_f16_ep_cpu import ET_BATCH, ET_CODE, ET_ITERS, ET_ITERS_USED, et_input

pytestmark = pytest.mark.gpu

ALGO = {"MS": (ALGO_MS, 0.0), "OMS": (ALGO_OMS, 0.375), "NMS": (ALGO_NMS, 0.8125)}
BATCHES = (1, 2, 7, 9, 17)
SOFT_FILL, HARD_FILL, ITS_FILL = 0x1234, 9, -7
_host_ref = {}


def _torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def _table(name):
    return ED.synthetic(*name) if isinstance(name, tuple) else load_table(name)


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


def rows_of(ref, batch):
    """the first `batch` codewords of a reference (codewords decode independently)"""
    return tuple(a[:batch] for a in ref)


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


def assert_ldseph(dec):
    assert dec.last_kernel == "ldsep" and dec.last_skipped is None
    assert dec.last_lds_shape == (0, False) and dec.last_et_stage == 0


def _status(fn):
    with pytest.raises(LdpcError) as e:
        fn()
    return e.value.status, str(e.value)


# ---- degrees x shapes x batches ---------------------------------------------------

@pytest.mark.parametrize("d,rows,Z", ED.ALL, ids=[ED.synthetic_name(*k) for k in ED.ALL])
def test_every_table(d, rows, Z):
    torch = _torch()
    name = (d, rows, Z)
    t = ED.synthetic(*name)
    x = R.make_input(max(BATCHES), t.n)
    dec = Decoder(Code(t), max_batch=max(BATCHES), f16_edge_parallel=True)
    assert dec.f16_edge_parallel is True and dec.f16_all_codes is False
    for algo in ("MS", "OMS", "NMS"):
        exp = host_ref(name, x, max(BATCHES), 3, algo)
        for batch in BATCHES:
            got = run_f16(dec, as_device(x[:batch]), 3, _params(algo))
            assert_ldseph(dec)
            assert_bits(got, rows_of(exp, batch), "%s %s batch %d" % (ED.synthetic_name(*name), algo, batch))
    # the table really is in the family's shape: the float32 decode forced to 9 runs too
    dec.set_kernel(9)
    y = torch.from_numpy(np.array(ST.f32_input(3, t.n))).cuda()
    hard = torch.zeros((3, t.n), dtype=torch.uint8, device="cuda")
    dec.decode_f32_device(y, hard, 2, params=default_params(algo=ALGO_MS))
    torch.cuda.synchronize()
    assert dec.last_kernel == "ldsep"
    dec.close()


# ---- the shipped tables -----------------------------------------------------------

@pytest.mark.parametrize("kernel", (0, 9))
@pytest.mark.parametrize("name", ("648x324", "576x288"))
def test_shipped_tables(name, kernel):
    t = _table(name)
    x = R.make_input(17, t.n)
    dev = as_device(x)
    dec = Decoder(Code(name), max_batch=17, kernel=kernel, f16_edge_parallel=True)
    for algo in ("MS", "OMS", "NMS"):
        got = run_f16(dec, dev, 20, _params(algo))
        assert_ldseph(dec)
        assert_bits(got, host_ref(name, x, 17, 20, algo), "%s kernel %d %s" % (name, kernel, algo))
    dec.close()


# ---- early termination ------------------------------------------------------------

def test_early_termination():
    x = et_input()
    exp = host_ref(ET_CODE, x, "ep_et", ET_ITERS, "MS", early=True)
    assert exp[2].tolist() == ET_ITERS_USED
    dec = Decoder(Code(ET_CODE), max_batch=ET_BATCH, f16_edge_parallel=True)
    for batch in (ET_BATCH, ET_BATCH - 1, 1):      # a lone last half; none; a lone half alone
        got = run_f16(dec, as_device(x[:batch]), ET_ITERS, _params("MS", early=True))
        assert_ldseph(dec)
        assert_bits(got, rows_of(exp, batch), "early termination, batch %d" % batch)
    for algo in ("OMS", "NMS"):
        got = run_f16(dec, as_device(x), ET_ITERS, _params(algo, early=True))
        assert_bits(got, host_ref(ET_CODE, x, "ep_et", ET_ITERS, algo, early=True), "early termination, " + algo)
    dec.close()


# ---- zeros of both signs ----------------------------------------------------------

def test_signed_zeros():
    """Codeword 0: every LLR +0.0 or -0.0, so every check sees zeros alone;
    codeword 1: the variables of checks 27 l .. 27 l + 8, l = 0, 1, 2, are zeros
    of both signs among ordinary LLRs; codeword 2: all -0.0.  After one
    iteration the soft output holds zeros of both signs in all three (the
    parities move them: (-0) + (-0) is the only sum that stays -0), after two
    the zeros are all +0.0: both are compared, sign bits included."""
    name = "648x324"
    t = _table(name)
    x = np.array(R.make_input(3, t.n))
    z = ((PD.splitmix64(np.uint64(77 << 32) + np.arange(t.n, dtype=np.uint64)) >> np.uint64(63)) << np.uint64(15))
    z = z.astype(np.uint16)
    x[0] = z
    ev = np.asarray(t.edge_var, dtype=np.int64)
    rows = check_rows(t)
    for layer in range(3):
        for e0, d in rows[27 * layer:27 * layer + 9]:
            x[1, ev[e0:e0 + d]] = z[ev[e0:e0 + d]]
    x[2] = 0x8000
    one = host_ref(name, x, "zeros", 1, "MS")[1]
    assert set(np.unique(one[0]).tolist()) == {0x0000, 0x8000}, "codeword 0 must stay zeros, of both signs"
    assert (one[1] == 0x8000).any() and (one[1] == 0x0000).any() and (one[2] == 0x8000).any()
    two = host_ref(name, x, "zeros", 2, "MS")[1]
    assert not two[0].any() and (two[1] == 0x0000).any()
    dec = Decoder(Code(name), max_batch=4, f16_edge_parallel=True)
    for iters in (1, 2):
        for algo in ("MS", "OMS", "NMS"):
            got = run_f16(dec, as_device(x), iters, _params(algo))
            assert_ldseph(dec)
            assert_bits(got, host_ref(name, x, "zeros", iters, algo), "signed zeros, %s, %d iterations" % (algo, iters))
    dec.close()


# ---- the buffer contract ----------------------------------------------------------

@pytest.mark.parametrize("batch", (1, 3, 9))
def test_buffer_contract(batch):
    """Inputs and outputs are slices starting 2 bytes (binary16), 1 byte (hard)
    and 4 bytes (iters_used) into larger buffers; everything outside the
    [batch] rows keeps its fill.  An odd batch leaves the last pair half empty."""
    torch = _torch()
    name = "576x288"
    t = _table(name)
    n, rows = t.n, 12
    x = R.make_input(batch, n)
    dec = Decoder(Code(t), max_batch=rows, kernel=9, f16_edge_parallel=True)
    buf_in = torch.full((rows * n + 1,), SOFT_FILL, dtype=torch.int16, device="cuda")
    buf_soft = torch.full((rows * n + 3,), SOFT_FILL, dtype=torch.int16, device="cuda")
    buf_hard = torch.full((rows * n + 3,), HARD_FILL, dtype=torch.uint8, device="cuda")
    buf_its = torch.full((rows + 2,), ITS_FILL, dtype=torch.int32, device="cuda")
    d_in = buf_in[1:1 + batch * n].view(torch.float16).view(batch, n)
    d_in.copy_(as_device(x))
    assert d_in.data_ptr() % 4 == 2
    d_soft = buf_soft[1:1 + batch * n].view(torch.float16).view(batch, n)
    d_hard = buf_hard[1:1 + batch * n].view(batch, n)
    d_its = buf_its[1:1 + batch]
    dec.decode_f16_device(d_in, d_hard, 2, params=_params("NMS"), soft=d_soft, iters_used=d_its)
    torch.cuda.synchronize()
    assert_ldseph(dec)
    soft, hard, its = buf_soft.cpu().numpy().view(np.uint16), buf_hard.cpu().numpy(), buf_its.cpu().numpy()
    assert soft[0] == SOFT_FILL and (soft[1 + batch * n:] == SOFT_FILL).all()
    assert hard[0] == HARD_FILL and (hard[1 + batch * n:] == HARD_FILL).all()
    assert its[0] == ITS_FILL and (its[1 + batch:] == ITS_FILL).all()
    assert (buf_in.cpu().numpy().view(np.uint16)[1 + batch * n:] == SOFT_FILL).all()
    exp = host_ref(name, x, ("contract", batch), 2, "NMS")
    got = (hard[1:1 + batch * n].reshape(batch, n), soft[1:1 + batch * n].reshape(batch, n), its[1:1 + batch])
    assert_bits(got, exp, "batch %d on unaligned slices" % batch)
    # hard decisions alone: no soft output, no iteration counts
    only = torch.full((batch + 1, n), HARD_FILL, dtype=torch.uint8, device="cuda")
    dec.decode_f16_device(d_in, only[:batch], 2, params=_params("NMS", early=True))
    torch.cuda.synchronize()
    only = only.cpu().numpy()
    assert (only[batch] == HARD_FILL).all()
    assert np.array_equal(only[:batch], host_ref(name, x, ("contract", batch), 2, "NMS", early=True)[0])
    dec.close()


# ---- selection and status ---------------------------------------------------------

def test_switch_off_is_the_parents_selection():
    torch = _torch()
    n = _table("648x324").n
    dev = as_device(R.make_input(2, n))
    hard = torch.full((2, n), HARD_FILL, dtype=torch.uint8, device="cuda")
    dec = Decoder(Code("648x324"), max_batch=64)
    assert dec.f16_edge_parallel is False
    for k in (0, 9):
        dec.set_kernel(k)
        st, msg = _status(lambda: dec.decode_f16_device(dev, hard, 1))
        assert st == _lib.LDPC_EUNSUPPORTED and "staircase" in msg, (k, msg)
    dec.set_f16_all_codes(True)
    st, msg = _status(lambda: dec.decode_f16_device(dev, hard, 1))
    assert st == _lib.LDPC_EUNSUPPORTED and "not applicable" in msg, msg
    dec.set_kernel(0)
    dec.decode_f16_device(dev, hard, 1)
    assert dec.last_kernel == "lds"
    # on and off again: the parent's answers are back
    dec.set_f16_edge_parallel(True)
    dec.decode_f16_device(dev, hard, 1)
    assert dec.last_kernel == "ldsep"
    dec.set_f16_edge_parallel(False)
    assert dec.f16_edge_parallel is False
    dec.decode_f16_device(dev, hard, 1)
    assert dec.last_kernel == "lds"
    dec.set_kernel(9)
    assert _status(lambda: dec.decode_f16_device(dev, hard, 1))[0] == _lib.LDPC_EUNSUPPORTED
    dec.close()


@pytest.mark.parametrize("all_codes", (False, True))
def test_switch_on_selection(all_codes):
    torch = _torch()
    name = "648x324"
    t = _table(name)
    x = R.make_input(4, t.n)
    dev = as_device(x)
    exp = host_ref(name, x, 4, 1, "MS")
    hard = torch.zeros((4, t.n), dtype=torch.uint8, device="cuda")
    dec = Decoder(Code(name), max_batch=64, f16_all_codes=all_codes, f16_edge_parallel=True)
    for k in (0, 9):
        dec.set_kernel(k)
        assert_bits(run_f16(dec, dev, 1, _params("MS")), exp, "kernel %d" % k)
        assert_ldseph(dec)
    for k, family in ((7, "lds"), (1, "generic")):      # as f16_all_codes decides
        dec.set_kernel(k)
        if all_codes:
            assert_bits(run_f16(dec, dev, 1, _params("MS")), exp, "forced %d" % k)
            assert dec.last_kernel == family
        else:
            st, msg = _status(lambda: dec.decode_f16_device(dev, hard, 1))
            assert st == _lib.LDPC_EUNSUPPORTED and "staircase" in msg, (k, msg)
    for k in (2, 3, 5, 8, 11):
        try:
            dec.set_kernel(k)
        except LdpcError:
            continue
        assert _status(lambda: dec.decode_f16_device(dev, hard, 1))[0] == _lib.LDPC_EUNSUPPORTED, k
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


@pytest.mark.parametrize("name", ("200x100", "dvbs2_r1_2"))
def test_switch_refused_where_the_family_does_not_fit(name):
    dec = Decoder(Code(name), max_batch=8)
    with pytest.raises(LdpcError):
        dec.set_kernel(9)
    for flag in (True, False):
        st, _ = _status(lambda: dec.set_f16_edge_parallel(flag))
        assert st == _lib.LDPC_EUNSUPPORTED
        assert dec.f16_edge_parallel is False
    dec.close()
    st, _ = _status(lambda: Decoder(Code(name), max_batch=8, f16_edge_parallel=True))
    assert st == _lib.LDPC_EUNSUPPORTED


def test_other_element_types_after_ldseph():
    """An ldseph decode allocates and leaves nothing: an int8 and a float32
    decode on the same context still equal the host decoder's."""
    torch = _torch()
    name = "648x324"
    t = _table(name)
    x = R.make_input(9, t.n)
    y = np.array(ST.f32_input(9, t.n))
    q = y.astype(np.int8)
    host = Decoder(Code(name), device=-1, max_batch=9)
    ref8 = host.decode_i8(q, 3)
    ref32 = host.decode_f32(y, 3, default_params(algo=ALGO_MS))
    host.close()
    dec = Decoder(Code(name), max_batch=16, f16_edge_parallel=True)
    assert_bits(run_f16(dec, as_device(x), 2, _params("OMS")), host_ref(name, x, 9, 2, "OMS"), "fresh context")
    assert_ldseph(dec)
    hard = torch.zeros((9, t.n), dtype=torch.uint8, device="cuda")
    dec.decode_i8_device(torch.from_numpy(q).cuda(), hard, 3)
    torch.cuda.synchronize()
    assert np.array_equal(hard.cpu().numpy(), ref8)
    dec.decode_f32_device(torch.from_numpy(y).cuda(), hard, 3, params=default_params(algo=ALGO_MS))
    torch.cuda.synchronize()
    assert dec.last_kernel == "ldsep"
    assert np.array_equal(hard.cpu().numpy(), ref32)
    assert_bits(run_f16(dec, as_device(x), 2, _params("OMS")), host_ref(name, x, 9, 2, "OMS"), "after the others")
    dec.close()
