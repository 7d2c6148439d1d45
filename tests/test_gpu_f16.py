"""The binary16 decode on the GPU: the packed half-precision staircase kernel
against the host decoder, which defines the half contract and
which test_f16_cpu.py ties to its numpy restatement.

* kernel == host decoder bit for bit (hard, soft as uint16, iters_used) on one
  synthetic table per X in {5, 8, 12, 20, 25, 28} (struct_domain.CORE), at
  every group width the table has (LDPC_STAIRF_S), batches 1, 17, 65 and 130
  (a half-filled pair, a lone codeword, a partial wave, more than one wave), 1,
  2 and 5 iterations, the three algorithms, on f16_ref.make_input (+-0,
  subnormals, ties, values beyond +-1024, +-65504, +-inf);
* early termination on struct_domain.ET_TABLES' stairf tables, where the two
  codewords of a pair stop at different iterations;
* every shipped DVB-S2 and shaped code once (3 codewords, 2 iterations);
* device conversion == host conversion;
* the buffer contract on 2-byte aligned slices: guard rows and the bytes around
  every output untouched, batch 0 writes nothing;
* status codes; scratch shared with a float32 decode on the same context."""
import ctypes as C

import numpy as np
import pytest

import f16_ref as R
import struct_domain as ST
from ldpcgputegra_amd import ALGO_BP, ALGO_MS, ALGO_NMS, ALGO_OMS, Code, Decoder, LdpcError, _lib, channel, \
    default_params, load_table

pytestmark = pytest.mark.gpu

ALGO = {"MS": (ALGO_MS, 0.0), "OMS": (ALGO_OMS, 0.375), "NMS": (ALGO_NMS, 0.8125)}
TABLE_OF_X = {5: "x5_q1_h57", 8: "x8_q5_h110", 12: "x12_q5_h110", 20: "x20_q3_h18", 25: "x25_q3_h33", 28: "x28_q6_h6"}
BATCHES = (1, 17, 65, 130)
ITERS = (1, 2, 5)
SHIPPED = ("dvbs2_r1_2", "dvbs2_r2_3", "dvbs2_r8_9", "dvbs2_r9_10", "dvbs2shape_r3_4", "dvbs2shape_r5_6")
SOFT_FILL, HARD_FILL, ITS_FILL = 0x1234, 9, -7
_host_ref = {}


def _torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def _table(name):
    return load_table(name) if name in SHIPPED or name[0].isdigit() else ST.table(name)


def _params(algo, early=False):
    a, beta = ALGO[algo]
    return default_params(algo=a, beta=beta, early_term=int(early))


def host_ref(name, x, key, iters, algo, early=False):
    """(hard, soft uint16, iters_used) of the host decoder, cached per input key"""
    k = (name, key, iters, algo, early)
    if k not in _host_ref:
        dec = Decoder(Code(_table(name)), device=-1, max_batch=x.shape[0])
        hard, soft, its = dec.decode_f16_soft(x, iters, _params(algo, early))
        dec.close()
        out = (hard, soft.view(np.uint16), its)
        for a in out:
            a.setflags(write=False)
        _host_ref[k] = out
    return _host_ref[k]


def as_device(x):
    """uint16 bit patterns -> a float16 device tensor"""
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


@pytest.mark.parametrize("X", sorted(TABLE_OF_X))
def test_kernel_equals_host(X, monkeypatch):
    name = TABLE_OF_X[X]
    t = _table(name)
    assert t.group_deg[0] == X + 2
    widths = ST.widths(name)
    assert widths, name
    dec = Decoder(Code(t), max_batch=max(BATCHES))
    for batch in BATCHES:
        x = R.make_input(batch, t.n)
        d = as_device(x)
        for iters in ITERS:
            for algo in sorted(ALGO):
                exp = host_ref(name, x, batch, iters, algo)
                for S in widths:
                    monkeypatch.setenv("LDPC_STAIRF_S", str(S))
                    got = run_f16(dec, d, iters, _params(algo))
                    assert dec.last_kernel == "stairf"
                    assert_bits(got, exp, "%s batch %d, %d iterations, %s, width %d" % (name, batch, iters, algo, S))
    monkeypatch.delenv("LDPC_STAIRF_S", raising=False)
    got = run_f16(dec, as_device(R.make_input(17, t.n)), 2, _params("MS"))       # the width rule's own choice
    assert_bits(got, host_ref(name, R.make_input(17, t.n), 17, 2, "MS"), name + " automatic width")
    dec.close()


@pytest.mark.parametrize("name", ST.ET_TABLES_F32)
def test_early_termination(name, monkeypatch):
    """struct_domain.f32_et_input (-63.5, 3.0, 254.0: binary16 values): three
    codewords of four stop after 1 or 2 iterations, every fourth never, so the
    halves of a pair differ in being alive.  Every width, the three algorithms."""
    t = _table(name)
    x = R.bits(ST.f32_et_input(name).astype(np.float16))
    d = as_device(x)
    dec = Decoder(Code(t), max_batch=ST.ET_BATCH)
    for algo in sorted(ALGO):
        exp = host_ref(name, x, "et", ST.ET_ITERS, algo, early=True)
        if algo == "MS":
            its = exp[2]
            assert its.min() < ST.ET_ITERS == its.max()
            assert (its[0:-1:2] != its[1::2]).any(), "no pair whose halves stop at different iterations"
        for S in ST.widths(name):
            monkeypatch.setenv("LDPC_STAIRF_S", str(S))
            got = run_f16(dec, d, ST.ET_ITERS, _params(algo, early=True))
            assert_bits(got, exp, "%s early termination %s width %d" % (name, algo, S))
    dec.close()


@pytest.mark.parametrize("name", SHIPPED)
def test_shipped_codes(name):
    t = _table(name)
    x = R.make_input(3, t.n)
    dec = Decoder(Code(name), max_batch=64)
    got = run_f16(dec, as_device(x), 2, _params("OMS"))
    assert dec.last_kernel == "stairf"
    assert_bits(got, host_ref(name, x, 3, 2, "OMS"), name)
    # the host-buffer entry point: copy in, decode, copy out
    assert np.array_equal(dec.decode_f16(x, 2, _params("OMS")), got[0])
    dec.close()


def test_convert_device_equals_host():
    torch = _torch()
    allh = np.arange(65536, dtype=np.uint16)
    h = allh[~np.isnan(allh.view(np.float16))].view(np.float16)
    fin = np.sort(h[np.isfinite(h)].astype(np.float64))
    mid = ((fin[:-1] + fin[1:]) / 2).astype(np.float32)
    rnd = ((R.make_input(4, 4096).astype(np.float32) - 32768.0) / 16.0).ravel().astype(np.float32)
    edge = np.array([1024.5, 65504.0, 65520.0, 1e30, np.inf, -1024.5, -65520.0, -1e30, -np.inf, 1e-8, -1e-8, 1e-40,
                     -1e-40, 0.0, -0.0], dtype=np.float32)
    y = np.concatenate([h.astype(np.float32), mid, np.nextafter(mid, np.float32(np.inf)),
                        np.nextafter(mid, np.float32(-np.inf)), rnd, edge])
    exp = channel.convert_f16_host(y).view(np.uint16)
    dec = Decoder(Code(_table(TABLE_OF_X[5])), max_batch=64)
    buf_y = torch.zeros(y.size + 1, dtype=torch.float32, device="cuda")
    buf_h = torch.full((y.size + 3,), SOFT_FILL, dtype=torch.int16, device="cuda")
    d_y, d_h = buf_y[1:], buf_h[1:1 + y.size]                 # 4-byte and 2-byte aligned slices
    d_y.copy_(torch.from_numpy(y))
    dec.convert_f16_device(d_y, d_h.view(torch.float16))
    torch.cuda.synchronize()
    out = buf_h.cpu().numpy().view(np.uint16)
    assert np.array_equal(out[1:1 + y.size], exp)
    assert out[0] == SOFT_FILL and (out[1 + y.size:] == SOFT_FILL).all()
    # count 0 touches nothing and takes NULL pointers
    assert _lib.lib().ldpc_convert_f32_f16_async(dec._ctx, None, None, None, 0) == _lib.LDPC_OK
    assert _lib.lib().ldpc_convert_f32_f16_async(dec._ctx, None, None, None, 4) == _lib.LDPC_EINVAL
    assert _lib.lib().ldpc_convert_f32_f16_async(dec._ctx, None, C.c_void_p(d_y.data_ptr()),
                                                 C.c_void_p(d_h.data_ptr()), -1) == _lib.LDPC_EINVAL
    dec.close()


@pytest.mark.parametrize("batch", (0, 1, 3, 64, 65))
def test_buffer_contract(batch):
    """Inputs and outputs are slices starting 2 bytes (binary16), 1 byte (hard)
    and 4 bytes (iters_used) into larger buffers; everything outside the
    [batch] rows keeps its fill."""
    torch = _torch()
    name = TABLE_OF_X[8]
    t = _table(name)
    n, rows = t.n, 66
    x = R.make_input(max(batch, 1), n)[:batch]
    dec = Decoder(Code(t), max_batch=rows)
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
    if batch:
        exp = host_ref(name, x, ("contract", batch), 2, "NMS")
        got = (hard[1:1 + batch * n].reshape(batch, n), soft[1:1 + batch * n].reshape(batch, n), its[1:1 + batch])
        assert_bits(got, exp, "%s batch %d on unaligned slices" % (name, batch))
    dec.close()


def _status(fn):
    with pytest.raises(LdpcError) as e:
        fn()
    return e.value.status, str(e.value)


def test_status_codes():
    torch = _torch()
    name = TABLE_OF_X[5]
    t = _table(name)
    d = as_device(R.make_input(4, t.n))
    hard = torch.zeros((4, t.n), dtype=torch.uint8, device="cuda")
    dec = Decoder(Code(t), max_batch=64)
    dec.decode_f16_device(d, hard, 1)
    torch.cuda.synchronize()
    assert dec.last_kernel == "stairf"
    # belief propagation, beta
    assert _status(lambda: dec.decode_f16_device(d, hard, 1, params=default_params(algo=ALGO_BP)))[0] == \
        _lib.LDPC_EUNSUPPORTED
    for beta in (-0.5, float("inf"), float("nan"), 65520.0):
        for algo in (ALGO_OMS, ALGO_NMS):
            assert _status(lambda: dec.decode_f16_device(d, hard, 1, params=default_params(algo=algo, beta=beta)))[0] \
                == _lib.LDPC_EINVAL, beta
    # a forced family other than stairf is not applicable; stairf forced is
    for k in (1, 2, 3, 5, 8):
        try:
            dec.set_kernel(k)
        except LdpcError:
            continue          # the family refuses this table altogether
        st, msg = _status(lambda: dec.decode_f16_device(d, hard, 1))
        assert st == _lib.LDPC_EUNSUPPORTED and "not applicable" in msg, (k, msg)
    dec.set_kernel(11)
    dec.decode_f16_device(d, hard, 1)
    dec.set_kernel(0)
    torch.cuda.synchronize()
    # a host context takes no device buffers
    host = Decoder(Code(t), device=-1, max_batch=64)
    assert _status(lambda: host.decode_f16_device(d, hard, 1))[0] == _lib.LDPC_EUNSUPPORTED
    host.close()
    dec.close()
    # a code without a staircase table
    n2 = _table("648x324").n
    other = Decoder(Code("648x324"), max_batch=64)
    st, msg = _status(lambda: other.decode_f16_device(as_device(R.make_input(2, n2)),
                                                      torch.zeros((2, n2), dtype=torch.uint8, device="cuda"), 1))
    assert st == _lib.LDPC_EUNSUPPORTED and "staircase" in msg
    other.close()


def test_stride_limit():
    """(n + 1) * stride * 2 < 2^32: at n = 64800 strides up to 33088 pass, 33152
    does not.  The refusal comes before anything is allocated or read."""
    torch = _torch()
    big = Decoder(Code("dvbs2_r1_2"), max_batch=33152)
    d = torch.zeros((4, 64800), dtype=torch.float16, device="cuda")
    p = default_params(algo=ALGO_MS)
    rc = _lib.lib().ldpc_decode_f16_async(big._ctx, None, C.c_void_p(d.data_ptr()), None, None, None, 33089, 1,
                                          C.byref(p))
    assert rc == _lib.LDPC_EUNSUPPORTED and b"2^32" in _lib.lib().ldpc_last_error()
    big.close()


def test_scratch_shared_with_float32():
    """A float32 decode (and an early-terminated one) on the context between two
    f16 decodes: the f16 results equal a fresh context's."""
    torch = _torch()
    name = TABLE_OF_X[12]
    t = _table(name)
    x = R.make_input(65, t.n)
    d = as_device(x)
    exp = host_ref(name, x, 65, 2, "OMS")
    dec = Decoder(Code(t), max_batch=130)
    y = torch.from_numpy(np.array(ST.f32_input(130, t.n))).cuda()
    hard32 = torch.zeros((130, t.n), dtype=torch.uint8, device="cuda")
    dec.decode_f32_device(y, hard32, 3, params=default_params(algo=ALGO_MS, early_term=1))
    assert_bits(run_f16(dec, d, 2, _params("OMS")), exp, "after a float32 decode")
    dec.decode_f32_device(y, hard32, 3)
    torch.cuda.synchronize()
    ref32 = hard32.cpu().numpy().copy()
    assert_bits(run_f16(dec, d, 2, _params("OMS", early=False)), exp, "after a second float32 decode")
    exp_et = host_ref(name, x, 65, 2, "OMS", early=True)
    assert_bits(run_f16(dec, d, 2, _params("OMS", early=True)), exp_et, "early termination after float32")
    dec.decode_f32_device(y, hard32, 3)                       # and float32 after f16 is unchanged too
    torch.cuda.synchronize()
    assert np.array_equal(hard32.cpu().numpy(), ref32)
    dec.close()
