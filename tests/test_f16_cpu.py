"""The binary16 decode on the host: the half contract.

* the host decoder (``ldpc_decode_f16_soft``) equals the numpy float16
  restatement f16_ref.decode bit for bit -- hard decisions, soft output as
  uint16, iters_used -- on 576x288, 648x324 and two synthetic staircase tables,
  under the three algorithms, with and without early termination, on inputs
  that hold +-0, subnormals, ties, values beyond +-1024, +-65504 and +-inf;
* ``ldpc_convert_f32_f16_host`` over all 65536 binary16 values, the float32
  midpoints between neighbours (ties to even) and the clamp edges;
* the status codes of the f16 entry points on a host context;
* quality against the host float32 decode on paired noise (648x324, 2000
  codewords of the project's float channel with true LLRs, norm = 2 / sigma^2).
  The expectations come from a numpy model of both decoders run on numpy's own
  Gaussian noise (not this channel): at 3.0 dB, 50 iterations of plain min-sum
  -- where float32's |V| reaches 4.7e5, far beyond binary16 -- both lost 0 of
  2000 frames; at 2.0 dB, 20 iterations, the frames whose outcome differs were
  D = 51 (f16 - f32 = -9) under MS and D = 3 (+1) under NMS 0.8125."""
import numpy as np
import pytest

import f16_ref as R
import struct_domain as ST
from ldpcgputegra_amd import ALGO_BP, ALGO_MS, ALGO_NMS, ALGO_OMS, Code, Decoder, LdpcError, _lib, channel, \
    default_params, load_table

ALGO = {"MS": (ALGO_MS, 0.0), "OMS": (ALGO_OMS, 0.375), "NMS": (ALGO_NMS, 0.8125)}
SHIPPED = ("576x288", "648x324")
SYNTH = ("x5_q1_h57", "x20_q3_h18")
BATCH, ITERS = 6, 3


def _table(name):
    return load_table(name) if name in SHIPPED else ST.table(name)


def _host(name, max_batch=64):
    return Decoder(Code(_table(name)), device=-1, max_batch=max_batch)


def _params(algo, early=False):
    a, beta = ALGO[algo]
    return default_params(algo=a, beta=beta, early_term=int(early))


def assert_bits(got, exp, where):
    for g, e, what in zip(got, exp, ("hard", "soft", "iters_used")):
        g = np.asarray(g)
        g = g.view(np.uint16) if g.dtype == np.float16 else g
        assert g.dtype == e.dtype and g.shape == e.shape, (where, what)
        bad = np.flatnonzero((g != e).ravel())
        assert bad.size == 0, "%s: %s differs in %d places, first at %d: %r vs %r" % (
            where, what, bad.size, bad[0], g.ravel()[bad[0]], e.ravel()[bad[0]])


@pytest.mark.parametrize("early", (False, True), ids=("full", "et"))
@pytest.mark.parametrize("algo", sorted(ALGO))
@pytest.mark.parametrize("name", SHIPPED + SYNTH)
def test_host_equals_restatement(name, algo, early):
    t = _table(name)
    x = R.make_input(BATCH, t.n)
    dec = _host(name)
    got = dec.decode_f16_soft(x, ITERS, _params(algo, early))
    assert dec.last_kernel == "host"
    exp = R.decode(t, x, ITERS, algo, ALGO[algo][1], early)
    assert_bits(got, exp, "%s %s early=%s" % (name, algo, early))
    # the plain host-buffer entry point gives the same hard decisions
    assert np.array_equal(dec.decode_f16(x, ITERS, _params(algo, early)), exp[0])
    dec.close()


@pytest.mark.parametrize("name", SYNTH)
def test_host_early_termination_stops(name):
    """On the float early-termination input of struct_domain (-63.5, 3.0 and
    254.0, all binary16 values) codewords stop at different iterations."""
    t = _table(name)
    x = ST.f32_et_input(name).astype(np.float16)
    assert np.array_equal(x.astype(np.float32), ST.f32_et_input(name))
    dec = _host(name, ST.ET_BATCH)
    got = dec.decode_f16_soft(x, ST.ET_ITERS, _params("MS", True))
    exp = R.decode(t, x, ST.ET_ITERS, "MS", 0.0, True)
    assert_bits(got, exp, name)
    assert exp[2].min() < ST.ET_ITERS == exp[2].max()
    dec.close()


def test_input_domain():
    """The shared input holds what the contract names."""
    x = R.make_input(BATCH, 576)
    v = x.view(np.float16).astype(np.float64)
    for u in (0x0000, 0x8000, 0x7C00, 0xFC00, 0x7BFF, 0xFBFF):
        assert (x == u).any(), hex(u)
    sub = (x & 0x7C00) == 0
    assert (sub & ((x & 0x03FF) != 0)).any() and (np.abs(v[np.isfinite(v)]) > 1024).any()
    assert not np.isnan(v).any()


def test_convert_exhaustive():
    allh = np.arange(65536, dtype=np.uint16)
    allh = allh[~np.isnan(allh.view(np.float16))]
    h = allh.view(np.float16)
    y = h.astype(np.float32)                                   # every binary16 value, exactly
    assert np.array_equal(channel.convert_f16_host(y).view(np.uint16), R.bits(R.clamp_v(h)))
    # midpoints between neighbouring finite values: ties go to the even mantissa
    fin = np.sort(h[np.isfinite(h)].astype(np.float64))
    mid = ((fin[:-1] + fin[1:]) / 2).astype(np.float32)
    assert np.array_equal(mid.astype(np.float64), (fin[:-1] + fin[1:]) / 2)    # exact in float32
    got = channel.convert_f16_host(mid)
    assert np.array_equal(got.view(np.uint16), R.bits(R.convert(mid)))
    inside = np.abs(mid) < 1024
    assert (got.view(np.uint16)[inside] & 1 == 0).all()
    # one float32 ulp to either side of a midpoint rounds to the nearer neighbour
    for d in (-np.inf, np.inf):
        off = np.nextafter(mid, np.float32(d))
        assert np.array_equal(channel.convert_f16_host(off).view(np.uint16), R.bits(R.convert(off)))
    # the clamp edges
    edge = np.array([1024.0, np.nextafter(np.float32(1024), np.float32(2000)), 1024.5, 65504.0, 65520.0, 1e30, np.inf,
                     -1024.0, -1024.5, -65520.0, -1e30, -np.inf, 1023.75, -1023.75, 1e-8, -1e-8, 1e-40, -1e-40],
                    dtype=np.float32)
    got = channel.convert_f16_host(edge)
    assert np.array_equal(got.view(np.uint16), R.bits(R.convert(edge)))
    assert (np.abs(got.astype(np.float32)) <= 1024).all()
    assert got.view(np.uint16)[-1] == 0x8000 and got.view(np.uint16)[-3] == 0x8000
    assert channel.convert_f16_host(np.zeros((0,), dtype=np.float32)).size == 0


def test_convert_args():
    L = _lib.lib()
    y = np.zeros(4, dtype=np.float32)
    h = np.full(4, 7, dtype=np.uint16)
    assert L.ldpc_convert_f32_f16_host(None, None, 0) == _lib.LDPC_OK
    assert L.ldpc_convert_f32_f16_host(y.ctypes.data, h.ctypes.data, 0) == _lib.LDPC_OK and (h == 7).all()
    assert L.ldpc_convert_f32_f16_host(None, h.ctypes.data, 4) == _lib.LDPC_EINVAL
    assert L.ldpc_convert_f32_f16_host(y.ctypes.data, None, 4) == _lib.LDPC_EINVAL
    assert L.ldpc_convert_f32_f16_host(y.ctypes.data, h.ctypes.data, -1) == _lib.LDPC_EINVAL
    assert (h == 7).all()


def test_status_codes_host_context():
    import ctypes as C
    name = "576x288"
    n = _table(name).n
    dec = _host(name, max_batch=4)
    x = R.make_input(4, n)

    def status(fn):
        with pytest.raises(LdpcError) as e:
            fn()
        return e.value.status

    assert status(lambda: dec.decode_f16_soft(x, 2, default_params(algo=ALGO_BP))) == _lib.LDPC_EUNSUPPORTED
    assert status(lambda: dec.decode_f16(x, 2, default_params(algo=ALGO_BP))) == _lib.LDPC_EUNSUPPORTED
    for beta in (-0.5, float("inf"), float("nan"), 65520.0, 1e6):
        for algo in (ALGO_OMS, ALGO_NMS):
            assert status(lambda: dec.decode_f16_soft(x, 2, default_params(algo=algo, beta=beta))) == \
                _lib.LDPC_EINVAL, beta
    # plain min-sum ignores beta; the int8 fields are ignored altogether
    ref = dec.decode_f16_soft(x, 2, default_params(algo=ALGO_MS))
    odd = dec.decode_f16_soft(x, 2, default_params(algo=ALGO_MS, beta=-3.0, var_max=5, var_min=-500, msg_max=999,
                                                   offset=-4, factor=-9))
    assert all(np.array_equal(a, b) for a, b in zip(ref, odd))
    assert np.array_equal(dec.decode_f16_soft(x, 2, default_params(algo=ALGO_OMS, beta=65504.0))[0].shape, (4, n))
    assert status(lambda: dec.decode_f16_soft(R.make_input(5, n), 2)) == _lib.LDPC_EINVAL      # batch > max_batch
    assert status(lambda: dec.decode_f16_soft(x, -1)) == _lib.LDPC_EINVAL
    # batch 0 touches nothing
    p = default_params(algo=ALGO_MS)
    assert _lib.lib().ldpc_decode_f16_soft(dec._ctx, None, None, None, None, 0, 2, C.byref(p)) == _lib.LDPC_OK
    assert _lib.lib().ldpc_decode_f16(dec._ctx, None, None, 0, 2, C.byref(p)) == _lib.LDPC_OK
    assert _lib.lib().ldpc_decode_f16(dec._ctx, None, None, 1, 2, C.byref(p)) == _lib.LDPC_EINVAL
    # the device-buffer entry points need a GPU context
    assert _lib.lib().ldpc_decode_f16_async(dec._ctx, None, x.ctypes.data, None, None, None, 1, 2, C.byref(p)) == \
        _lib.LDPC_EUNSUPPORTED
    assert _lib.lib().ldpc_convert_f32_f16_async(dec._ctx, None, x.ctypes.data, x.ctypes.data, 1) == \
        _lib.LDPC_EUNSUPPORTED
    assert dec.last_kernel == "host"
    dec.close()


# ---- quality on paired noise ---------------------------------------------------

QN, QFRAMES = "648x324", 2000
_q = {}


def _outcomes(ebn0, iters, algo, beta):
    """(frame lost in f32 [F] bool, frame lost in f16 [F] bool): the host
    decoders on the same channel samples, all-zero codeword, errors counted over
    the K information positions."""
    key = (ebn0, iters, algo, beta)
    if key not in _q:
        t = load_table(QN)
        k = t.n - t.m
        sigma = channel.sigma_from_ebn0(ebn0, k / t.n)
        y = channel.awgn_f32_host(t.n, QFRAMES, seed=11, sigma=sigma, normalize=True)
        dec = Decoder(Code(QN), device=-1, max_batch=QFRAMES)
        p = default_params(algo=algo, beta=beta)
        h32 = dec.decode_f32(y, iters, p)
        h16 = dec.decode_f16(channel.convert_f16_host(y), iters, p)
        dec.close()
        _q[key] = (h32[:, :k].any(axis=1), h16[:, :k].any(axis=1))
    return _q[key]


def test_quality_saturation():
    """3.0 dB, 50 iterations of plain min-sum: float32's V grows far beyond
    binary16's range; with V clamped at 1024 and the messages at 256 the f16
    decode loses no frame that float32 does not lose."""
    fe32, fe16 = _outcomes(3.0, 50, ALGO_MS, 0.0)
    print("saturation: FE32 %d FE16 %d of %d, lost by f16 alone %d" % (fe32.sum(), fe16.sum(), QFRAMES,
                                                                       (fe16 & ~fe32).sum()))
    assert not (fe16 & ~fe32).any()


@pytest.mark.parametrize("algo", ("MS", "NMS"))
def test_quality_paired_count(algo):
    """2.0 dB, 20 iterations: with D the frames whose outcome differs between
    the two decoders, FE16 - FE32 <= 3 sqrt(D) (under equal quality the
    difference of the paired counts has standard deviation sqrt(D)), and
    D <= 10 % of the frames."""
    fe32, fe16 = _outcomes(2.0, 20, *ALGO[algo])
    D = int((fe32 != fe16).sum())
    diff = int(fe16.sum()) - int(fe32.sum())
    print("%s: FE32 %d FE16 %d of %d, D %d, difference %+d" % (algo, fe32.sum(), fe16.sum(), QFRAMES, D, diff))
    assert D <= QFRAMES // 10
    assert diff <= 3.0 * np.sqrt(D)
