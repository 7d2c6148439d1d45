"""The float AWGN channel's host twin (ldpc_awgn_f32_host, generator in
ldpcgputegra_amd/csrc/awgn_f32.h) against a numpy / scipy restatement:

    u = splitmix64(((first_cw + b) * N + i) ^ (seed * 0xD1B54A32D192ED03)) >> 32
    z = Phi^-1((u + 0.5) * 2^-32),   y = float32(norm * (-amp + sigma * z))

A test reaches a chosen u through first_cw: splitmix64 is a bijection, so
awgn_f32_domain.index_of(u) is an element index with that u, and a call with
n = 1, batch = 1 and first_cw = index draws exactly it.

Reading z itself through a float output: for z > 0, sigma = norm = 1 and an amp
within a factor 2 of z make t = z - amp exact (Sterbenz).  With amp1 = the
expected z cut to 20 bits, y1 = float(z - amp1) holds the next 24 bits; with
amp2 = amp1 + y1 the rest, z - amp2, is a multiple of ulp(z) below 2^-44 z and
so a float: z = amp2 + y2 exactly.  For z < 0 nothing cancels (both terms of
-amp + sigma z are negative), so the lower half is checked through its float
images: y(2^32 - 1 - u) must be float32(norm * (-amp - sigma * z(u))) bit for
bit, z(u) being the exact value read in the upper half."""
import ctypes as C

import numpy as np
import pytest
from scipy.stats import norm as N01

import awgn_f32_domain as D
from ldpcgputegra_amd import _lib, channel

SEED = 3
TOP = (1 << 32) - 1


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def structured_u():
    """Every power of two +- 1 and its mirror image, 2^16 equally spaced values,
    the generator's region boundaries +- 2."""
    s = set()
    for k in range(33):
        for d in (-1, 0, 1):
            v = (1 << k) + d
            if 0 <= v <= TOP:
                s.update((v, TOP - v))
    s.update(range(1 << 15, 1 << 32, 1 << 16))
    for b in (D.U_LO, D.U_HI, (1 << 31) - 1):
        s.update(v for v in range(b - 2, b + 4) if 0 <= v <= TOP)
    return s


_out = np.empty(1, dtype=np.float32)


def sample(u, sigma, amp, norm=1.0):
    """The host twin's y at one chosen u (bit 0)."""
    _lib.check(_lib.lib().ldpc_awgn_f32_host(1, 1, D.index_of(u, SEED), SEED, sigma, amp, norm, None,
                                             _out.ctypes.data))
    return _out[0]


@pytest.fixture(scope="module")
def upper():
    """(u sorted, exact z) for the structured set folded into u >= 2^31."""
    us = np.array(sorted({u if u >= 1 << 31 else TOP - u for u in structured_u()}), dtype=np.uint64)
    zref = N01.ppf((us.astype(np.float64) + 0.5) * 2.0 ** -32)
    z = np.empty(len(us))
    for i, (u, zr) in enumerate(zip(us.tolist(), zref.tolist())):
        m, e = np.frexp(zr)
        amp1 = float(np.ldexp(np.round(m * 2.0 ** 20), e - 20))
        amp2 = amp1 + float(sample(u, 1.0, amp1))
        z[i] = amp2 + float(sample(u, 1.0, amp2))
    return us, z, zref


@pytest.mark.parametrize("n,batch", [(648, 8), (200, 5)])
@pytest.mark.parametrize("first_cw", [0, 5, 1 << 33])
@pytest.mark.parametrize("mode", ["bpsk", "qpsk", "normalised"])
def test_definition(n, batch, first_cw, mode):
    amp = D.QPSK if mode == "qpsk" else 1.0
    normalize = mode == "normalised"
    norm = 2.0 / D.SIGMA_1DB ** 2 if normalize else 1.0
    got = channel.awgn_f32_host(n, batch, SEED, D.SIGMA_1DB, amp=amp, normalize=normalize, first_cw=first_cw)
    exp, excusable = D.restate(n, batch, SEED, D.SIGMA_1DB, amp, norm, first_cw)
    differ = bits(got) != bits(exp)
    assert not (differ & ~excusable).any()
    # a difference is excused only within 1e-9 (relative) of a float rounding boundary, and rarely
    assert differ.sum() <= 1e-3 * n * batch


def test_accuracy_upper_half(upper):
    us, z, zref = upper
    assert len(us) > 1 << 16
    err = np.abs(z - zref)
    assert (err <= 1e-9 * np.maximum(1.0, np.abs(z))).all(), err.max()
    # the exact read-back is self-consistent: the float image of z is what a plain call gives
    for i in range(0, len(us), 997):
        assert sample(int(us[i]), 1.0, 2.0 ** -80) == np.float32(-(2.0 ** -80) + z[i])


def test_order_upper_half(upper):
    us, z, _ = upper
    assert (np.diff(z) >= 0).all() and z[0] > 0
    # strictly increasing wherever Phi^-1 moves by more than its 1e-9 error bound: everywhere on this set
    assert (np.diff(z) > 0).all()


@pytest.mark.parametrize("sigma,amp,norm", [(1.0, 2.0 ** -80, 1.0), (D.SIGMA_1DB, 1.0, 1.0),
                                            (D.SIGMA_1DB, D.QPSK, 2.0 / D.SIGMA_1DB ** 2)])
def test_antisymmetry_and_lower_half(upper, sigma, amp, norm):
    """y(2^32 - 1 - u) is the float image of -z(u): the lower half's accuracy and
    order are the upper half's."""
    us, z, _ = upper
    got = np.array([sample(TOP - u, sigma, amp, norm) for u in us.tolist()], dtype=np.float32)
    exp = (norm * (-amp + sigma * -z)).astype(np.float32)
    assert np.array_equal(bits(got), bits(exp))
    assert (np.diff(got[::-1]) >= 0).all()      # us ascending -> mirrors descending


def test_tails():
    assert {u for _, _, u in D.TAILS} >= {0, TOP}
    for first_cw, pos, u in D.TAILS:
        assert u < 1 << 6 or u > TOP - (1 << 6)
        assert int(D.u_of(D.TAIL_N, 1, D.TAIL_SEED, first_cw)[0, pos]) == u
        got = channel.awgn_f32_host(D.TAIL_N, 1, D.TAIL_SEED, D.SIGMA_1DB, first_cw=first_cw)
        exp, excusable = D.restate(D.TAIL_N, 1, D.TAIL_SEED, D.SIGMA_1DB, first_cw=first_cw)
        assert bits(got)[0, pos] == bits(exp)[0, pos] or excusable[0, pos]
        assert not ((bits(got) != bits(exp)) & ~excusable).any()
    # 32 bits of u bound |z|: the extreme samples, sigma = 1, amp negligible
    zmax = float(sample(TOP, 1.0, 2.0 ** -80))
    assert 6.33 < zmax < 6.34 and float(sample(0, 1.0, 2.0 ** -80)) == -zmax


def test_codeword_bits_negate():
    n, batch = 200, 5
    cw = (np.random.default_rng(1).integers(0, 2, (batch, n))).astype(np.uint8)
    zero = channel.awgn_f32_host(n, batch, SEED, D.SIGMA_1DB)
    assert np.array_equal(bits(zero), bits(channel.awgn_f32_host(n, batch, SEED, D.SIGMA_1DB,
                                                                 codeword=np.zeros_like(cw))))
    got = channel.awgn_f32_host(n, batch, SEED, D.SIGMA_1DB, codeword=cw)
    assert np.array_equal(bits(got), bits(np.where(cw != 0, -zero, zero)))
    # any non-zero byte is a 1, as in the int8 channel
    assert np.array_equal(bits(got), bits(channel.awgn_f32_host(n, batch, SEED, D.SIGMA_1DB, codeword=cw * 255)))


def test_slicing():
    n = 648
    whole = channel.awgn_f32_host(n, 64, SEED, D.SIGMA_1DB)
    halves = [channel.awgn_f32_host(n, 32, SEED, D.SIGMA_1DB, first_cw=f) for f in (0, 32)]
    assert np.array_equal(bits(whole), bits(np.concatenate(halves)))
    assert not np.array_equal(whole[:32], whole[32:])


def int8_differences(n, batch, seed, sigma, amp=1.0, normalize=False, first_cw=0):
    """quantised float channel minus the int8 channel, per sample (the table's
    norm is part of the float channel's y already)."""
    y = channel.awgn_f32_host(n, batch, seed, sigma, amp=amp, normalize=normalize, first_cw=first_cw)
    q = channel.awgn_i8_host(n, batch, seed, channel.i8_table(sigma, amp=amp, normalize=normalize),
                             first_cw=first_cw)
    return D.quantize(y).astype(np.int32) - q.astype(np.int32)


@pytest.mark.parametrize("n,batch,amp,normalize", [(648, 1024, 1.0, False), (64800, 4, 1.0, False),
                                                   (648, 1024, D.QPSK, True)])
def test_quantised_float_channel_is_the_int8_channel(n, batch, amp, normalize):
    """clip(trunc(8 y), +-31) of the float channel against awgn_i8_host on the
    same (seed, first_cw): they differ at most at the edge of a quantisation
    cell (one u per threshold, plus the float-rounding band of y: about 2e-6
    of the samples), and then by one level."""
    d = int8_differences(n, batch, 1, D.SIGMA_1DB, amp, normalize)
    assert np.count_nonzero(d) <= 1e-5 * d.size
    assert (np.abs(d) <= 1).all()


def test_sim_seed_has_no_cell_edge_sample():
    """What tests/test_sim_f32.py runs through ldpc_sim (648x324 at D.SIM_EBN0
    dB, seed D.SIM_SEED, frames 0 .. D.SIM_FRAMES - 1): the two host twins agree
    on every byte, so the -f32q chain must count what the int8 chain counts."""
    sigma = channel.sigma_from_ebn0(D.SIM_EBN0, 324 / 648)
    assert not int8_differences(648, D.SIM_FRAMES, D.SIM_SEED, sigma).any()


def test_argument_checks():
    L = _lib.lib()
    y = np.zeros(8, dtype=np.float32)
    ok = (4, 2, 0, 1, 0.9, 1.0, 1.0, None, y.ctypes.data)

    def call(**kw):
        a = dict(zip(("n", "batch", "first_cw", "seed", "sigma", "amp", "norm", "cw", "y"), ok))
        a.update(kw)
        return L.ldpc_awgn_f32_host(*a.values())

    assert call() == _lib.LDPC_OK
    for bad in (dict(y=None), dict(batch=-1), dict(sigma=0.0), dict(sigma=-1.0), dict(amp=0.0), dict(amp=-1.0),
                dict(norm=0.0), dict(norm=-2.0), dict(sigma=float("nan")), dict(n=0)):
        assert call(**bad) == _lib.LDPC_EINVAL, bad
    # batch 0 writes nothing
    y[:] = 7.0
    assert call(batch=0) == _lib.LDPC_OK and (y == 7.0).all()
    with pytest.raises(_lib.LdpcError):
        channel.awgn_f32_host(4, 2, 1, sigma=0.0)


def test_host_context_refuses_device_buffers():
    """A host context (device -1) gets the refusal every device-buffer entry gives."""
    from ldpcgputegra_amd import Code, Decoder
    dec = Decoder(Code("200x100"), device=-1, max_batch=4)
    y = np.zeros(200, dtype=np.float32)
    r = _lib.lib().ldpc_awgn_f32_async(dec._ctx, None, y.ctypes.data, 1, 0, 1, 0.9, 1.0, 1.0, None)
    assert r == _lib.LDPC_EUNSUPPORTED
    assert b"device buffers need a GPU" in _lib.lib().ldpc_last_error()
    assert _lib.lib().ldpc_awgn_f32_async(dec._ctx, None, None, 1, 0, 1, 0.9, 1.0, 1.0, None) == _lib.LDPC_EINVAL
    dec.close()
