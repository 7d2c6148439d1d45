"""The float AWGN channel on the device (awgn_f32_k through
ldpc_awgn_f32_async) against its host twin, bit for bit: the generator is one
header (ldpcgputegra_amd/csrc/awgn_f32.h) compiled for both sides, built from
integer work and IEEE double + - * / sqrt only, so every sample must agree
exactly -- f64 division and square root of the device included.  The host twin
itself is checked against scipy in test_awgn_f32_cpu.py."""
import ctypes as C

import numpy as np
import pytest

import awgn_f32_domain as D
import oracle as O
from ldpcgputegra_amd import ALGO_MS, Code, Decoder, _lib, channel, default_params, load_table
from ldpcgputegra_amd.codes import Table

pytestmark = pytest.mark.gpu

SEED = 3
SENTINEL = 12345.0
# an odd N: 67 checks of degree 3 over 201 variables (no row of y but the first is 16-byte aligned)
ODD = Table(201, 67, [(3, 67)], np.arange(201, dtype=np.uint32))
_decoders = {}


def _torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def decoder(code):
    if code not in _decoders:
        _decoders[code] = Decoder(Code(ODD if code == "odd" else code), max_batch=1024)
    return _decoders[code]


def n_of(code):
    return ODD.n if code == "odd" else load_table(code).n


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def device_channel(code, batch, first_cw, sigma, amp=1.0, normalize=False, codeword=None, offset=0, seed=SEED):
    """(y, before, after): the device channel's output written `offset` floats
    into a sentinel-filled, 256-byte aligned buffer, and the sentinels around it."""
    torch = _torch()
    n = n_of(code)
    big = torch.full((offset + batch * n + 64,), SENTINEL, dtype=torch.float32, device="cuda")
    assert big.data_ptr() % 256 == 0
    y = big[offset:offset + batch * n].view(batch, n)
    cw = None if codeword is None else torch.from_numpy(codeword).cuda()
    decoder(code).awgn_f32_device(y, first_cw, seed, sigma, amp=amp, normalize=normalize, codeword=cw)
    torch.cuda.synchronize()
    out = big.cpu().numpy()
    return out[offset:offset + batch * n].reshape(batch, n), out[:offset], out[offset + batch * n:]


MODES = {"bpsk": (1.0, False), "qpsk": (D.QPSK, False), "normalised": (1.0, True)}


@pytest.mark.parametrize("code,batch,first_cw", [("648x324", 1, 0), ("648x324", 37, 5), ("200x100", 5, 1 << 33),
                                                 ("odd", 7, 3), ("dvbs2_r1_2", 3, 0)])
@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("with_codeword", [False, True])
def test_device_equals_host(code, batch, first_cw, mode, with_codeword):
    amp, normalize = MODES[mode]
    n = n_of(code)
    cw = np.random.default_rng(batch).integers(0, 2, (batch, n)).astype(np.uint8) if with_codeword else None
    exp = channel.awgn_f32_host(n, batch, SEED, D.SIGMA_1DB, amp=amp, normalize=normalize, first_cw=first_cw,
                                codeword=cw)
    got, _, after = device_channel(code, batch, first_cw, D.SIGMA_1DB, amp, normalize, cw)
    assert np.array_equal(bits(got), bits(exp))
    assert (after == SENTINEL).all()


def test_tail_indices():
    """u below 2^6 and above 2^32 - 2^6: the longest logarithms and square roots."""
    for first_cw, pos, u in D.TAILS:
        exp = channel.awgn_f32_host(D.TAIL_N, 1, D.TAIL_SEED, D.SIGMA_1DB, first_cw=first_cw)
        got, _, _ = device_channel("648x324", 1, first_cw, D.SIGMA_1DB, seed=D.TAIL_SEED)
        assert np.array_equal(bits(got), bits(exp))
        assert abs(float(got[0, pos])) > 3.9 and (got[0, pos] < 0) == (u < 1 << 31)


@pytest.mark.parametrize("offset", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("code,batch", [("odd", 7), ("648x324", 3)])
def test_buffers(code, batch, offset):
    """Output slices 0 .. 16 bytes past a 16-byte boundary: offset 4 and 0 store
    float4 throughout (a ragged end aside), 1 .. 3 store the first lane's
    elements one by one and float4 from the next boundary on.  The values do
    not depend on the path; the floats around [batch][N] keep their sentinel."""
    exp = channel.awgn_f32_host(n_of(code), batch, SEED, D.SIGMA_1DB)
    got, before, after = device_channel(code, batch, 0, D.SIGMA_1DB, offset=offset)
    assert np.array_equal(bits(got), bits(exp))
    assert (before == SENTINEL).all() and (after == SENTINEL).all()


def test_batch_zero_is_a_noop():
    torch = _torch()
    big = torch.full((648 + 8,), SENTINEL, dtype=torch.float32, device="cuda")
    # through the C-ABI: torch gives an empty view a NULL data pointer, which the entry refuses
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream or None)
    assert _lib.lib().ldpc_awgn_f32_async(decoder("648x324")._ctx, stream, C.c_void_p(big.data_ptr() + 16), 0, 0,
                                          SEED, D.SIGMA_1DB, 1.0, 1.0, None) == _lib.LDPC_OK
    torch.cuda.synchronize()
    assert bool((big == SENTINEL).all())


def test_chain_quantised_float_channel_is_the_int8_channel():
    torch = _torch()
    n, batch = 648, 1024
    dec = decoder("648x324")
    y = torch.empty((batch, n), dtype=torch.float32, device="cuda")
    q = torch.empty((batch, n), dtype=torch.int8, device="cuda")
    llr = torch.empty((batch, n), dtype=torch.int8, device="cuda")
    dec.awgn_f32_device(y, 0, 1, D.SIGMA_1DB)
    dec.quantize_device(y, q)
    dec.awgn_i8_device(llr, 0, 1, channel.i8_table(D.SIGMA_1DB))
    torch.cuda.synchronize()
    d = q.cpu().numpy().astype(np.int32) - llr.cpu().numpy().astype(np.int32)
    assert np.count_nonzero(d) <= 1e-5 * d.size
    assert (np.abs(d) <= 1).all()


def test_chain_float_channel_into_decode_count():
    torch = _torch()
    t = load_table("648x324")
    n, k, batch, iters = t.n, t.k_info, 64, 10
    sigma = channel.sigma_from_ebn0(2.0, k / n)
    # the oracle's MS is OMS with offset 0
    hard_ref, _, _ = O.decode_f32(t, channel.awgn_f32_host(n, batch, SEED, sigma), iters, O.OMS, 0.0)
    wrong = hard_ref[:, :k] != 0
    assert wrong.any()                         # the point leaves errors to count
    dec = decoder("648x324")
    y = torch.empty((batch, n), dtype=torch.float32, device="cuda")
    hard = torch.empty((batch, n), dtype=torch.uint8, device="cuda")
    counts = torch.zeros(2, dtype=torch.int64, device="cuda")
    dec.awgn_f32_device(y, 0, SEED, sigma)
    dec.decode_count_device(y, hard, iters, k, counts, params=default_params(algo=ALGO_MS, beta=0.0))
    torch.cuda.synchronize()
    assert np.array_equal(hard.cpu().numpy(), hard_ref)
    assert counts.tolist() == [int(wrong.sum()), int(wrong.any(axis=1).sum())]
