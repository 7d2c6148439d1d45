"""ldpc_encode_async (csrc/genc.hip) against the host encoder, byte for byte,
at the shapes where the GF(2) product kernel can go wrong -- K below two
words, K not a multiple of 64, rank below / not a multiple of the 256-column
tile, batches that are no multiple of the 16-codeword tile, K spanning several
16-word chunks, scattered and forced positions -- its buffer hygiene, the
delegation to the IRA kernel, and what the encoder is for: the short-code
decode kernels on random codewords, pinned to the oracle."""
import functools

import numpy as np
import pytest

import oracle as O
from ldpcgputegra_amd import ALGO_NMS, ALGO_OMS, Code, Decoder, LdpcError, channel, default_params, load_table

pytestmark = pytest.mark.gpu

#                         what the shape exercises
SHAPES = ["200x100",    # K = 100 < two words; rank 100 < one tile; scattered positions
          "648x324",    # K = 324 = 5 * 64 + 4; rank 324 = 256 + 68
          "816x408",    # one parity position inside the information range
          "2048x384",   # rank 325 < M: 59 forced zeros; K = 1664 = 26 words, two chunks
          "9972x4986"]  # K = 4986 = 77 * 64 + 58: five chunks, tail word; rank = 19 tiles + 122
BATCHES = (1, 3, 16, 17, 67)
FLOAT_TOL = 1e-6


def _torch():
    import torch
    assert torch.cuda.is_available()
    return torch


@functools.lru_cache(maxsize=None)
def encoder(name):
    return Code(name).encoder()


@functools.lru_cache(maxsize=None)
def decoder(name):
    """One context per code with its encoder attached (shared, read only)."""
    enc = encoder(name)
    dec = Decoder(enc.code, max_batch=64)
    dec.set_encoder(enc)
    return dec


def encode_device(torch, dec, info, fill=0xAA, pad=4096):
    """Codewords of info through the device encoder; the output buffer is
    pre-filled and a canary of `pad` bytes behind it must stay as it was."""
    B, n = info.shape[0], dec.code.n
    buf = torch.full((B * n + pad,), fill, dtype=torch.uint8, device="cuda")
    dec.encode_any_device(torch.from_numpy(info).cuda(), buf[:B * n].view(B, n))
    torch.cuda.synchronize()
    out = buf.cpu().numpy()
    assert (out[B * n:] == fill).all(), "canary"
    return out[:B * n].reshape(B, n)


@pytest.mark.parametrize("name", SHAPES)
def test_device_equals_host(name):
    torch = _torch()
    enc, dec = encoder(name), decoder(name)
    rng = np.random.default_rng(31)
    for batch in BATCHES:
        info = rng.integers(0, 2, size=(batch, enc.k), dtype=np.uint8)
        got = encode_device(torch, dec, info)
        assert got.max() <= 1, batch                          # every 0xAA byte was overwritten
        assert np.array_equal(got, enc.encode(info)), batch


@pytest.mark.parametrize("name", ["648x324", "2048x384"])
def test_input_bytes_are_taken_and_1(name):
    torch = _torch()
    enc, dec = encoder(name), decoder(name)
    rng = np.random.default_rng(32)
    bits = rng.integers(0, 2, size=(17, enc.k), dtype=np.uint8)
    info = np.where(bits == 1, np.uint8(0xFF), np.uint8(0x02))
    got = encode_device(torch, dec, info)
    assert np.array_equal(got, enc.encode(bits))
    assert np.array_equal(got[:, enc.info_pos], bits)


@pytest.mark.parametrize("name", ["648x324", "200x100"])
def test_result_independent_of_batch_and_position(name):
    torch = _torch()
    enc, dec = encoder(name), decoder(name)
    info = np.random.default_rng(33).integers(0, 2, size=(35, enc.k), dtype=np.uint8)
    whole = encode_device(torch, dec, info)
    for b in (0, 15, 16, 34):
        assert np.array_equal(encode_device(torch, dec, info[b:b + 1]), whole[b:b + 1]), b
    assert np.array_equal(encode_device(torch, dec, info[::-1].copy()), whole[::-1])
    assert np.array_equal(encode_device(torch, dec, info[3:20].copy()), whole[3:20])


@pytest.mark.parametrize("offset", [0, 1, 8])
def test_unaligned_buffers(offset):
    torch = _torch()
    enc, dec = encoder("648x324"), decoder("648x324")
    B, n, k = 5, enc.n, enc.k
    info = np.random.default_rng(34).integers(0, 2, size=(B, k), dtype=np.uint8)
    d_in = torch.zeros((offset + B * k,), dtype=torch.uint8, device="cuda")
    d_in[offset:] = torch.from_numpy(info.ravel()).cuda()
    buf = torch.full((offset + B * n + 4096,), 0xAA, dtype=torch.uint8, device="cuda")
    dec.encode_any_device(d_in[offset:].view(B, k), buf[offset:offset + B * n].view(B, n))
    torch.cuda.synchronize()
    out = buf.cpu().numpy()
    assert np.array_equal(out[offset:offset + B * n].reshape(B, n), enc.encode(info))
    assert (out[:offset] == 0xAA).all() and (out[offset + B * n:] == 0xAA).all()


def test_batch_zero_overlap_and_missing_encoder():
    torch = _torch()
    enc, dec = encoder("648x324"), decoder("648x324")
    dec.encode_any_device(torch.empty((0, enc.k), dtype=torch.uint8, device="cuda"),
                          torch.empty((0, enc.n), dtype=torch.uint8, device="cuda"))
    buf = torch.zeros((2 * enc.n,), dtype=torch.uint8, device="cuda")
    with pytest.raises(LdpcError) as ei:
        dec.encode_any_device(buf[:enc.k].view(1, -1), buf[16:16 + enc.n].view(1, -1))
    assert ei.value.status == -1 and "overlap" in str(ei.value)
    bare = Decoder(enc.code, max_batch=8)
    with pytest.raises(LdpcError) as ei:
        bare.encode_any_device(buf[:enc.k].view(1, -1), buf[enc.n:].view(1, -1))
    assert ei.value.status == -1 and "no encoder attached" in str(ei.value)
    with pytest.raises(LdpcError) as ei:
        bare.set_encoder(encoder("200x100"))
    assert ei.value.status == -1 and "another code" in str(ei.value)
    torch.cuda.synchronize()
    bare.close()


def test_replacing_the_encoder():
    """A second ldpc_ctx_set_encoder replaces the first upload."""
    torch = _torch()
    enc = encoder("816x408")
    dec = Decoder(enc.code, max_batch=8)
    info = np.random.default_rng(35).integers(0, 2, size=(3, enc.k), dtype=np.uint8)
    dec.set_encoder(enc)
    first = encode_device(torch, dec, info)
    dec.set_encoder(Code("816x408").encoder())     # the same code, loaded again
    assert np.array_equal(encode_device(torch, dec, info), first)
    assert np.array_equal(first, enc.encode(info))
    dec.close()


def test_delegation_equals_dvbs2_encode_async():
    torch = _torch()
    code = Code("dvbs2_r1_2")
    dec = Decoder(code, max_batch=8)
    dec.set_encoder(code.encoder())
    info = np.random.default_rng(36).integers(0, 2, size=(5, code.k_info), dtype=np.uint8)
    d_info = torch.from_numpy(info).cuda()
    a = torch.full((5, code.n), 0xAA, dtype=torch.uint8, device="cuda")
    b = torch.full((5, code.n), 0xAA, dtype=torch.uint8, device="cuda")
    dec.encode_any_device(d_info, a)
    dec.encode_device(d_info, b)
    torch.cuda.synchronize()
    dec.close()
    assert np.array_equal(a.cpu().numpy(), b.cpu().numpy())
    assert np.array_equal(a.cpu().numpy(), code.encode(info))


# ---- what the encoder is for: the short-code kernels on random codewords ----

@functools.lru_cache(maxsize=None)
def chain(name):
    """64 random codewords of `name` through the device encoder and the device
    channel at 2.0 dB: (codewords, int8 LLRs), computed once, read only."""
    torch = _torch()
    enc, dec = encoder(name), decoder(name)
    B = 64
    table = channel.i8_table(channel.sigma_from_ebn0(2.0, enc.k / enc.n))
    d_info = torch.empty((B, enc.k), dtype=torch.uint8, device="cuda")
    d_cw = torch.empty((B, enc.n), dtype=torch.uint8, device="cuda")
    d_llr = torch.empty((B, enc.n), dtype=torch.int8, device="cuda")
    dec.info_bits_device(d_info, 5, seed=41)
    dec.encode_any_device(d_info, d_cw)
    dec.awgn_i8_device(d_llr, 5, 41, table, codeword=d_cw)
    torch.cuda.synchronize()
    cw, llr = d_cw.cpu().numpy(), d_llr.cpu().numpy()
    info = channel.info_bits_host(enc.k, B, 41, first_cw=5)
    assert np.array_equal(cw, enc.encode(info))
    assert np.array_equal(llr, channel.awgn_i8_host(enc.n, B, 41, table, first_cw=5, codeword=cw))
    assert 0.3 < cw.mean() < 0.7                               # not the all-zero codeword
    llr.setflags(write=False)
    return cw, llr


@pytest.mark.parametrize("kernel", [1, 7])
@pytest.mark.parametrize("algo,param", [(ALGO_OMS, 1), (ALGO_NMS, 29)])
@pytest.mark.parametrize("name", ["648x324", "576x288"])
def test_int8_kernels_on_random_codewords(name, algo, param, kernel):
    torch = _torch()
    _, llr = chain(name)
    t = load_table(name)
    ref_hard, ref_soft, _ = O.decode_i8(t, llr, 10, O.NMS if algo == ALGO_NMS else O.OMS, param, return_soft=True)
    dec = Decoder(encoder(name).code, max_batch=64, kernel=kernel)
    d_hard = torch.empty(llr.shape, dtype=torch.uint8, device="cuda")
    d_soft = torch.empty(llr.shape, dtype=torch.int8, device="cuda")
    dec.decode_i8_device(torch.from_numpy(llr.copy()).cuda(), d_hard, 10,
                         params=default_params(algo=algo, offset=param, factor=param), soft=d_soft)
    torch.cuda.synchronize()
    assert dec.last_kernel == {1: "generic", 7: "lds"}[kernel]
    dec.close()
    assert np.array_equal(d_soft.cpu().numpy(), ref_soft)
    assert np.array_equal(d_hard.cpu().numpy(), ref_hard)


@pytest.mark.parametrize("kernel", [9, 7])
@pytest.mark.parametrize("algo,beta", [(ALGO_OMS, 1.0), (ALGO_NMS, 29 / 32)])
@pytest.mark.parametrize("name", ["648x324", "576x288"])
def test_float_kernels_on_random_codewords(name, algo, beta, kernel):
    """The same LLRs as floats; OMS 1 and NMS 29 / 32 are the float forms of
    the int8 offset 1 and factor 29 (scaled by 1 / 32)."""
    torch = _torch()
    _, llr_i8 = chain(name)
    llr = llr_i8.astype(np.float32)
    t = load_table(name)
    ref_hard, ref_soft, _ = O.decode_f32(t, llr, 10, O.NMS if algo == ALGO_NMS else O.OMS, beta)
    dec = Decoder(encoder(name).code, max_batch=64, kernel=kernel)
    d_hard = torch.empty(llr.shape, dtype=torch.uint8, device="cuda")
    d_soft = torch.empty(llr.shape, dtype=torch.float32, device="cuda")
    dec.decode_f32_device(torch.from_numpy(llr).cuda(), d_hard, 10, params=default_params(algo=algo, beta=beta),
                          soft=d_soft)
    torch.cuda.synchronize()
    assert dec.last_kernel == {9: "ldsep", 7: "lds"}[kernel]
    dec.close()
    assert np.max(np.abs(d_soft.cpu().numpy() - ref_soft)) <= FLOAT_TOL
    assert np.array_equal(d_hard.cpu().numpy(), ref_hard)
