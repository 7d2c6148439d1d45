"""The bit source and the encoder entry points, as far as they go without a
GPU: ldpc_info_bits_host against a numpy restatement of its formula, the
device entry points on a host context, and the CPU half of the chain test of
test_gpu_encoder.py (bits -> encode -> AWGN -> decode)."""
import functools

import numpy as np

from ldpcgputegra_amd import Code, Decoder, _lib, channel

M64 = (1 << 64) - 1


def splitmix64(x):
    x = (x + np.uint64(0x9E3779B97F4A7C15))
    x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def info_bits_numpy(k, batch, seed, first_cw):
    key = np.uint64((seed * 0xA0761D6478BD642F) & M64)
    with np.errstate(over="ignore"):
        cw = np.array([(first_cw + b) & M64 for b in range(batch)], dtype=np.uint64)[:, None]
        idx = cw * np.uint64(k) + np.arange(k, dtype=np.uint64)[None, :]
        return (splitmix64(idx ^ key) >> np.uint64(63)).astype(np.uint8)


def chain_inputs():
    """The chain test's inputs (shared with test_gpu_encoder.py): dvbs2_r1_2,
    16 codewords, Eb/N0 2.0 dB, seed 11."""
    code = Code("dvbs2_r1_2")
    table = channel.i8_table(channel.sigma_from_ebn0(2.0, code.k_info / code.n))
    return code, table, dict(batch=16, seed=11, first_cw=3, iters=50)


@functools.lru_cache(maxsize=None)
def cpu_chain():
    """(info, codeword, hard) of the chain on the CPU: info_bits_host ->
    Code.encode -> awgn_i8_host -> host-context decode (50 iterations, OMS 1).
    Computed once; the callers only read it."""
    code, table, c = chain_inputs()
    info = channel.info_bits_host(code.k_info, c["batch"], c["seed"], first_cw=c["first_cw"])
    cw = code.encode(info)
    llr = channel.awgn_i8_host(code.n, c["batch"], c["seed"], table, first_cw=c["first_cw"], codeword=cw)
    dec = Decoder(code, device=-1, max_batch=c["batch"])
    hard = dec.decode_i8(llr, c["iters"], _lib.default_params(algo=_lib.ALGO_OMS, offset=1))
    dec.close()
    return info, cw, hard


def test_info_bits_host_matches_formula():
    first = 2**33 + 5
    got = channel.info_bits_host(360, 3, seed=7, first_cw=first)
    assert got.shape == (3, 360) and got.dtype == np.uint8
    assert np.array_equal(got, info_bits_numpy(360, 3, 7, first))
    assert set(np.unique(got)) <= {0, 1}


def test_info_bits_indexed_per_codeword():
    whole = channel.info_bits_host(360, 7, seed=9, first_cw=0)
    part = channel.info_bits_host(360, 2, seed=9, first_cw=5)
    assert np.array_equal(whole[5:7], part)
    assert not np.array_equal(whole[5:7], channel.info_bits_host(360, 2, seed=10, first_cw=5))


def test_info_bits_mean():
    bits = channel.info_bits_host(64800, 4, seed=1)
    assert 0.49 < bits.mean() < 0.51


def test_info_bits_host_arguments():
    L = _lib.lib()
    buf = np.zeros(8, dtype=np.uint8)
    assert L.ldpc_info_bits_host(0, 1, 0, 0, buf.ctypes.data) == _lib.LDPC_EINVAL
    assert L.ldpc_info_bits_host(8, -1, 0, 0, buf.ctypes.data) == _lib.LDPC_EINVAL
    assert L.ldpc_info_bits_host(8, 1, 0, 0, None) == _lib.LDPC_EINVAL
    assert L.ldpc_info_bits_host(8, 0, 0, 0, None) == _lib.LDPC_OK


def test_async_entry_points_reject_host_context():
    L = _lib.lib()
    dec = Decoder(Code("dvbs2_r1_2"), device=-1, max_batch=4)
    a = np.zeros(16, dtype=np.uint8)   # never dereferenced: the context is checked first
    b = np.zeros(16, dtype=np.uint8)
    assert L.ldpc_info_bits_async(dec._ctx, None, a.ctypes.data, 1, 0, 1) == _lib.LDPC_EUNSUPPORTED
    assert b"host context" in L.ldpc_last_error()
    assert L.ldpc_dvbs2_encode_async(dec._ctx, None, a.ctypes.data, b.ctypes.data, 1) == _lib.LDPC_EUNSUPPORTED
    assert b"host context" in L.ldpc_last_error()
    table = channel.i8_table(0.8)
    assert L.ldpc_awgn_i8_async(dec._ctx, None, a.ctypes.data, 1, 0, 1, table.ctypes.data,
                                b.ctypes.data) == _lib.LDPC_EUNSUPPORTED
    # argument checks come first
    assert L.ldpc_info_bits_async(None, None, a.ctypes.data, 1, 0, 1) == _lib.LDPC_EINVAL
    assert L.ldpc_info_bits_async(dec._ctx, None, None, 1, 0, 1) == _lib.LDPC_EINVAL
    assert L.ldpc_info_bits_async(dec._ctx, None, a.ctypes.data, -1, 0, 1) == _lib.LDPC_EINVAL
    assert L.ldpc_dvbs2_encode_async(None, None, a.ctypes.data, b.ctypes.data, 1) == _lib.LDPC_EINVAL
    assert L.ldpc_dvbs2_encode_async(dec._ctx, None, None, b.ctypes.data, 1) == _lib.LDPC_EINVAL
    assert L.ldpc_dvbs2_encode_async(dec._ctx, None, a.ctypes.data, None, 1) == _lib.LDPC_EINVAL
    assert L.ldpc_dvbs2_encode_async(dec._ctx, None, a.ctypes.data, b.ctypes.data, -1) == _lib.LDPC_EINVAL
    dec.close()


def test_cpu_chain_decodes_without_errors():
    info, cw, hard = cpu_chain()
    k = info.shape[1]
    assert np.array_equal(cw[:, :k], info)
    assert int((hard[:, :k] != info).sum()) == 0
