"""ldpc_sim -gencoder: the simulator's chain through the general encoder
(ldpc_encoder_create / ldpc_encode / ldpc_encode_async), which takes any
code.  With -fresh the whole chain runs on the device and is deterministic in
the seed, so its counters are checked exactly against the same chain on the
CPU."""
import numpy as np
import pytest

from ldpcgputegra_amd import Code, Decoder, channel, default_params
from test_sim_driver import points, run

pytestmark = pytest.mark.gpu


def cpu_chain_counts(name, seed, ebn0, iters, batch):
    """(bit errors, frame errors) over the first K positions of codewords
    0 .. batch-1: info_bits_host -> Encoder.encode -> awgn_i8_host -> host
    decoder (bit-exact with the kernels) -> count."""
    code = Code(name)
    n, k = code.n, code.k_info
    enc = code.encoder()
    info = channel.info_bits_host(k, batch, seed, first_cw=0)
    cw = enc.encode(info)
    table = channel.i8_table(channel.sigma_from_ebn0(ebn0, k / n))
    llr = channel.awgn_i8_host(n, batch, seed, table, first_cw=0, codeword=cw)
    dec = Decoder(code, device=-1, max_batch=batch)
    hard = dec.decode_i8(llr, iters, default_params())
    dec.close()
    wrong = hard[:, :k] != cw[:, :k]
    return int(wrong.sum()), int(wrong.any(axis=1).sum())


def test_sim_gencoder_fresh_exact_counters():
    r = run(["-code", "648x324", "-gencoder", "-fresh", "-seed", "7", "-min", "2", "-max", "2", "-iter", "20",
             "-batch", "1024", "-frames", "1024", "-fer", "1000000000"])
    assert r.returncode == 0, r.stderr
    (p,) = points(r.stdout)
    be, fe = cpu_chain_counts("648x324", seed=7, ebn0=2.0, iters=20, batch=1024)
    assert fe > 0                                       # 2 dB is inside the waterfall: the counters are exercised
    assert p["frames"] == 1024
    assert (p["bit_errors"], p["frame_errors"]) == (be, fe)


def test_sim_gencoder_non_systematic_code():
    r = run(["-code", "200x100", "-gencoder", "-min", "3", "-max", "3", "-iter", "10", "-batch", "256", "-frames", "256",
             "-fer", "1000000000"])
    assert r.returncode == 0, r.stderr
    (p,) = points(r.stdout)
    assert p["frames"] == 256 and 0 <= p["frame_errors"] <= 256


def test_sim_gencoder_and_encoder_exclude_each_other():
    r = run(["-code", "648x324", "-min", "2", "-max", "2", "-gencoder", "-encoder"])
    assert r.returncode == 2
    assert "usage" in r.stderr and "-gencoder" in r.stderr and "-encoder" in r.stderr
