"""The head of the chain on the GPU: ldpc_info_bits_async and
ldpc_dvbs2_encode_async (csrc/encode.hip) against their host twins, byte for
byte -- every shipped Annex-B table, small tables at the shapes where the
quasi-cyclic kernel can go wrong (q = 1, odd q, rows of different length, the
360-of-384 partial wave, odd batches), non-0/1 input, a canary behind the
output -- and the whole device chain bits -> encode -> AWGN -> decode -> count
against the CPU chain of test_encoder_host.py."""
import numpy as np
import pytest

from ldpcgputegra_amd import Code, Decoder, LdpcError, _lib, channel
from test_encoder_host import chain_inputs, cpu_chain

pytestmark = pytest.mark.gpu

ANNEX_B = ["dvbs2_r1_2", "dvbs2_r2_3", "dvbs2_r8_9", "dvbs2_r9_10", "dvbs2shape_r3_4", "dvbs2shape_r5_6"]
# (q, addresses per residue for each row): every check gets the same information degree
SMALL = {"q1": (1, [1]), "q3": (3, [2]), "q2": (2, [1, 2, 1]), "q7": (7, [3, 1])}
SMALL_N = {"q1": 720, "q3": 1440, "q2": 1800, "q7": 3240}


def _torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def write_small_table(path, q, c, seed):
    """Annex-B style table: row g holds, for each residue s < q, c[g] distinct
    t of 0..359 as the addresses q t + s."""
    rng = np.random.default_rng(seed)
    k, m = 360 * len(c), 360 * q
    lines = ["# N=%d K=%d" % (k + m, k)]
    for cg in c:
        row = [q * int(t) + s for s in range(q) for t in rng.choice(360, size=cg, replace=False)]
        lines.append(" ".join(str(x) for x in rng.permutation(row)))
    path.write_text("\n".join(lines) + "\n")
    return k + m


def encode_device(torch, dec, info):
    d_info = torch.from_numpy(info).cuda()
    d_cw = torch.empty((info.shape[0], dec.code.n), dtype=torch.uint8, device="cuda")
    dec.encode_device(d_info, d_cw)
    torch.cuda.synchronize()
    return d_cw.cpu().numpy()


@pytest.mark.parametrize("name", ANNEX_B)
def test_shipped_tables_equal_host_encoder(name):
    torch = _torch()
    code = Code(name)
    info = np.random.default_rng(5).integers(0, 2, size=(5, code.k_info), dtype=np.uint8)
    dec = Decoder(code, max_batch=8)
    got = encode_device(torch, dec, info)
    dec.close()
    assert np.array_equal(got, code.encode(info))


@pytest.mark.parametrize("key", sorted(SMALL))
def test_small_tables_equal_host_encoder(key, tmp_path):
    torch = _torch()
    q, c = SMALL[key]
    n = write_small_table(tmp_path / (key + ".txt"), q, c, seed=17)
    assert n == SMALL_N[key]
    code = Code(str(tmp_path / (key + ".txt")))
    assert (code.n, code.m) == (n, 360 * q)
    dec = Decoder(code, max_batch=8)     # the encoder takes any batch: it has no per-batch scratch
    rng = np.random.default_rng(23)
    for batch in (1, 3, 64, 67):
        info = rng.integers(0, 2, size=(batch, code.k_info), dtype=np.uint8)
        assert np.array_equal(encode_device(torch, dec, info), code.encode(info)), batch
    dec.close()


def test_result_independent_of_batch_and_position():
    torch = _torch()
    code = Code("dvbs2_r8_9")
    info = np.random.default_rng(6).integers(0, 2, size=(6, code.k_info), dtype=np.uint8)
    dec = Decoder(code, max_batch=8)
    whole = encode_device(torch, dec, info)
    for b in (0, 5):
        assert np.array_equal(encode_device(torch, dec, info[b:b + 1]), whole[b:b + 1])
    assert np.array_equal(encode_device(torch, dec, info[::-1].copy()), whole[::-1])
    dec.close()


def test_input_bytes_are_taken_and_1():
    torch = _torch()
    code = Code("dvbs2_r9_10")
    info = np.random.default_rng(7).integers(0, 256, size=(3, code.k_info), dtype=np.uint8)
    dec = Decoder(code, max_batch=8)
    got = encode_device(torch, dec, info)
    dec.close()
    assert np.array_equal(got, code.encode(info))
    assert np.array_equal(got[:, :code.k_info], info & 1)


@pytest.mark.parametrize("offset", [0, 8, 3])    # 16-byte, 8-byte and byte stores
def test_systematic_part_and_canary(offset):
    torch = _torch()
    code = Code("dvbs2_r1_2")
    B, n, k = 3, code.n, code.k_info
    info = np.random.default_rng(8).integers(0, 256, size=(B, k), dtype=np.uint8)
    dec = Decoder(code, max_batch=8)
    buf = torch.full((offset + B * n + 4096,), 0xA5, dtype=torch.uint8, device="cuda")
    d_cw = buf[offset:offset + B * n].view(B, n)
    dec.encode_device(torch.from_numpy(info).cuda(), d_cw)
    torch.cuda.synchronize()
    dec.close()
    out = buf.cpu().numpy()
    cw = out[offset:offset + B * n].reshape(B, n)
    assert np.array_equal(cw[:, :k], info & 1)
    assert np.array_equal(cw, code.encode(info))
    assert (out[:offset] == 0xA5).all() and (out[offset + B * n:] == 0xA5).all()


def test_encode_batch_zero_and_overlap():
    torch = _torch()
    code = Code("dvbs2_r1_2")
    dec = Decoder(code, max_batch=8)
    dec.encode_device(torch.empty((0, code.k_info), dtype=torch.uint8, device="cuda"),
                      torch.empty((0, code.n), dtype=torch.uint8, device="cuda"))
    buf = torch.zeros((2 * code.n,), dtype=torch.uint8, device="cuda")
    with pytest.raises(LdpcError) as ei:
        dec.encode_device(buf[:code.k_info].view(1, -1), buf[16:16 + code.n].view(1, -1))
    assert ei.value.status == -1
    torch.cuda.synchronize()
    dec.close()


def test_info_bits_device_equals_host():
    torch = _torch()
    code = Code("dvbs2_r1_2")
    assert code.k_info == 32400
    first = 2**33 + 5
    dec = Decoder(code, max_batch=8)
    buf = torch.full((67 * 32400 + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    dec.info_bits_device(buf[:67 * 32400].view(67, 32400), first, seed=12)
    torch.cuda.synchronize()
    dec.close()
    out = buf.cpu().numpy()
    assert np.array_equal(out[:67 * 32400].reshape(67, 32400), channel.info_bits_host(32400, 67, 12, first_cw=first))
    assert (out[67 * 32400:] == 0xA5).all()


@pytest.mark.parametrize("offset", [0, 1])
def test_info_bits_device_tail_and_unaligned(offset):
    """K = 506: 3 codewords are no multiple of the 8 bytes a lane writes."""
    torch = _torch()
    code = Code("1024x518")
    k = code.k_info
    assert (3 * k) % 8 != 0
    dec = Decoder(code, max_batch=8)
    buf = torch.full((offset + 3 * k + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    dec.info_bits_device(buf[offset:offset + 3 * k].view(3, k), 40, seed=3)
    torch.cuda.synchronize()
    dec.close()
    out = buf.cpu().numpy()
    assert np.array_equal(out[offset:offset + 3 * k].reshape(3, k), channel.info_bits_host(k, 3, 3, first_cw=40))
    assert (out[:offset] == 0xA5).all() and (out[offset + 3 * k:] == 0xA5).all()


def test_encode_unsupported_code():
    torch = _torch()
    code = Code("576x288")
    dec = Decoder(code, max_batch=8)
    info = torch.zeros((1, code.k_info), dtype=torch.uint8, device="cuda")
    cw = torch.zeros((1, code.n), dtype=torch.uint8, device="cuda")
    with pytest.raises(LdpcError) as ei:
        dec.encode_device(info, cw)
    assert ei.value.status == -2
    assert "not built from a DVB-S2 table" in str(ei.value)
    dec.close()


def test_device_chain_equals_cpu_chain():
    torch = _torch()
    code, table, c = chain_inputs()
    info, cw, hard = cpu_chain()
    B, n, k = c["batch"], code.n, code.k_info
    dec = Decoder(code, max_batch=B)
    d_info = torch.empty((B, k), dtype=torch.uint8, device="cuda")
    d_cw = torch.empty((B, n), dtype=torch.uint8, device="cuda")
    d_llr = torch.empty((B, n), dtype=torch.int8, device="cuda")
    d_hard = torch.empty((B, n), dtype=torch.uint8, device="cuda")
    d_cnt = torch.zeros(2, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    s = dec.stream
    dec.info_bits_device(d_info, c["first_cw"], c["seed"], stream=s)
    dec.encode_device(d_info, d_cw, stream=s)
    dec.awgn_i8_device(d_llr, c["first_cw"], c["seed"], table, codeword=d_cw, stream=s)
    dec.decode_i8_device(d_llr, d_hard, c["iters"], params=_lib.default_params(algo=_lib.ALGO_OMS, offset=1), stream=s)
    dec.count_errors_device(d_hard, k, d_cnt, ref=d_cw, stream=s)
    torch.cuda.synchronize()
    dec.close()
    assert np.array_equal(d_info.cpu().numpy(), info)
    assert np.array_equal(d_cw.cpu().numpy(), cw)
    got = d_hard.cpu().numpy()
    assert np.array_equal(got, hard)
    assert d_cnt.cpu().tolist() == [0, 0]
    assert np.array_equal(got[:, :k], info)
