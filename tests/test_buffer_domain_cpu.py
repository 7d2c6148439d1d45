"""What test_gpu_buffer_domain.py takes for granted, shown without a GPU, and
the host (device -1) context under the same buffer contract:

* the oracle decodes every codeword on its own, so the first B codewords of
  its 65-codeword result are its result for the first B codewords -- int8 and
  float, with and without early termination;
* the early-termination inputs (param_domain.ET_EDGE, float_domain.EDGE_EBN0)
  put stopped and still-running codewords among the first 17 and make
  codeword 64, alone in its group at batch 65, stop for one code and run on
  for the other;
* the numpy restatement of the quantiser's rule agrees with oracle.quantize;
* host-context decodes at the batch edges and around the 32-codeword AVX2
  block, from numpy views at byte offset 1 (int8) and 4 (float) into a
  canary-guarded hard array at offset 1 (host.cpp copies the LLRs into its own
  64-byte aligned V / msg blocks: host_simd.h's aligned loads and stores touch
  only those and the aligned `live` array, never a caller's buffer);
* buffer_domain.EXPECTED_PATH names every case the GPU file generates."""
import numpy as np
import pytest

import buffer_domain as BD
import float_domain as FD
import oracle as O
import param_domain as PD
from ldpcgputegra_amd import ALGO_MS, Code, Decoder, default_params, load_table

HOST_BATCHES = BD.BATCHES + (31, 32, 33)     # 32: codewords per AVX2 block of the host decoder


def same(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


@pytest.mark.parametrize("code", ["648x324", "dvbs2_r1_2"])
def test_oracle_int8_prefix_independence(code):
    t = load_table(code)
    x, full = BD.i8_input(code), BD.i8_oracle(code)
    assert np.array_equal(x[:17], PD.make_input("ext", 17, t.n))
    for B in BD.BATCHES:
        part = O.decode_i8(t, x[:B], BD.ITERS, return_soft=True, threads=O.host_threads())
        assert same(part, BD.prefix(full, B)), B


@pytest.mark.parametrize("code", ["dvbs2_r1_2", "dvbs2_r8_9"])
def test_oracle_int8_prefix_independence_early_termination(code):
    t = load_table(code)
    x, full = BD.et_input(code), BD.et_oracle(code)
    assert np.array_equal(x[:17], PD.et_input(code, 17, PD.ET_EDGE[code]))
    for B in (1, 17, 65):
        part = O.decode_i8(t, x[:B], BD.ET_ITERS, early_term=True, return_soft=True, threads=O.host_threads())
        assert same(part, BD.prefix(full, B)), B


@pytest.mark.parametrize("code,early", [("648x324", False), ("648x324", True), ("dvbs2_r1_2", False),
                                        ("dvbs2_r8_9", True)])
def test_oracle_float_prefix_independence(code, early):
    t = load_table(code)
    ebn0 = FD.EDGE_EBN0.get(code) if early else None
    iters = BD.ET_ITERS if early else BD.ITERS
    x, full = BD.f32_input(code, ebn0), BD.f32_oracle(code, iters, early, ebn0)
    assert np.array_equal(x[:17], FD.grid_input(code, 17, FD.EBN0[code] if ebn0 is None else ebn0, *FD.FINE))
    assert not np.signbit(x[x == 0]).any()      # no -0.0: ldsep equals the oracle bit for bit on this input
    for B in (1, 17, 65) if early else BD.BATCHES:
        part = O.decode_f32(t, x[:B], iters, O.OMS, 0.0, early_term=early, threads=O.host_threads())
        assert same(part, BD.prefix(full, B)), B


def test_early_termination_inputs_sit_on_the_edges():
    """Iterations used by codewords 0 .. 16 and by codeword 64 of the two
    codes, on the oracle alone."""
    its = {c: BD.et_oracle(c)[2] for c in ("dvbs2_r1_2", "dvbs2_r8_9")}
    fts = {c: BD.f32_oracle(c, BD.ET_ITERS, True, FD.EDGE_EBN0[c])[2] for c in ("dvbs2_r1_2", "dvbs2_r8_9")}
    for what, d in (("int8", its), ("float", fts)):
        for c, v in d.items():
            print("%s %s: codewords 0 .. 16 %s, codeword 64 %d" % (what, c, v[:17].tolist(), v[64]))
        cond = BD.et_edge_conditions(d["dvbs2_r1_2"], d["dvbs2_r8_9"])
        assert all(cond.values()), (what, cond)
    # the 648x324 float step of the call sequences: 3 codewords, not all stopping together
    short = BD.f32_oracle("648x324", BD.ET_ITERS, True)[2][:3]
    assert short.min() < short.max()


@pytest.mark.parametrize("factor,sat_neg,sat_pos", BD.QUANT_SETS)
def test_quantiser_restatement_vs_oracle(factor, sat_neg, sat_pos):
    s = BD.quantize_specials(factor)
    assert np.isnan(s[:2]).all() and np.signbit(s[1]) and not np.signbit(s[0])
    edge = np.float32(2147483648.0 / factor)
    assert {float(edge), float(-edge)} <= set(s[8:].tolist()) and float(edge) * factor == 2.0 ** 31
    exp = BD.quantize_rule(s, factor, sat_neg, sat_pos)
    # NaN, +-2^31 and beyond: sat_neg; just inside: the saturation of its sign; zeros and subnormals: 0 clamped
    assert exp.tolist() == [sat_neg, sat_neg, sat_neg, sat_neg] + [min(max(0, sat_neg), sat_pos)] * 4 + \
        [sat_pos, sat_neg, sat_neg, sat_neg, sat_neg, sat_neg]
    assert np.array_equal(O.quantize(s, factor, sat_neg, sat_pos), exp)
    y = BD.quantize_input(2 ** 16, factor)
    exp = BD.quantize_rule(y, factor, sat_neg, sat_pos)
    assert np.array_equal(O.quantize(y, factor, sat_neg, sat_pos), exp)
    assert exp.min() == sat_neg and exp.max() == sat_pos and len(np.unique(exp)) >= min(sat_pos - sat_neg, 40)
    host = Decoder(Code("576x288"), device=-1, max_batch=1)
    assert np.array_equal(host.quantize(y, factor, sat_neg, sat_pos), exp)
    host.close()


@pytest.mark.parametrize("code", ["576x288", "dvbs2_r1_2"])
def test_host_context_int8_at_the_batch_edges(code):
    t = load_table(code)
    x, exp = BD.i8_input(code), BD.i8_oracle(code)
    dec = Decoder(Code(code), device=-1, max_batch=BD.MAX_BATCH)
    for B in HOST_BATCHES:
        llr, c0 = BD.carve_host((B, t.n), np.int8, 1, BD.PAD_BYTE, "llr")
        llr[...] = x[:B]
        hard, c1 = BD.carve_host((B, t.n), np.uint8, 1, 9, "hard")
        assert llr.ctypes.data % 2 == 1 and hard.ctypes.data % 2 == 1
        out = dec.decode_i8(llr, BD.ITERS, params=PD.CONTROL.product(), out=hard)
        assert out is hard and dec.last_kernel == "host"
        assert np.array_equal(hard, exp[0][:B]), B
        c0()
        c1()
    dec.close()


def test_host_context_float_at_the_batch_edges():
    code = "648x324"
    t = load_table(code)
    x, exp = BD.f32_input(code), BD.f32_oracle(code)
    dec = Decoder(Code(code), device=-1, max_batch=BD.MAX_BATCH)
    for B in HOST_BATCHES:
        llr, c0 = BD.carve_host((B, t.n), np.float32, 4, BD.PAD_BYTE, "llr")
        llr[...] = x[:B]
        hard, c1 = BD.carve_host((B, t.n), np.uint8, 1, 9, "hard")
        assert llr.ctypes.data % 16 == 4
        dec.decode_f32(llr, BD.ITERS, params=default_params(algo=ALGO_MS, beta=0.0), out=hard)
        assert np.array_equal(hard, exp[0][:B]), B
        c0()
        c1()
    dec.close()


def test_canaries_catch_a_stray_write():
    view, check = BD.carve_host((3, 10), np.uint8, 1, 9)
    check()
    view[...] = 1
    check()
    flat = view.reshape(-1)
    np.lib.stride_tricks.as_strided(flat, shape=(31,), strides=(1,))[30] = 1      # one byte past the payload
    with pytest.raises(AssertionError, match="0 bytes past the end"):
        check()


def test_expected_path_names_every_gpu_case():
    import test_gpu_buffer_domain as G
    assert set(G.ALIGN_IDS) <= set(BD.EXPECTED_PATH)
    assert all(BD.pytest_id(c).startswith(BD.case_id(c) + "=") for c in BD.ALIGN_CASES)
    others = (["mixed-llr%d-out%d.%d" % o for o in BD.MIXED_OFFSETS] +
              [BD.count_id(c, h, r) for c in BD.COUNT_CODES for h in BD.COUNT_OFFSETS for r in BD.COUNT_OFFSETS + (None,)] +
              ["decode_count-648x324-f32-k9", "decode_count-648x324-f32-k7", "decode_count-576x288-i8-k7",
               "awgn-576x288-out1", "quantize-576x288-in4-out1", "info_bits-576x288-out0", "info_bits-576x288-out1",
               "info_bits-9972x4986-out0"])
    assert set(others) <= set(BD.EXPECTED_PATH)
    assert set(BD.EXPECTED_PATH) == set(G.ALIGN_IDS) | set(others)      # and nothing names a case that does not exist
    # the one path no aligned pointer reaches is pinned by an unaligned case of each coop3 code
    assert sum(p.startswith("interleave_grp_k ") for p in BD.EXPECTED_PATH.values()) == 6
    # the shapes the table was written for
    assert load_table("576x288").n % 16 == 0 and load_table("648x324").n % 16 == 8
    assert (4 * load_table("648x324").n) % 16 == 0 and (4 * load_table("200x100").n) % 16 == 0
    assert load_table("dvbs2_r1_2").k_info == BD.COUNT_CODES["dvbs2_r1_2"] == 16 * 2025
    assert BD.COUNT_CODES["576x288"] % 16 == 12 and BD.COUNT_CODES["9972x4986"] % 4 == 2
