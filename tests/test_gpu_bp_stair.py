"""Layered belief propagation on the float staircase kernel (csrc/stairbp*,
LDPC_KERNEL_STAIRF with ldpc_ctx_set_bp_staircase on) against the host decoder
(device = -1, decode_f32_soft), bit for bit on hard decisions, soft output
(as uint32) and iterations used.  test_bp_stair_cpu.py holds the host decoder
to the definition on a staircase table.

Tables: one per degree from struct_domain with M % 16 == 0 and a hazard that
admits all four group widths, and x5_q1_h57 (M = 360: widths 2, 4, 8, so a
request for 16 falls back).  Batch 37 decodes unrounded true LLRs, batch 5 the
coarse grid with its zeros and every 7th column -0.0; batch 5 is stride 64:
two waves at S = 2, the second all padding and no XCD remap, 16 waves with the
remap at S = 16.  3 iterations cross the tail -> check 0 wrap twice, and
G = M / S is odd (135) at S = 16 for M = 2160."""
import numpy as np
import pytest

import bp_ref as R
import float_domain as FD
import struct_domain as ST
from ldpcgputegra_amd import ALGO_BP, ALGO_MS, Code, Decoder, LdpcError, _lib, channel, default_params, load_table
from test_bp_cpu import ET_ITERS, awgn_llr, host
from test_gpu_bp import assert_same, bp, run

pytestmark = pytest.mark.gpu

ALL4 = ["x5_q6_h144", "x8_q4_h160", "x12_q4_h160", "x20_q4_h96", "x25_q6_h96", "x28_q6_h96"]
FALLBACK = "x5_q1_h57"
WIDTHS = (2, 4, 8, 16)
_decs = {}
_refs = {}


def _torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def struct_dec(name, device=0):
    key = (name, device)
    if key not in _decs:
        _decs[key] = Decoder(Code(ST.table(name)), device=device, max_batch=64, bp_staircase=device >= 0)
    return _decs[key]


def struct_llr(name, batch):
    """Batch 37: unrounded true LLRs of the all-zero codeword at 2.0 dB; batch
    5: the first N columns of dvbs2_r1_2's coarse grid (zeros +0.0), every 7th
    column -0.0."""
    t = ST.table(name)
    if batch == 37:
        sigma = channel.sigma_from_ebn0(2.0, t.k_info / t.n)
        return channel.awgn_f32_host(t.n, batch, seed=R.INPUT_SEED, sigma=sigma, normalize=True)
    x = np.array(FD.grid("dvbs2_r1_2", batch, "coarse")[:, :t.n])
    x[:, ::7] = -0.0
    return x


def struct_ref(name, batch, iters):
    key = (name, batch, iters)
    if key not in _refs:
        llr = struct_llr(name, batch)
        out = struct_dec(name, -1).decode_f32_soft(llr, iters, bp())
        llr.setflags(write=False)
        for a in out:
            a.setflags(write=False)
        _refs[key] = (llr, out)
    return _refs[key]


def real_ref(name, iters, early=False):
    key = (name, iters, early)
    if key not in _refs:
        llr = awgn_llr(name, 5)        # float_domain.EBN0
        _refs[key] = (llr, host(name).decode_f32_soft(llr, iters, bp(early)))
    return _refs[key]


def real_dec(name):
    if name not in _decs:
        _decs[name] = Decoder(Code(name), max_batch=64, bp_staircase=True)
    return _decs[name]


def test_tables_have_the_widths():
    for name in ALL4:
        assert ST.widths(name) == WIDTHS and ST.table(name).m % 16 == 0 and 3600 <= ST.table(name).n <= 11880
    assert sorted(ST.table(n).groups[0][0] - 2 for n in ALL4) == sorted(ST.XS)
    assert ST.widths(FALLBACK) == (2, 4, 8) and ST.table(FALLBACK).m == 360
    assert ST.table("x5_q6_h144").m // 16 == 135
    g = struct_llr(ALL4[0], 5).view(np.uint32)
    assert (g == 0).any() and (g == 0x80000000).any()


@pytest.mark.parametrize("iters", [1, 3])
@pytest.mark.parametrize("batch", [37, 5])
@pytest.mark.parametrize("S", WIDTHS)
@pytest.mark.parametrize("name", ALL4 + [FALLBACK])
def test_decode_is_the_host_decoders(name, S, batch, iters, monkeypatch):
    monkeypatch.setenv("LDPC_STAIRF_S", str(S))
    llr, exp = struct_ref(name, batch, iters)
    dec = struct_dec(name)
    assert dec.bp_staircase and dec.kernel == 0
    assert_same(run(dec, llr, iters, bp()), exp, "%s S = %d batch %d, %d iterations" % (name, S, batch, iters))
    assert dec.last_kernel == "stairf" and dec.last_skipped is None


@pytest.mark.parametrize("name", FD.DVBS2)
def test_real_codes(name):
    """Every DVB-S2 code, automatic width, kernel AUTO with the switch on."""
    llr, exp = real_ref(name, 2)
    dec = real_dec(name)
    assert_same(run(dec, llr, 2, bp()), exp, name)
    assert dec.last_kernel == "stairf" and dec.last_skipped is None


@pytest.mark.parametrize("S", [2, 16])
def test_early_termination(S, monkeypatch):
    """dvbs2_r1_2 at float_domain.EBN0 (2.0 dB), 16 iterations; iters_used of
    the 5 codewords, from the host decoder: [7 7 8 7 8].  At S = 16 codewords
    0 .. 3 share a wave (one goes on while three are frozen) and codeword 4
    sits with padding."""
    monkeypatch.setenv("LDPC_STAIRF_S", str(S))
    llr, exp = real_ref("dvbs2_r1_2", ET_ITERS, early=True)
    assert len(set(int(u) for u in exp[2] if u < ET_ITERS)) >= 2, exp[2]
    dec = real_dec("dvbs2_r1_2")
    assert_same(run(dec, llr, ET_ITERS, bp(early=True)), exp, "early, S = %d" % S)
    assert dec.last_kernel == "stairf"


# ---- selection -------------------------------------------------------------

def _decode_status(dec, llr, params):
    torch = _torch()
    d_llr = torch.from_numpy(np.array(llr)).cuda()
    d_hard = torch.full(llr.shape, 9, dtype=torch.uint8, device="cuda")
    try:
        dec.decode_f32_device(d_llr, d_hard, 1, params=params)
    except LdpcError as e:
        torch.cuda.synchronize()
        assert (d_hard.cpu().numpy() == 9).all()
        return e.status
    torch.cuda.synchronize()
    return _lib.LDPC_OK


def test_switch_off_is_as_before():
    name = "dvbs2_r1_2"
    llr, exp = real_ref(name, 1)
    dec = Decoder(Code(name), max_batch=64, kernel=11)
    assert dec.bp_staircase is False
    assert _decode_status(dec, llr, bp()) == _lib.LDPC_EUNSUPPORTED and dec.kernel == 11
    dec.set_kernel(0)
    assert_same(run(dec, llr, 1, bp()), exp, "auto, switch off")
    assert dec.last_kernel == "generic" and dec.last_skipped == "stairf"
    # on, then off again
    dec.set_bp_staircase(True)
    assert dec.bp_staircase is True
    dec.set_bp_staircase(False)
    assert dec.bp_staircase is False
    assert_same(run(dec, llr, 1, bp()), exp, "auto, switch off again")
    assert dec.last_kernel == "generic" and dec.last_skipped == "stairf"
    dec.close()


def test_switch_on_selection():
    name = "dvbs2_r1_2"
    llr, exp = real_ref(name, 1)
    dec = Decoder(Code(name), max_batch=64, bp_staircase=True)
    assert dec.bp_staircase is True
    for kernel, family in ((0, "stairf"), (11, "stairf"), (1, "generic")):
        dec.set_kernel(kernel)
        assert_same(run(dec, llr, 1, bp()), exp, "kernel %d, switch on" % kernel)
        assert dec.last_kernel == family and dec.last_skipped is None
    for kernel in (2, 3, 5, 8):       # the int8 families still refuse BP; dvbs2_r1_2 has no family 7
        dec.set_kernel(kernel)
        assert _decode_status(dec, llr, bp()) == _lib.LDPC_EUNSUPPORTED
    dec.close()


def test_a_stride_stairf_cannot_take():
    """stairf addresses V with u32 byte offsets, (N + 1) * stride * 4 < 2^32:
    N = 64800 allows strides up to 16512.  At batch 16640, with the switch on:
    forced 11 is LDPC_EUNSUPPORTED, for BP as for min-sum, and touches nothing;
    the automatic choice decodes BP on generic and last_skipped names stairf.
    With the switch off last_skipped stays None for such a batch, as before.
    Selection is what is checked: the input is all-zero LLRs (every decision 0)
    in buffers of the full batch, one iteration; about 25 GB on the device."""
    torch = _torch()
    B, n = 16640, 64800
    assert (n + 1) * 16512 * 4 < 2 ** 32 <= (n + 1) * B * 4 and B % 64 == 0
    dec = Decoder(Code("dvbs2_r1_2"), max_batch=B, bp_staircase=True, kernel=11)
    d_llr = torch.zeros((B, n), dtype=torch.float32, device="cuda")
    d_hard = torch.empty((B, n), dtype=torch.uint8, device="cuda")
    d_hard[::1024] = 9
    for p in (bp(), default_params(algo=ALGO_MS)):
        with pytest.raises(LdpcError) as e:
            dec.decode_f32_device(d_llr, d_hard, 1, params=p)
        assert e.value.status == _lib.LDPC_EUNSUPPORTED
    torch.cuda.synchronize()
    assert bool((d_hard[::1024] == 9).all()) and dec.kernel == 11
    dec.set_kernel(0)
    for switch, skipped in ((True, "stairf"), (False, None)):
        dec.set_bp_staircase(switch)
        d_hard[::1024] = 9
        dec.decode_f32_device(d_llr, d_hard, 1, params=bp())
        torch.cuda.synchronize()
        assert dec.last_kernel == "generic" and dec.last_skipped == skipped, (switch, dec.last_kernel, dec.last_skipped)
        assert bool((d_hard[::1024] == 0).all())
    dec.close()
    del d_llr, d_hard
    torch.cuda.empty_cache()


def test_set_refused_without_a_table():
    for make in (lambda: Decoder(Code("dvbs2_r1_2"), device=-1, max_batch=4), lambda: Decoder(Code("648x324"), max_batch=4)):
        dec = make()
        with pytest.raises(LdpcError) as e:
            dec.set_bp_staircase(True)
        assert e.value.status == _lib.LDPC_EUNSUPPORTED and dec.bp_staircase is False
        dec.close()


def test_min_sum_after_bp_on_one_context():
    name = "dvbs2_r1_2"
    llr, exp = real_ref(name, 2)
    dec = real_dec(name)
    assert_same(run(dec, llr, 2, bp()), exp, "bp")
    ms = default_params(algo=ALGO_MS)
    hard, soft, its = run(dec, llr, 2, ms)
    assert dec.last_kernel == "stairf" and dec.last_skipped is None
    eh, es, eit = host(name).decode_f32_soft(llr, 2, ms)
    assert_same((hard, soft, its), (eh, es, eit), "min-sum after bp")
    assert not np.array_equal(es.view(np.uint32), exp[1].view(np.uint32))     # it is another algorithm's result
    assert_same(run(dec, llr, 2, bp()), exp, "bp again")


def test_rows_beyond_the_batch_are_untouched():
    name = ALL4[0]
    llr, exp = struct_ref(name, 5, 3)
    hard, soft, its = run(struct_dec(name), llr, 3, bp(), rows=7)
    assert_same((hard[:5], soft[:5], its[:5]), exp, name)
    assert (hard[5:] == 9).all() and (soft[5:] == 99.0).all() and (its[5:] == -7).all()


def test_counting_decode():
    """ldpc_decode_f32_count_async counts what a decode followed by
    ldpc_count_errors_async counts (1 iteration leaves errors)."""
    torch = _torch()
    name = ALL4[0]
    llr, exp = struct_ref(name, 37, 1)
    dec = struct_dec(name)
    n, k = dec.code.n, dec.code.k_info
    d_llr = torch.from_numpy(np.array(llr)).cuda()
    d_hard = torch.zeros((37, n), dtype=torch.uint8, device="cuda")
    d_cnt = torch.zeros(4, dtype=torch.int64, device="cuda")
    dec.decode_count_device(d_llr, d_hard, 1, k, d_cnt[:2], params=bp())
    assert dec.last_kernel == "stairf"
    d_hard2 = torch.zeros_like(d_hard)
    dec.decode_f32_device(d_llr, d_hard2, 1, params=bp())
    dec.count_errors_device(d_hard2, k, d_cnt[2:])
    torch.cuda.synchronize()
    cnt = d_cnt.cpu().numpy()
    assert np.array_equal(d_hard.cpu().numpy(), exp[0]) and np.array_equal(d_hard2.cpu().numpy(), exp[0])
    assert cnt[0] == cnt[2] == int(exp[0][:, :k].sum()) and cnt[1] == cnt[3] == int(exp[0][:, :k].any(axis=1).sum())
    assert cnt[1] > 0
