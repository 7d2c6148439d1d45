"""Belief propagation on the float staircase kernel, the part a CPU can check:
the host BP decoder -- the reference of test_gpu_bp_stair.py -- against the
numpy restatement bp_ref on a staircase table, which pins the tail check of
degree D0 - 1 and the wrap from the tail to check 0 that the GPU comparisons
rely on; the group-width rule of the BP kernel against its restatement; and
the new entry points on a host context."""
import ctypes as C
import math

import numpy as np
import pytest

import bp_ref as R
import float_domain as FD
import struct_domain as ST
from ldpcgputegra_amd import ALGO_BP, Code, Decoder, LdpcError, _lib, channel, default_params, load_table
from test_bp_cpu import u32

TABLE = ST.short_staircase(5, 32)      # 32 checks: 31 of degree 7 and the tail of degree 6; N = 160
ITERS = 2
BATCH = 5


def grid_llr(n, batch):
    """The first n columns of float_domain's coarse grid of 648x324 (it has
    zeros, +0.0), every 7th column -0.0."""
    x = np.array(FD.grid("648x324", batch, "coarse")[:, :n])
    x[:, ::7] = -0.0
    return x


def awgn_llr(t, batch, ebn0=2.0):
    sigma = channel.sigma_from_ebn0(ebn0, t.k_info / t.n)
    return channel.awgn_f32_host(t.n, batch, seed=R.INPUT_SEED, sigma=sigma, normalize=True)


@pytest.mark.parametrize("kind", ["grid", "awgn"])
def test_host_decoder_is_the_definition_on_a_staircase(kind):
    t = TABLE
    assert [tuple(g) for g in t.groups] == [(7, 31), (6, 1)] and t.n == 160
    llr = grid_llr(t.n, BATCH) if kind == "grid" else awgn_llr(t, BATCH)
    if kind == "grid":
        z = u32(llr)
        assert (z == 0).any() and (z == 0x80000000).any()
    exp = R.decode(t, llr, ITERS)
    dec = Decoder(Code(t), device=-1, max_batch=BATCH)
    got = dec.decode_f32_soft(llr, ITERS, default_params(algo=ALGO_BP))
    assert np.array_equal(got[0], exp[0])
    assert np.array_equal(u32(got[1]), u32(exp[1])), "%d soft values differ" % int((u32(got[1]) != u32(exp[1])).sum())
    assert np.array_equal(got[2], exp[2]) and (got[2] == ITERS).all()
    dec.close()


def model_width(X, m, stride, widths):
    """stairbp.hip stairbp_model_width, restated: the least of
    (m / S) * (3X - 1 + S) * f(w) -- groups per iteration, box-plus per group,
    and what sharing a CU costs a wave: w = stride * S / 64 / 256 waves per CU,
    f = 1 up to two and (w / 2) ** (5 / 8) beyond; the wider width on a tie."""
    best = None
    for S in (16, 8, 4, 2):
        if S not in widths or m % S:
            continue
        w = stride * S / 64.0 / 256.0
        cost = float((m // S) * (3 * X - 1 + S)) * (math.pow(w / 2.0, 0.625) if w > 2.0 else 1.0)
        if best is None or cost < best[0]:
            best = (cost, S)
    return best[1] if best else 0


def lib_width(X, m, stride, widths):
    return _lib.lib().ldpc_bp_staircase_width_model(X, m, stride, sum(widths))


def test_width_model():
    """DVB-S2 r1/2 (X = 5, M = 32400, all four widths): 16 at batch 1024, where
    every width leaves at most two waves on a CU, 8 at 4096 and at 16384 (the
    fastest measured widths, profiles/bp_stair_rate.json), where min-sum takes
    4 and 2."""
    t = load_table("dvbs2_r1_2")
    X, m = t.groups[0][0] - 2, t.m
    assert (X, m) == (5, 32400)
    all4 = (2, 4, 8, 16)
    assert [model_width(X, m, s, all4) for s in (1024, 4096, 16384)] == [16, 8, 8]
    for stride in (64, 1024, 2048, 4096, 4160, 8192, 16384):
        for widths in (all4, (2, 4, 8), (2,), (4, 16), ()):
            for XX, mm in ((X, m), (28, 6480), (12, 1440), (5, 360)):
                assert lib_width(XX, mm, stride, widths) == model_width(XX, mm, stride, widths), (stride, widths, XX, mm)
    assert lib_width(5, 360, 1024, all4) == model_width(5, 360, 1024, all4) == 8    # 360 % 16 != 0


def test_switch_on_a_host_context():
    L = _lib.lib()
    dec = Decoder(Code("dvbs2_r1_2"), device=-1, max_batch=4)
    assert dec.bp_staircase is False
    with pytest.raises(LdpcError) as e:
        dec.set_bp_staircase(True)
    assert e.value.status == _lib.LDPC_EUNSUPPORTED and dec.bp_staircase is False
    with pytest.raises(LdpcError) as e:
        Decoder(Code("dvbs2_r1_2"), device=-1, max_batch=4, bp_staircase=True)
    assert e.value.status == _lib.LDPC_EUNSUPPORTED
    on = C.c_int(5)
    assert L.ldpc_ctx_set_bp_staircase(None, 1) == _lib.LDPC_EINVAL
    assert L.ldpc_ctx_get_bp_staircase(None, C.byref(on)) == _lib.LDPC_EINVAL
    assert L.ldpc_ctx_get_bp_staircase(dec._ctx, None) == _lib.LDPC_EINVAL and on.value == 5
    dec.close()
