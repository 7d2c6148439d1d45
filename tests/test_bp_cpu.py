"""Layered belief propagation (LDPC_ALGO_BP), CPU side: g and the box-plus of
csrc/bp_math.h against float64, and the host decoder (device = -1) against
bp_ref.py's numpy restatement of the definition, bit for bit.

test_gpu_bp.py rests on this file: its reference is the host decoder, and its
box-plus inputs are bp_ref.pairs().

Measured here (the figures of DESIGN.md §3):
  g:   max |g(x) - ln(1 + e^-x)| = 1.77e-7 over the inputs below (bound 2^-21 = 4.77e-7)
  [+]: max error above 2^-23 min(|a|, |b|) = 1.90e-7 (bound 2^-20 = 9.54e-7)
  648x324, 2.0 dB, 2000 codewords, 20 iterations: min-sum / BP frame errors, see test_bp_beats_min_sum
"""
import numpy as np
import pytest

import bp_ref as R
import float_domain as FD
import short_domain as SD
from ldpcgputegra_amd import (ALGO_BP, ALGO_MS, Code, Decoder, LdpcError, _lib, boxplus_host, channel, default_params,
                              load_table)

REAL = ["648x324", "576x288", "200x100"]
SYNTH = [2, 3, 4, 32]          # first-group check degree of short_domain.synthetic(d, Z_SYNTH)
Z_SYNTH = SD.Z_SPLIT
BATCH = 5
ET_ITERS = 16
_decs = {}


def u32(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def table_of(name):
    return SD.synthetic(name, Z_SYNTH) if isinstance(name, int) else load_table(name)


def host(name):
    if name not in _decs:
        _decs[name] = Decoder(Code(table_of(name) if isinstance(name, int) else name), device=-1, max_batch=4096)
    return _decs[name]


def awgn_llr(name, batch, ebn0=None):
    """Unrounded true LLRs 2 y / sigma^2 of the all-zero codeword."""
    t = table_of(name)
    ebn0 = FD.EBN0[name] if ebn0 is None else ebn0
    sigma = channel.sigma_from_ebn0(ebn0, t.k_info / t.n)
    return channel.awgn_f32_host(t.n, batch, seed=R.INPUT_SEED, sigma=sigma, normalize=True)


def grid_llr(name, batch):
    """float_domain's coarse grid with its zeros and every 7th column -0.0; a
    synthetic table (N = 384) takes the first N columns of 648x324's."""
    if isinstance(name, int):
        x = np.array(FD.make("648x324", batch, "negzero")[:, :table_of(name).n])
        x.setflags(write=False)
        return x
    return FD.make(name, batch, "negzero")


# ---- g and the box-plus ----------------------------------------------------

def test_input_set_is_what_it_says():
    a, b = R.pairs()
    assert a.dtype == np.float32 and a.shape == b.shape and not a.flags.writeable
    assert a.size >= 4_000_000 + (2 * R.GRID.size) ** 2
    n = R.N_RANDOM
    assert 39.9 < np.abs(a[:n]).max() <= 40 and 1.99 < np.abs(b[n:2 * n]).max() <= 2
    g = a[2 * n:2 * n + (2 * R.GRID.size) ** 2]
    assert np.signbit(g[g == 0]).any() and not np.signbit(g[g == 0]).all()      # both zeros
    assert (np.abs(g[g != 0]) < np.finfo(np.float32).tiny).any() and (np.abs(g) == np.float32(1e30)).any()
    assert (np.abs(a) == np.abs(b)).sum() >= 4 * 4096
    bnd = R.g_boundaries()
    assert (bnd < R.G_CUT).any() and (bnd >= R.G_CUT).any() and bnd.size == 27 * 17
    # both sides of every range-reduction boundary: k steps inside each group of 17
    k = np.trunc(np.minimum(bnd, R.G_CUT) * R.INV_LN2 + np.float32(0.5)).reshape(27, 17)
    assert (k[:26, 0] + 1 == k[:26, -1]).all()


def test_numpy_restatement_is_the_products_boxplus():
    """box32 / g32 (bp_ref.py) restate bp_math.h operation by operation: equal
    to ldpc_boxplus_f32_host on every pair, so what the next test measures on
    g32 is the g inside the product."""
    a, b = R.pairs()
    assert np.array_equal(u32(boxplus_host(a, b)), u32(R.box32(a, b)))


def test_g_against_float64():
    a, b = R.pairs()
    x = np.concatenate([np.abs(a) + np.abs(b), np.abs(np.abs(a) - np.abs(b)), np.abs(a), R.g_boundaries(), R.GRID])
    g = R.g32(x)
    err = np.abs(g.astype(np.float64) - R.g64(x))
    print("g: max error %.3e at x = %r (bound %.3e)" % (err.max(), float(x[err.argmax()]), 2.0 ** -21))
    assert err.max() <= 2.0 ** -21
    assert (g[x >= R.G_CUT] == 0).all() and not np.signbit(g[x >= R.G_CUT]).any()     # exactly +0 from the cutoff on
    assert (g[x < R.G_CUT] > 0).all()


def test_boxplus_against_float64():
    a, b = R.pairs()
    got = boxplus_host(a, b)
    assert np.isfinite(got).all()
    mn = np.minimum(np.abs(a), np.abs(b)).astype(np.float64)
    err = np.abs(got.astype(np.float64) - R.box64(a, b))
    over = err - 2.0 ** -23 * mn
    print("[+]: max error above 2^-23 min(|a|, |b|): %.3e at (%r, %r) (bound %.3e); max error %.3e"
          % (over.max(), float(a[over.argmax()]), float(b[over.argmax()]), 2.0 ** -20, err.max()))
    assert (err <= 2.0 ** -20 + 2.0 ** -23 * mn).all()
    # the sign rule: equal signs (zero and -0.0 count as non-negative) give a non-positive result
    same = (a < 0) == (b < 0)
    assert np.signbit(got[same]).all() and not np.signbit(got[~same]).any()


def test_boxplus_zero_and_commutative():
    a, b = R.pairs()
    assert np.array_equal(u32(boxplus_host(a, b)), u32(boxplus_host(b, a)))
    for z in (np.float32(0.0), np.float32(-0.0)):
        r = boxplus_host(a, np.full_like(a, z))
        assert (r == 0).all()
        assert np.array_equal(np.signbit(r), ~(a < 0))          # a [+] 0 = -+0: -0 for a >= 0, +0 for a < 0


def test_boxplus_entry_conventions():
    L = _lib.lib()
    x = np.ones(4, dtype=np.float32)
    out = np.full(4, 7.0, dtype=np.float32)
    assert L.ldpc_boxplus_f32_host(x.ctypes.data, x.ctypes.data, out.ctypes.data, 0) == _lib.LDPC_OK
    assert (out == 7.0).all()
    assert L.ldpc_boxplus_f32_host(None, x.ctypes.data, out.ctypes.data, 4) == _lib.LDPC_EINVAL
    assert L.ldpc_boxplus_f32_host(x.ctypes.data, None, out.ctypes.data, 4) == _lib.LDPC_EINVAL
    assert L.ldpc_boxplus_f32_host(x.ctypes.data, x.ctypes.data, None, 4) == _lib.LDPC_EINVAL
    assert L.ldpc_boxplus_f32_host(x.ctypes.data, x.ctypes.data, out.ctypes.data, -1) == _lib.LDPC_EINVAL
    dec = host("200x100")
    assert L.ldpc_boxplus_f32_async(dec._ctx, None, x.ctypes.data, x.ctypes.data, out.ctypes.data, 4) == \
        _lib.LDPC_EUNSUPPORTED


# ---- the host decoder against the numpy restatement ------------------------

def same_as_ref(name, llr, iters, early=False):
    exp = R.decode(table_of(name), llr, iters, early)
    got = host(name).decode_f32_soft(llr, iters, default_params(algo=ALGO_BP, early_term=int(early)))
    assert np.array_equal(got[0], exp[0]), "%d hard decisions differ" % int((got[0] != exp[0]).sum())
    assert np.array_equal(u32(got[1]), u32(exp[1])), "%d soft values differ" % int((u32(got[1]) != u32(exp[1])).sum())
    assert np.array_equal(got[2], exp[2])
    # the plain entry point gives the same hard decisions
    assert np.array_equal(host(name).decode_f32(llr, iters, default_params(algo=ALGO_BP, early_term=int(early))), exp[0])
    return exp


@pytest.mark.parametrize("iters", [1, 3])
@pytest.mark.parametrize("kind", ["grid", "awgn"])
@pytest.mark.parametrize("name", REAL + SYNTH, ids=str)
def test_host_decoder_is_the_definition(name, kind, iters):
    llr = grid_llr(name, BATCH) if kind == "grid" else awgn_llr(name, BATCH, 2.0)
    _, soft, used = same_as_ref(name, llr, iters)
    assert (used == iters).all() and np.isfinite(soft).all()


# Eb/N0 of the early-termination cases: float_domain.EBN0 (2.0 dB); iters_used of the 5 codewords, measured:
#   648x324  [5 7 4 4 4]      576x288  [5 16 6 4 4]      200x100  [5 3 3 16 6]
@pytest.mark.parametrize("name", REAL)
def test_host_decoder_early_termination(name):
    _, _, used = same_as_ref(name, awgn_llr(name, BATCH), ET_ITERS, early=True)
    print(name, used)
    assert len(set(int(u) for u in used if u < ET_ITERS)) >= 2


def test_beta_is_ignored():
    llr = awgn_llr("200x100", BATCH)
    a = host("200x100").decode_f32_soft(llr, 3, default_params(algo=ALGO_BP, beta=0.15))
    b = host("200x100").decode_f32_soft(llr, 3, default_params(algo=ALGO_BP, beta=7.0))
    assert np.array_equal(u32(a[1]), u32(b[1]))


def test_soft_host_decode_of_min_sum_is_the_oracle():
    """ldpc_decode_f32_soft is new with BP; on min-sum it gives the oracle's
    soft output and iteration counts (the reference the GPU float tests use)."""
    import oracle as O
    llr = FD.make("648x324", 8, "fine")
    exp = FD.oracle_f32("648x324", ("fine", 8), llr, O.OMS, 0.0, 16, early=True)
    got = host("648x324").decode_f32_soft(llr, 16, default_params(algo=ALGO_MS, early_term=1))
    assert np.array_equal(got[0], exp[0]) and np.array_equal(u32(got[1]), u32(exp[1]))
    assert np.array_equal(got[2], exp[2])


def test_bp_beats_min_sum():
    """648x324 at 2.0 dB, 2000 all-zero codewords, 20 iterations, true LLRs:
    measured 166 frame errors under plain min-sum, 21 under BP."""
    s = R.SANITY
    t = load_table(s["code"])
    sigma = channel.sigma_from_ebn0(s["ebn0"], t.k_info / t.n)
    llr = channel.awgn_f32_host(t.n, s["frames"], seed=s["seed"], sigma=sigma, normalize=True)
    fe = {}
    for name, algo in (("MS", ALGO_MS), ("BP", ALGO_BP)):
        hard = host(s["code"]).decode_f32(llr, s["iters"], default_params(algo=algo))
        fe[name] = int(hard[:, :t.k_info].any(axis=1).sum())
    print("frame errors of %d: MS %d, BP %d" % (s["frames"], fe["MS"], fe["BP"]))
    assert fe["MS"] >= 30 and fe["BP"] < fe["MS"] / 2


# ---- the entry points' verdicts --------------------------------------------

def test_int8_bp_is_unsupported_and_algo_4_invalid():
    dec = host("200x100")
    n = dec.code.n
    with pytest.raises(LdpcError) as e:
        dec.decode_i8(np.zeros((1, n), dtype=np.int8), 1, default_params(algo=ALGO_BP))
    assert e.value.status == _lib.LDPC_EUNSUPPORTED
    with pytest.raises(LdpcError) as e:
        dec.decode_f32(np.zeros((1, n), dtype=np.float32), 1, default_params(algo=4))
    assert e.value.status == _lib.LDPC_EINVAL
    assert ALGO_BP == 3 and _lib.lib().ldpc_abi_version() == 1
