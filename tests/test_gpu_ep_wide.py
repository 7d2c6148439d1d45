"""`ldsepw` on the GPU: kernel family 9 with one codeword spread over W = 2 or 4
waves (csrc/ldsepw.hip, behind the ep_wide switch), against the oracle's serial
float decode (oracle/ldpc_oracle.c oracle_decode_f32).  The comparison is
test_gpu_float_domain.assert_same's, as for `ldsep`: soft output equal to the
oracle's as floats, bit for bit equal to the oracle on the input + 0.0, hard
decisions and iterations used exact.  Inputs are on float_domain's dyadic
grids, so nothing rounds and equality is the tolerance.

* the synthetic tables of test_ep_wide_cpu.SYNTHETIC (ragged, idle and full
  waves; a last pass of four checks and of one; the largest Z) at check degrees
  2, 5 and 8 (six padding lanes; the odd flip; none), every compiled W forced by
  LDPC_EPW_WAVES, MS / OMS 0.5 / NMS 0.75 at batches 1 and 5 with guard rows
  behind every output, 3 iterations, on the coarse grid and with -0.0;
* 1944x972, 1248x624 and 2304x1152 at every compiled W, 6 iterations at batch
  5: coarse grid, -0.0, and the fine grid scaled into the subnormals and to 2^100;
* early termination on the inputs test_ep_wide_cpu fixes: neighbouring
  workgroups stop at different iterations, one never stops;
* the switch: off, every answer is the parent's; on, the automatic choice
  follows ``waves_auto``, 648x324 keeps the one-wave kernel, BP, binary16 and
  int8 are untouched, a W outside the mask is LDPC_EUNSUPPORTED;
* the fused error count against the separate count kernel;
* a 648x324 and a 1944x972 decoder used alternately, the latter alternating
  its W and its family."""
import numpy as np
import pytest

import float_domain as FD
import ldsep_domain as ED
import oracle as O
import test_ep_wide_cpu as EW
from float_short_domain import synthetic_input      # the coarse grid at 2 dB for a Table
from ldpcgputegra_amd import ALGO_BP, ALGO_MS, ALGO_NMS, ALGO_OMS, Code, Decoder, LdpcError, _lib, default_params
from test_gpu_float_domain import assert_same

pytestmark = pytest.mark.gpu

# name -> (product algo, oracle algo, beta)
ALGOS = {"MS": (ALGO_MS, O.OMS, 0.0), "OMS0.5": (ALGO_OMS, O.OMS, 0.5), "NMS0.75": (ALGO_NMS, O.NMS, 0.75)}
HARD_FILL, SOFT_FILL, ITS_FILL = 9, 99.0, -7
SYN_BATCH, SYN_ITERS = 5, 3
SHIP_BATCH, SHIP_ITERS, SHIP_EBN0 = 5, 6, 2.0
_inputs = {}


def _torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def run(dec, x, iters, params, extra=2):
    """(hard, soft, iters_used) of one device decode of the host array x, with guard rows behind every output"""
    torch = _torch()
    B, n = x.shape
    d_llr = torch.from_numpy(np.array(x)).cuda()
    d_hard = torch.full((B + extra, n), HARD_FILL, dtype=torch.uint8, device="cuda")
    d_soft = torch.full((B + extra, n), SOFT_FILL, dtype=torch.float32, device="cuda")
    d_its = torch.full((B + extra,), ITS_FILL, dtype=torch.int32, device="cuda")
    dec.decode_f32_device(d_llr, d_hard, iters, params=params, soft=d_soft, iters_used=d_its)
    torch.cuda.synchronize()
    hard, soft, its = d_hard.cpu().numpy(), d_soft.cpu().numpy(), d_its.cpu().numpy()
    assert (hard[B:] == HARD_FILL).all() and (soft[B:] == SOFT_FILL).all() and (its[B:] == ITS_FILL).all(), \
        "rows beyond the batch written"
    return hard[:B], soft[:B], its[:B]


_oracle = {}


def oracle(t, x, oalgo, beta, iters, early=False, plus_zero=False):
    """(hard, soft, iters_used) of the oracle on x (plus_zero: on x + 0.0), computed once per case and read-only;
    t and x are the cached objects of this module and of float_domain, so their identity names them"""
    key = (id(t), id(x), oalgo, float(beta), iters, bool(early), plus_zero)
    if key not in _oracle:
        y = x + np.float32(0.0) if plus_zero else x
        out = O.decode_f32(t, y, iters, oalgo, beta, early_term=early, threads=O.host_threads())
        for a in out:
            a.setflags(write=False)
        _oracle[key] = (out, t, x)      # t and x kept alive: their ids stay theirs
    return _oracle[key][0]


def compare(dec, t, x, algo, iters, where, early=False, beta_scale=1.0, batches=None):
    """decode x[:b] for every b of `batches` on dec and hold it to the oracle on x and on x + 0.0"""
    palgo, oalgo, beta = ALGOS[algo]
    b = beta if oalgo == O.NMS else beta * beta_scale
    exp = exp_pos = oracle(t, x, oalgo, b, iters, early)
    if np.signbit(x[x == 0]).any():
        exp_pos = oracle(t, x, oalgo, b, iters, early, plus_zero=True)
    params = default_params(algo=palgo, beta=b, early_term=int(early))
    for batch in batches or (x.shape[0],):
        got = run(dec, x[:batch], iters, params)
        w = "%s batch %d W %d" % (where, batch, dec.last_ep_waves)
        assert dec.last_kernel == "ldsep" and dec.last_lds_shape == (0, False), w
        assert_same(got, tuple(a[:batch] for a in exp), w, bitwise=False)
        assert_same(got, tuple(a[:batch] for a in exp_pos), w + " vs the oracle on the input + 0.0", bitwise=True)
    return exp


# ---- synthetic tables -------------------------------------------------------------

SYN_CASES = [(d, rows, Z) for rows, Z in sorted(EW.SYNTHETIC) for d in EW.DEGREES]


@pytest.mark.parametrize("d,rows,Z", SYN_CASES, ids=[ED.synthetic_name(*k) for k in SYN_CASES])
def test_synthetic_tables(d, rows, Z, monkeypatch):
    t = ED.synthetic(d, rows, Z)
    waves = EW.SYNTHETIC[(rows, Z)][1]
    x = synthetic_input(t, ("syn", d, rows, Z), SYN_BATCH)
    neg = _inputs.setdefault(("syn-0", d, rows, Z), FD.negzero(x))
    dec = Decoder(Code(t), max_batch=8, kernel=9, ep_wide=True)
    assert dec.ep_wide is True
    for w in waves:
        monkeypatch.setenv("LDPC_EPW_WAVES", str(w))
        for algo in sorted(ALGOS):
            for kind, inp in (("coarse", x), ("negzero", neg)):
                compare(dec, t, inp, algo, SYN_ITERS, "%s %s %s" % (ED.synthetic_name(d, rows, Z), kind, algo),
                        batches=(1, SYN_BATCH))
                assert dec.last_ep_waves == w
    dec.close()


# ---- the shipped tables -----------------------------------------------------------

def shipped_input(code, kind):
    key = ("ship", code, kind)
    if key not in _inputs:
        if kind in FD.GRIDS:
            _inputs[key] = FD.grid_input(code, SHIP_BATCH, SHIP_EBN0, *FD.GRIDS[kind])
        elif kind == "negzero":
            _inputs[key] = FD.negzero(shipped_input(code, "coarse"))
        else:
            _inputs[key] = FD.scaled(shipped_input(code, "fine"), FD.SCALES[kind])
    return _inputs[key]


@pytest.mark.parametrize("code", sorted(EW.SHIPPED))
def test_shipped_tables(code, monkeypatch):
    from ldpcgputegra_amd import load_table
    t = load_table(code)
    dec = Decoder(Code(code), max_batch=8, kernel=9, ep_wide=True)
    for w in EW.SHIPPED[code][2]:
        monkeypatch.setenv("LDPC_EPW_WAVES", str(w))
        for kind in ("coarse", "negzero", "sub", "big"):
            x = shipped_input(code, kind)
            # on the scaled inputs the offset is scaled like the input; NMS would round there
            for algo in (("MS", "OMS0.5") if kind in FD.SCALES else sorted(ALGOS)):
                exp = compare(dec, t, x, algo, SHIP_ITERS, "%s %s %s" % (code, kind, algo),
                              beta_scale=FD.SCALES.get(kind, 1.0))
                assert dec.last_ep_waves == w
            if kind == "sub":      # subnormals are kept: the soft output holds them
                soft = exp[1]
                assert ((soft != 0) & (np.abs(soft) < np.finfo(np.float32).tiny)).any()
    dec.close()


# ---- early termination ------------------------------------------------------------

@pytest.mark.parametrize("code", sorted(EW.ET_EBN0))
def test_early_termination(code, monkeypatch):
    from ldpcgputegra_amd import load_table
    t = load_table(code)
    x = EW.et_input(code)
    ref_its = EW.et_oracle(code)[2]
    assert len(set(ref_its.tolist())) >= 2 and (ref_its == EW.ET_ITERS).any()
    dec = Decoder(Code(code), max_batch=16, kernel=9, ep_wide=True)
    for w in EW.SHIPPED[code][2]:
        monkeypatch.setenv("LDPC_EPW_WAVES", str(w))
        for algo in sorted(ALGOS):
            exp = compare(dec, t, x, algo, EW.ET_ITERS, "%s early termination %s" % (code, algo), early=True,
                          batches=(EW.ET_BATCH, 1))
            assert dec.last_ep_waves == w
            if algo == "MS":
                assert np.array_equal(exp[2], ref_its)
    dec.close()


# ---- the switch and the selection -------------------------------------------------

def _status(fn):
    with pytest.raises(LdpcError) as e:
        fn()
    return e.value.status


def _decode(dec, x, params=None, iters=2):
    torch = _torch()
    hard = torch.zeros(x.shape, dtype=torch.uint8, device="cuda")
    dec.decode_f32_device(torch.from_numpy(np.array(x)).cuda(), hard, iters, params=params)
    torch.cuda.synchronize()
    return hard.cpu().numpy()


def test_switch_off_is_the_parent():
    x = shipped_input("1944x972", "coarse")
    dec = Decoder(Code("1944x972"), max_batch=8)
    assert dec.ep_wide is False
    _decode(dec, x)
    assert dec.last_kernel == "lds" and dec.last_ep_waves == 0
    assert _status(lambda: dec.set_kernel(9)) == _lib.LDPC_EUNSUPPORTED
    assert dec.kernel == 0
    # on and off again: the parent's answers are back
    dec.set_ep_wide(True)
    dec.set_kernel(9)
    _decode(dec, x)
    assert dec.last_kernel == "ldsep" and dec.last_ep_waves in (2, 4)
    dec.set_ep_wide(False)
    assert _status(lambda: _decode(dec, x)) == _lib.LDPC_EUNSUPPORTED      # a forced 9 no longer fits
    dec.set_kernel(0)
    _decode(dec, x)
    assert dec.last_kernel == "lds" and dec.last_ep_waves == 0
    assert _status(lambda: dec.set_kernel(9)) == _lib.LDPC_EUNSUPPORTED
    dec.close()


@pytest.mark.parametrize("code", sorted(EW.SHIPPED))
def test_switch_on_automatic_choice(code, monkeypatch):
    monkeypatch.delenv("LDPC_EPW_WAVES", raising=False)
    from ldpcgputegra_amd import load_table
    t = load_table(code)
    x = shipped_input(code, "coarse")
    exp = oracle(t, x, O.OMS, 0.0, 2)[0]
    c = Code(code)
    dec = Decoder(c, max_batch=8, ep_wide=True)
    off = Decoder(c, max_batch=8)
    auto = c.ep_wide_info(x.shape[0])["waves_auto"]
    hard = _decode(dec, x)
    assert np.array_equal(hard, exp)
    _decode(off, x)
    if auto:
        assert (dec.last_kernel, dec.last_ep_waves) == ("ldsep", auto)
    else:       # the rule leaves this batch to the old family
        assert (dec.last_kernel, dec.last_ep_waves) == (off.last_kernel, 0)
    # BP keeps its family, whatever the switch says, forced 9 included
    bp = default_params(algo=ALGO_BP)
    hb = _decode(dec, x, bp)
    assert np.array_equal(hb, _decode(off, x, bp))
    assert dec.last_kernel == off.last_kernel == "lds" and dec.last_ep_waves == 0
    dec.set_kernel(9)
    assert _status(lambda: _decode(dec, x, bp)) == _lib.LDPC_EUNSUPPORTED
    dec.close()
    off.close()


def test_short_code_keeps_the_one_wave_kernel(monkeypatch):
    monkeypatch.setenv("LDPC_EPW_WAVES", "4")      # forces W only where ldsepw runs
    x = FD.make("648x324", 5, "coarse")
    for kernel in (0, 9):
        dec = Decoder(Code("648x324"), max_batch=8, kernel=kernel, ep_wide=True)
        hard = _decode(dec, x, iters=6)
        assert dec.last_kernel == "ldsep" and dec.last_ep_waves == 0
        assert np.array_equal(hard, FD.oracle_on("648x324", 5, "coarse", O.OMS, 0.0, 6)[0])
        dec.close()
    # a table of neither shape: the switch is accepted and changes nothing
    dec = Decoder(Code("200x100"), max_batch=8, ep_wide=True)
    assert _status(lambda: dec.set_kernel(9)) == _lib.LDPC_EUNSUPPORTED
    _decode(dec, FD.make("200x100", 5, "coarse"))
    assert dec.last_kernel == "generic" and dec.last_ep_waves == 0
    dec.close()


def test_other_element_types_unchanged():
    """binary16 (with f16_all_codes, which 1944x972 needs) and int8 on 1944x972: the same family and the same
    bytes with the switch on and off, with family 9 forced (refused) and not"""
    torch = _torch()
    code = Code("1944x972")
    x = shipped_input("1944x972", "coarse")
    q = torch.from_numpy(np.array(x).astype(np.int8)).cuda()
    h = torch.from_numpy(np.array(x)).cuda().to(torch.float16)
    out = {}
    for on in (False, True):
        dec = Decoder(code, max_batch=8, f16_all_codes=True, ep_wide=on)
        hard = torch.zeros(x.shape, dtype=torch.uint8, device="cuda")
        soft = torch.zeros(x.shape, dtype=torch.float16, device="cuda")
        dec.decode_f16_device(h, hard, 3, soft=soft)
        torch.cuda.synchronize()
        f16 = (dec.last_kernel, dec.last_ep_waves, hard.cpu().numpy(), soft.cpu().numpy().view(np.uint16))
        dec.decode_i8_device(q, hard, 3)
        torch.cuda.synchronize()
        out[on] = f16 + (dec.last_kernel, dec.last_ep_waves, hard.cpu().numpy())
        if on:
            dec.set_kernel(9)
            assert _status(lambda: dec.decode_f16_device(h, hard, 3)) == _lib.LDPC_EUNSUPPORTED
            assert _status(lambda: dec.decode_i8_device(q, hard, 3)) == _lib.LDPC_EUNSUPPORTED
        dec.close()
    for a, b in zip(out[False], out[True]):
        assert np.array_equal(a, b)
    assert out[True][0] == "lds" and out[True][1] == 0 and out[True][5] == 0


def test_waves_outside_the_mask(monkeypatch):
    x = shipped_input("2304x1152", "coarse")
    dec = Decoder(Code("2304x1152"), max_batch=8, kernel=9, ep_wide=True)
    for w in ("2", "3", "8", "1"):
        monkeypatch.setenv("LDPC_EPW_WAVES", w)
        assert _status(lambda: _decode(dec, x)) == _lib.LDPC_EUNSUPPORTED, w
    monkeypatch.setenv("LDPC_EPW_WAVES", "4")
    _decode(dec, x)
    assert dec.last_ep_waves == 4
    dec.close()


# ---- error counts -----------------------------------------------------------------

@pytest.mark.parametrize("w", (2, 4))
def test_fused_error_count(w, monkeypatch):
    """13 codewords of 1944x972 at 1.6 dB, 4 iterations: some frames fail.  The count of ldsepw's epilogue, the
    separate count kernel (LDPC_FUSED_COUNT=0) and numpy on the hard decisions agree, with and without a
    reference codeword array."""
    torch = _torch()
    code = Code("1944x972")
    n, k = code.n, code.k_info
    x = FD.grid_input("1944x972", 13, 1.6, *FD.FINE)
    d_llr = torch.from_numpy(np.array(x)).cuda()
    ref = torch.zeros((13, n), dtype=torch.uint8, device="cuda")
    ref[:, ::5] = 1
    monkeypatch.setenv("LDPC_EPW_WAVES", str(w))
    dec = Decoder(code, max_batch=16, kernel=9, ep_wide=True)
    for r in (None, ref):
        got = {}
        for fused in ("1", "0"):
            monkeypatch.setenv("LDPC_FUSED_COUNT", fused)
            hard = torch.zeros((13, n), dtype=torch.uint8, device="cuda")
            counts = torch.zeros(2, dtype=torch.int64, device="cuda")
            dec.decode_count_device(d_llr, hard, 4, k, counts, ref=r)
            torch.cuda.synchronize()
            assert (dec.last_kernel, dec.last_ep_waves) == ("ldsep", w)
            got[fused] = tuple(int(v) for v in counts.cpu().numpy())
            diff = hard.cpu().numpy()[:, :k] ^ (0 if r is None else r.cpu().numpy()[:, :k])
            assert got[fused] == (int(diff.sum()), int(diff.any(axis=1).sum())), (fused, r is None)
        assert got["1"] == got["0"]
        assert got["1"][1] > 0
    dec.close()


# ---- context reuse ----------------------------------------------------------------

def test_decoders_used_alternately(monkeypatch):
    from ldpcgputegra_amd import load_table
    monkeypatch.delenv("LDPC_EPW_WAVES", raising=False)
    short = Decoder(Code("648x324"), max_batch=64, ep_wide=True)
    wide = Decoder(Code("1944x972"), max_batch=64, kernel=9, ep_wide=True)
    xs = FD.make("648x324", 37, "coarse")
    xw = FD.grid_input("1944x972", 37, SHIP_EBN0, *FD.COARSE)
    es = FD.oracle_on("648x324", 37, "coarse", O.OMS, 0.0, 6)
    ew = oracle(load_table("1944x972"), xw, O.OMS, 0.0, 6)
    p = default_params(algo=ALGO_MS)
    for rnd, (batch, w, kernel) in enumerate(((37, "2", 9), (5, "4", 9), (1, "2", 7), (37, "4", 9), (9, None, 9))):
        got = run(short, xs[:batch], 6, p)
        assert (short.last_kernel, short.last_ep_waves) == ("ldsep", 0)
        assert_same(got, tuple(a[:batch] for a in es), "648x324 round %d" % rnd, bitwise=True)     # no zero is -0.0 here
        if w:
            monkeypatch.setenv("LDPC_EPW_WAVES", w)
        else:
            monkeypatch.delenv("LDPC_EPW_WAVES", raising=False)
        wide.set_kernel(kernel)
        got = run(wide, xw[:batch], 6, p)
        assert wide.last_kernel == ("ldsep" if kernel == 9 else "lds")
        assert wide.last_ep_waves == (0 if kernel == 7 else int(w) if w else
                                      EW.rule(12, 11, 0b10100, batch)[0])
        assert_same(got, tuple(a[:batch] for a in ew), "1944x972 round %d" % rnd, bitwise=True)
    short.close()
    wide.close()
