"""The float kernels -- generic (1), lds (7), ldsep (9), stairf (11) and the
automatic choice -- on tied, zero, -0.0, subnormal and large LLRs
(float_domain.py), forced one by one, against the oracle's serial float decode
(oracle/ldpc_oracle.c oracle_decode_f32, the definition of the float decode).

The AWGN inputs of test_gpu_parity.py never hold two equal |LLR| in a check, a
zero, a -0.0 or a subnormal, so they cannot tell a wrong tie merge of a
min1 / min2 reduction, a sign-bit test standing in for c < 0, or a flushed
subnormal from a right one.  The inputs here are small dyadic numbers: plain
and offset min-sum with a dyadic beta never round on them, so the comparison
is equality, not a tolerance:

* soft output: no NaN, and equal to the oracle's as floats for every kernel
  (-0.0 == 0.0 counts as equal: ldsep documents that only the sign of a zero
  may differ).  That alone cannot see a sign-bit test: a zero's sign only ever
  reaches messages whose magnitude is zero (the zero is the minimum of every
  other edge of its check, and its own message leaves its own sign out), so
  it changes nothing but the sign of other zeros.  Hence, more than that:
  generic, lds and stairf do the oracle's operations in its order and must
  equal it bit for bit, the sign of a zero included; ldsep makes every zero
  LLR +0.0 on load and must equal, bit for bit, the oracle on that input
  (which never produces a -0.0: test_float_domain_cpu.py);
* hard decisions and iterations used: exactly equal.

test_float_domain_cpu.py shows that the inputs hold the ties and zeros, that
the oracle commutes with the power-of-two scalings, and that the host decoder
agrees with it.

Shapes: batch 37 leaves a ragged ldsep workgroup (4 codewords each) and a
partly empty second stairf wave at every group width (32 / 16 / 8 / 4
codewords per wave); at batch 37 and 5 the lds kernel gives a codeword the
whole wave, which is two lanes per check for the codes whose widest layer is
<= 32 checks (648x324: 27, 200x100: 9) and one lane per check for the others
(576x288: 48, 1944x972: 81); at batch 4096 it packs two codewords of 648x324
into a wave.  6 iterations on the short codes, 3 on N = 64800."""
import numpy as np
import pytest

import float_domain as FD
import oracle as O
from ldpcgputegra_amd import ALGO_MS, ALGO_NMS, ALGO_OMS, Code, Decoder, default_params, load_table

pytestmark = pytest.mark.gpu

CODES = FD.SHORT + FD.DVBS2
BATCH = 37
# name -> (product algo, oracle algo, beta).  ALGO_OMS with beta 0.0 is plain min-sum: same reference as ALGO_MS,
# so the two must give the same result; beta 4.0 clamps most messages to zero
ALGOS = {"MS": (ALGO_MS, O.OMS, 0.0), "OMS0": (ALGO_OMS, O.OMS, 0.0), "OMS0.5": (ALGO_OMS, O.OMS, 0.5),
         "OMS4": (ALGO_OMS, O.OMS, 4.0), "NMS0.75": (ALGO_NMS, O.NMS, 0.75), "NMS1": (ALGO_NMS, O.NMS, 1.0)}
# (kernel, LDPC_STAIRF_S) entries per code, pinned so that none drops out unnoticed (test_tables_match_the_codes),
# and the kernel the automatic choice (0) takes
WIDTHS = [(11, 2), (11, 4), (11, 8), (11, 16)]
KERNELS = {"648x324": [(1, None), (7, None), (9, None), (0, None)], "576x288": [(1, None), (7, None), (9, None), (0, None)],
           "200x100": [(1, None), (7, None), (0, None)], "1944x972": [(1, None), (7, None), (0, None)]}
KERNELS.update({c: [(1, None)] + WIDTHS + [(0, None)] for c in FD.DVBS2})
AUTO = {"648x324": "ldsep", "576x288": "ldsep", "200x100": "generic", "1944x972": "lds"}
AUTO.update({c: "stairf" for c in FD.DVBS2})

_decoders = {}
_device_inputs = {}


def iters_of(code):
    return 3 if load_table(code).n > 10000 else 6


def decoder(code, kernel, max_batch=64):
    key = (code, kernel, max_batch)
    if key not in _decoders:
        _decoders[key] = Decoder(Code(code), max_batch=max_batch, kernel=kernel)
    return _decoders[key]


def _torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def device_input(code, batch, kind):
    key = (code, batch, kind)
    if key not in _device_inputs:
        _device_inputs[key] = _torch().from_numpy(FD.make(code, batch, kind).copy()).cuda()
    return _device_inputs[key]


def run(dec, d_llr, iters, params):
    """(hard, soft, iters_used) of one device decode."""
    torch = _torch()
    B, n = d_llr.shape
    d_hard = torch.full((B, n), 9, dtype=torch.uint8, device="cuda")
    d_soft = torch.full((B, n), 99.0, dtype=torch.float32, device="cuda")
    d_its = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    dec.decode_f32_device(d_llr, d_hard, iters, params=params, soft=d_soft, iters_used=d_its)
    torch.cuda.synchronize()
    return d_hard.cpu().numpy(), d_soft.cpu().numpy(), d_its.cpu().numpy()


def assert_same(got, exp, where, bitwise):
    """The comparison rule of this file; bitwise: the sign of a zero counts."""
    (hard, soft, its), (eh, es, eit) = got, exp
    assert not np.isnan(soft).any(), "%s: NaN in the soft output" % where
    diff = (soft.view(np.uint32) != es.view(np.uint32)) if bitwise else (soft != es)
    assert not diff.any(), "%s: %d soft values differ from the oracle%s, the first at %s: %r, expected %r" % (
        where, int(diff.sum()), " (%d only in the sign of a zero)" % int((diff & (soft == es)).sum()) if bitwise else "",
        tuple(np.argwhere(diff)[0]), soft[diff][0], es[diff][0])
    assert np.array_equal(hard, eh), "%s: %d hard decisions differ" % (where, int((hard != eh).sum()))
    assert np.array_equal(its, eit), "%s: iterations used %s, expected %s" % (where, its.tolist(), eit.tolist())


def check(monkeypatch, code, batch, kind, algo, iters, early=False, entries=None, refs=(), max_batch=64):
    """Decode the named input with every entry of KERNELS[code] (or `entries`)
    and compare with the oracle on that input and with each further reference
    of `refs`.  On the scaled inputs the OMS offset is scaled like the input."""
    palgo, oalgo, beta = ALGOS[algo]
    b = beta if oalgo == O.NMS else beta * FD.SCALES.get(kind, 1.0)
    x = FD.make(code, batch, kind)
    exp = exp_pos = FD.oracle_f32(code, (kind, batch), x, oalgo, b, iters, early)
    if np.signbit(x[x == 0]).any():   # ldsep's reference for the sign of a zero: the input with every zero +0.0
        exp_pos = FD.oracle_f32(code, (kind + " + 0.0", batch), x + np.float32(0.0), oalgo, b, iters, early)
    params = default_params(algo=palgo, beta=b, early_term=int(early))
    for k, width in entries or KERNELS[code]:
        if width:
            monkeypatch.setenv("LDPC_STAIRF_S", str(width))
        else:
            monkeypatch.delenv("LDPC_STAIRF_S", raising=False)
        dec = decoder(code, k, max_batch)
        got = run(dec, device_input(code, batch, kind), iters, params)
        where = "%s %s %s batch %d kernel %d (%s) width %s" % (code, kind, algo, batch, k, dec.last_kernel, width)
        assert dec.last_kernel == (Decoder.KERNEL_NAMES[k] if k else AUTO[code]), where
        if dec.last_kernel == "ldsep":
            assert_same(got, exp, where, bitwise=False)
            assert_same(got, exp_pos, where + " vs the oracle on the input + 0.0", bitwise=True)
        else:
            assert_same(got, exp, where, bitwise=True)
        for ref in refs:
            assert_same(got, ref, where + " vs the scaled reference", bitwise=True)
    return exp


def short_and_dvbs2(short_batches=(BATCH, 5)):
    return [(c, b) for c in FD.SHORT for b in short_batches] + [(c, BATCH) for c in FD.DVBS2]


def test_tables_match_the_codes():
    for code in CODES:
        info = Code(code).layer_info()
        assert info["lds_f32"] == ((7, None) in KERNELS[code]), code
    # the lds kernel's two layouts at batch <= 37 (one codeword per wave): two lanes per check iff 64 >= 2 max_width
    widest = {c: Code(c).layer_info()["max_width"] for c in FD.SHORT}
    assert widest == {"648x324": 27, "576x288": 48, "200x100": 9, "1944x972": 81}


@pytest.mark.parametrize("algo", sorted(ALGOS))
@pytest.mark.parametrize("grid", sorted(FD.GRIDS))
@pytest.mark.parametrize("code,batch", short_and_dvbs2())
def test_grid_inputs_vs_oracle(code, batch, grid, algo, monkeypatch):
    """Coarse and fine grid (ties and zeros in more than a tenth of the checks
    from the first iteration on), every algorithm, every kernel."""
    check(monkeypatch, code, batch, grid, algo, iters_of(code))


@pytest.mark.parametrize("algo", ["MS", "OMS4"])
@pytest.mark.parametrize("code,batch", short_and_dvbs2())
def test_negative_zero_inputs_vs_oracle(code, batch, algo, monkeypatch):
    """Every zero of the coarse grid and every 7th column -0.0: c < 0.0f is
    false for -0.0 where a sign-bit test is true.  OMS 4.0 turns most messages
    into +-0.0 as well.  Also after one iteration only: a -0.0 seldom survives
    a second one (c = V - m with V = m = -0.0 is +0.0), so that is where the
    oracle's output still holds -0.0 and the bit-for-bit comparison can tell
    c < 0.0f from a sign-bit test."""
    exp = check(monkeypatch, code, batch, "negzero", algo, iters_of(code))
    assert (exp[1] == 0).any()
    exp = check(monkeypatch, code, batch, "negzero", algo, 1)
    assert np.signbit(exp[1][exp[1] == 0]).any()


@pytest.mark.parametrize("algo", ["MS", "OMS0.5"])
@pytest.mark.parametrize("scale", sorted(FD.SCALES))
@pytest.mark.parametrize("code", ["648x324", "576x288", "dvbs2_r1_2", "dvbs2_r9_10"])
def test_scaled_inputs_vs_oracle(code, scale, algo, monkeypatch):
    """Fine grid times 2^-130 (every nonzero LLR, message and offset a
    subnormal) and times 2^100, against the oracle on the scaled input and
    against the oracle on the unscaled input times the scale: a kernel that
    flushes subnormals, in a min / max or in the integer ordering of ldsep,
    fails both."""
    _, oalgo, beta = ALGOS[algo]
    iters = iters_of(code)
    h0, v0, i0 = FD.oracle_f32(code, ("fine", BATCH), FD.make(code, BATCH, "fine"), oalgo, beta, iters)
    exp = check(monkeypatch, code, BATCH, scale, algo, iters, refs=[(h0, FD.scaled(v0, FD.SCALES[scale]), i0)])
    assert (exp[1] != 0).mean() > 0.9


ET_ITERS = 16
ET_CODES = FD.SHORT + ["dvbs2_r1_2", "dvbs2_r2_3", "dvbs2shape_r5_6", "dvbs2_r9_10"]


@pytest.mark.parametrize("algo", ["MS", "OMS0.5", "NMS0.75"])
@pytest.mark.parametrize("code", ET_CODES)
def test_early_termination_vs_oracle(code, algo, monkeypatch):
    """Early termination on the fine grid at float_domain.EBN0: the syndrome
    is taken on V > 0 with V full of zeros; the codewords stop at different
    iterations, and iterations used, soft and hard output equal the oracle's.
    ldsep, lds and generic on the short codes, stairf at every width.
    Iterations used by the 37 codewords (first .. last to stop; 16 = never),
    under MS / OMS 0.5 / NMS 0.75:
      648x324     3..16 / 3..11 / 3..16     576x288          2..16 / 2..16 / 2..16
      200x100     1..16 / 1..16 / 2..16     1944x972         4..10 / 4..8  / 4..10
      dvbs2_r1_2  7..10 / 7..9  / 9..16     dvbs2_r2_3       6..8  / 6..8  / 7..12
      dvbs2_r9_10 4..6  / 3..6  / 4..5      dvbs2shape_r5_6  5..7  / 5..7  / 5..7"""
    entries = KERNELS[code] if code in FD.SHORT else WIDTHS + [(0, None)]
    _, _, ref_its = check(monkeypatch, code, BATCH, "fine", algo, ET_ITERS, early=True, entries=entries)
    print("%s %s: iterations used %d .. %d" % (code, algo, ref_its.min(), ref_its.max()))
    assert ref_its.min() < ref_its.max()


@pytest.mark.parametrize("algo", ["MS", "OMS0.5", "NMS0.75"])
def test_lds_packed_waves_vs_oracle(algo, monkeypatch):
    """Kernel 7 at batch 4096 on 648x324: two codewords per wave, one lane per
    check (the layout test_lds_kernel_large_batches runs on untied inputs)."""
    check(monkeypatch, "648x324", 4096, "fine", algo, 6, entries=[(7, None)], max_batch=4096)
