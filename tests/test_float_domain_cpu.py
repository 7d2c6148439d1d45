"""The float decode on tied, zero, -0.0, subnormal and large LLRs, CPU side
(float_domain.py): the inputs do hold the ties and zeros they are meant to,
the oracle's serial float decode (oracle/ldpc_oracle.c oracle_decode_f32, the
definition: the reference has no float decoder) commutes with a power-of-two
scaling into the subnormal and the large range, its outputs keep zeros and no
NaN, and the product's host float decoder (device = -1, csrc/host.cpp) gives
the oracle's hard decisions on all of them.

test_gpu_float_domain.py rests on this file: its references are these oracle
decodes, and the scaling identity gives its subnormal case a reference that
does not rest on the host's handling of subnormals alone."""
import numpy as np
import pytest

import float_domain as FD
import oracle as O
from ldpcgputegra_amd import ALGO_MS, ALGO_NMS, ALGO_OMS, Code, Decoder, default_params, load_table

CODES = FD.SHORT + FD.DVBS2
HOST_CODES = ["648x324", "576x288", "dvbs2_r1_2"]
HOST_BATCH = 8
# (name, product algo, oracle algo, beta)
HOST_ALGOS = [("MS", ALGO_MS, O.OMS, 0.0), ("OMS0.5", ALGO_OMS, O.OMS, 0.5), ("OMS4", ALGO_OMS, O.OMS, 4.0),
              ("NMS0.75", ALGO_NMS, O.NMS, 0.75)]
_decs = {}


def iters_of(code):
    return 3 if load_table(code).n > 10000 else 6


def host(code):
    if code not in _decs:
        _decs[code] = Decoder(Code(code), device=-1, max_batch=64)
    return _decs[code]


def test_grid_input_is_what_it_says():
    x = FD.make("648x324", 8, "fine")
    assert x.dtype == np.float32 and x.shape == (8, 648) and not x.flags.writeable
    assert FD.make("648x324", 8, "fine") is x
    k = x.astype(np.float64) / 0.5
    assert np.array_equal(k, np.rint(k)) and np.abs(k).max() == 16 and not np.signbit(x[x == 0]).any()
    c = FD.make("648x324", 8, "coarse")
    assert sorted(np.unique(c).tolist()) == [-4, -3, -2, -1, 0, 1, 2, 3, 4]
    assert x.mean() < -3.0 and c.mean() < -2.0            # the all-zero codeword: negative LLRs
    z = FD.make("648x324", 8, "negzero")
    assert np.array_equal(z == 0, (c == 0) | (np.arange(648) % 7 == 0)[None, :])
    assert np.signbit(z[z == 0]).all() and np.array_equal(z[z != 0], c[z != 0])
    sub, big = FD.make("648x324", 8, "sub"), FD.make("648x324", 8, "big")
    tiny = np.finfo(np.float32).tiny
    assert ((sub == 0) == (x == 0)).all() and (np.abs(sub[sub != 0]) < tiny).all()      # every nonzero is subnormal
    assert np.array_equal(sub.astype(np.float64) * 2.0 ** 130, x) and np.array_equal(big.astype(np.float64) * 2.0 ** -100, x)
    # another stream is another input
    assert not np.array_equal(FD.grid("648x324", 8, "fine", stream=12), x)


@pytest.mark.parametrize("grid", sorted(FD.GRIDS))
@pytest.mark.parametrize("code", CODES)
def test_inputs_hold_ties_and_zeros(code, grid):
    """A condition on the inputs: in the first iteration at least a tenth of
    the checks meet min1 == min2, and at least a tenth meet min1 == 0.
    Measured with 8 codewords, (ties, zeros) on the coarse / the fine grid:
      648x324          0.383 0.438 / 0.224 0.260    576x288          0.340 0.379 / 0.209 0.217
      200x100          0.324 0.388 / 0.171 0.214    1944x972         0.382 0.409 / 0.232 0.227
      dvbs2_r1_2       0.373 0.406 / 0.221 0.226    dvbs2_r2_3       0.332 0.323 / 0.187 0.176
      dvbs2shape_r3_4  0.331 0.304 / 0.186 0.160    dvbs2shape_r5_6  0.335 0.301 / 0.185 0.162
      dvbs2_r8_9       0.315 0.217 / 0.152 0.114    dvbs2_r9_10      0.314 0.207 / 0.146 0.111"""
    ties, zeros = FD.first_iteration_shares(load_table(code), FD.make(code, 8, grid))
    print("%s %s: ties %.3f zeros %.3f" % (code, grid, ties, zeros))
    assert ties >= 0.10 and zeros >= 0.10, (ties, zeros)


@pytest.mark.parametrize("beta", [0.0, 0.5])
@pytest.mark.parametrize("scale", sorted(FD.SCALES))
@pytest.mark.parametrize("code", ["648x324", "dvbs2_r1_2"])
def test_oracle_scaling_identity(code, scale, beta):
    """decode(x * s, OMS, beta * s) = decode(x, OMS, beta) * s for s = 2^-130
    (every nonzero value subnormal) and 2^100: soft output equal, hard
    decisions the same.  Every operation of the decode on a grid input is
    exact, so it commutes with an exact scaling."""
    s = FD.SCALES[scale]
    h0, v0, _ = FD.oracle_on(code, HOST_BATCH, "fine", O.OMS, beta, 6)
    h1, v1, _ = FD.oracle_on(code, HOST_BATCH, scale, O.OMS, beta, 6)
    assert not np.isnan(v1).any()
    assert np.array_equal(v1, FD.scaled(v0, s))
    assert np.array_equal(h1, h0)
    assert (v1 != 0).any() and (scale != "sub" or np.abs(v1).max() < 2.0 ** -110)


@pytest.mark.parametrize("code", CODES)
def test_oracle_outputs_hold_zeros_and_no_nan(code):
    """The references of the GPU tests: no NaN on any input kind, and zeros in
    the soft output of the zero-heavy cases (coarse grid under plain min-sum;
    measured 1 .. 7 %), so the zero path stays exercised to the end."""
    iters = iters_of(code)
    for kind in ("coarse", "fine", "negzero", "sub", "big"):
        for name, _, oalgo, beta in HOST_ALGOS:
            if kind in FD.SCALES and oalgo == O.NMS:
                continue
            _, v, _ = FD.oracle_on(code, HOST_BATCH, kind, oalgo, beta, iters)
            assert not np.isnan(v).any() and np.isfinite(v).all(), (kind, name)
    _, v, _ = FD.oracle_on(code, HOST_BATCH, "coarse", O.OMS, 0.0, iters)
    print("%s coarse MS: %.2f %% zeros" % (code, 100 * (v == 0).mean()))
    assert (v == 0).mean() > 0


def test_oracle_clamped_negzero_output_holds_zeros():
    """-0.0 input under OMS beta = 4.0 (most messages clamp to zero), 648x324,
    6 iterations: measured 18 % zeros in the soft output."""
    _, v, _ = FD.oracle_on("648x324", HOST_BATCH, "negzero", O.OMS, 4.0, 6)
    print("negzero OMS 4.0: %.2f %% zeros, %.2f %% of them -0.0" % (100 * (v == 0).mean(),
                                                                   100 * np.signbit(v[v == 0]).mean()))
    assert (v == 0).mean() > 0


@pytest.mark.parametrize("algo", HOST_ALGOS, ids=[a[0] for a in HOST_ALGOS])
@pytest.mark.parametrize("code", ["648x324", "dvbs2_r1_2"])
def test_oracle_sign_of_zero(code, algo):
    """What the GPU test holds ldsep to: the sign of a zero LLR changes only
    the sign of zero outputs (c < 0 is false for both, and a zero's sign only
    reaches messages of magnitude zero), and from an input without -0.0 the
    decode never produces one (c = V - m and V = c + m are -0.0 only from
    -0.0 operands, and only V = -0.0 + -0.0 needs no -0.0 c).  A -0.0 input
    seldom survives a second iteration (c = V - m with V = m = -0.0 is +0.0),
    so the sign of a zero is looked at after one iteration as well: there the
    output of the -0.0 input still holds -0.0 under every algorithm."""
    name, _, oalgo, beta = algo
    x = FD.make(code, HOST_BATCH, "negzero")
    for iters in (1, iters_of(code)):
        h0, v0, _ = FD.oracle_f32(code, ("negzero", HOST_BATCH), x, oalgo, beta, iters)
        h1, v1, _ = FD.oracle_f32(code, ("negzero + 0.0", HOST_BATCH), x + np.float32(0.0), oalgo, beta, iters)
        assert np.array_equal(v0, v1) and np.array_equal(h0, h1)
        assert not np.signbit(v1[v1 == 0]).any()
        print("%s %s %d iterations: %d zeros, %d of them -0.0" % (code, name, iters, (v0 == 0).sum(),
                                                                  np.signbit(v0[v0 == 0]).sum()))
        assert iters > 1 or np.signbit(v0[v0 == 0]).any()


@pytest.mark.parametrize("algo", HOST_ALGOS, ids=[a[0] for a in HOST_ALGOS])
@pytest.mark.parametrize("kind", ["coarse", "negzero", "sub", "big"])
@pytest.mark.parametrize("code", HOST_CODES)
def test_host_float_decoder_vs_oracle(code, kind, algo):
    """The host float decoder returns hard decisions only: equal to the
    oracle's.  On the scaled inputs the OMS offset is scaled like the input;
    the NMS factor is not."""
    name, palgo, oalgo, beta = algo
    llr = FD.make(code, HOST_BATCH, kind)
    b = beta if oalgo == O.NMS else beta * FD.SCALES.get(kind, 1.0)
    exp, _, _ = FD.oracle_f32(code, (kind, HOST_BATCH), llr, oalgo, b, iters_of(code))
    got = host(code).decode_f32(llr, iters_of(code), default_params(algo=palgo, beta=b))
    assert np.array_equal(got, exp), "%d hard decisions differ" % int((got != exp).sum())
