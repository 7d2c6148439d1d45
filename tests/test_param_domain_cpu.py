"""The CPU checkers over the whole parameter and LLR range (param_domain.py):
the oracle against the reference's own SSE decoder (oracle/_ref, where it was
built), and the product's host decoder (device = -1, csrc/host.cpp) against
the oracle, on full-range int8 inputs -- magnitudes 32 .. 127 and -128, which
channel.i8_table's default saturation of 31 never produces -- and on decoder
parameters inside and outside the fast DVB-S2 kernels' domain.  Every
comparison is bit for bit: 0 differing hard decisions.

test_gpu_param_domain.py rests on this file: a mismatch it finds on the GPU is
a kernel or dispatch bug, not a checker bug.

The host decoder's C-ABI entry (ldpc_decode_i8) returns hard decisions only,
no iterations used; with early termination a codeword's hard decisions freeze
at the iteration it stops, so they are what is compared."""
import numpy as np
import pytest

import oracle as O
import param_domain as PD
from ldpcgputegra_amd import Code, Decoder, load_table

REF_CODES = ["dvbs2_r1_2", "dvbs2_r8_9", "dvbs2_r9_10"]
# one code per first-group degree of the staircase kernels (7, 10, 14, 22, 27, 30) and the short 16200x7560
HOST_CODES = ["dvbs2_r1_2", "dvbs2_r2_3", "dvbs2shape_r3_4", "dvbs2shape_r5_6", "dvbs2_r8_9", "dvbs2_r9_10",
              "16200x7560"]
HOST_BATCH, HOST_ITERS = 37, 4
FIXED_INPUTS = ("u128", "sat_flip", "ties")
_decs = {}


def host(code):
    if code not in _decs:
        _decs[code] = Decoder(Code(code), device=-1, max_batch=64)
    return _decs[code]


def test_inputs_are_what_they_say():
    n = 64800
    u = PD.make_input("u128", 32, n)
    assert u.dtype == np.int8 and u.shape == (32, n)
    cnt = np.bincount(u.astype(np.int32).ravel() + 128, minlength=256)
    assert cnt.min() > 0.9 * u.size / 256 and cnt.max() < 1.1 * u.size / 256      # 8100 expected per value
    e = PD.make_input("ext", 32, n)
    vals, cnt = np.unique(e, return_counts=True)
    assert vals.tolist() == [-128, -127, -1, 0, 1, 127] and cnt.min() > 0.98 * e.size / 6
    s = PD.make_input("sat_flip", 32, n)
    assert set(np.unique(s).tolist()) == {-127, 127} and 0.038 < (s == 127).mean() < 0.042
    t = PD.make_input("ties", 32, n)
    assert set(np.unique(t).tolist()) == {-127, 127} and 0.49 < (t == 127).mean() < 0.51
    assert not np.array_equal(s, t) and PD.make_input("ties", 32, n) is t
    # the generator is pinned: splitmix64's first outputs for the state 0 and 1 streams
    assert int(PD.splitmix64(np.uint64(0))) == 0xE220A8397B1DCDAF
    assert int(PD.splitmix64(np.uint64(0x9E3779B97F4A7C15))) == 0x6E789E6AA1B965F4


@pytest.mark.parametrize("code", sorted(PD.ET_RECIPE))
def test_saturated_awgn_input_saturates_and_stops(code):
    """param_domain.et_input: at least 10 % of the bytes are +-127, and under
    OMS 4 / msg_max 63 some codewords stop within the host test's 4
    iterations and some do not stop at the same one."""
    llr = PD.et_input(code, HOST_BATCH)
    assert llr.dtype == np.int8 and llr.shape == (HOST_BATCH, load_table(code).n)
    assert (np.abs(llr.astype(np.int32)) == 127).mean() >= 0.10
    _, _, eit = PD.oracle_decode(code, ("et", HOST_BATCH), llr, PD.Params("OMS", 4, -127, 63), HOST_ITERS, early=True)
    assert eit.min() < HOST_ITERS and eit.max() > eit.min()


def test_grid_holds_the_required_points():
    have = {(p.algo, p.param if p.algo != "MS" else None, p.var_min, p.msg_max) for p in PD.GRID}
    for algo, param, msg_max in [("OMS", 0, 63), ("OMS", 63, 63), ("OMS", 31, 31), ("OMS", 32, 31), ("OMS", 5, 0),
                                 ("OMS", 0, 1), ("OMS", 1, 31), ("MS", None, 31), ("NMS", 0, 63), ("NMS", 1, 63),
                                 ("NMS", 32, 63), ("NMS", 33, 63), ("NMS", 64, 63), ("NMS", 64, 31), ("OMS", 3, 127),
                                 ("OMS", 64, 63), ("NMS", 65, 63), ("NMS", 255, 127)]:
        assert (algo, param, -127, msg_max) in have
    assert ("OMS", 1, -128, 31) in have and ("OMS", 1, -64, 31) in have
    assert len(set(PD.GRID)) == len(PD.GRID) and set(PD.SUBSET) <= set(PD.GRID)


@pytest.mark.parametrize("params", PD.GRID, ids=lambda p: p.id)
@pytest.mark.parametrize("code", REF_CODES)
def test_oracle_equals_reference(code, params):
    """16 frames (one call of the reference's 16-frame SSE decoder), 3
    iterations, the four full-range inputs: 0 differing hard decisions."""
    if not O.ref_available(code):
        pytest.skip("reference library for %s not built here" % code)
    n = load_table(code).n
    for kind in PD.INPUTS:
        llr = PD.make_input(kind, 16, n)
        exp = PD.ref_decode(code, llr, params, 3)
        got, _, _ = PD.oracle_on(code, kind, 16, params, 3)
        diff = int((got != exp).sum())
        assert diff == 0, "%s: %d hard decisions differ from the reference" % (kind, diff)


def _host_vs_oracle(code, params, early):
    """Fixed iterations: `u128`, `sat_flip` and `ties`.  Early termination:
    `ext` (the syndrome on -128, 0 and the saturations; it stops nowhere, so
    this is its fixed-iteration decode as well) and the saturated AWGN input
    of param_domain.et_input, on which codewords do stop (`sat_flip` for
    16200x7560, which has no recipe).  The oracle is most of the time spent,
    so each input goes through one of the two legs."""
    n = load_table(code).n
    d = host(code)
    for kind in (FIXED_INPUTS if not early else ("ext", "et" if code in PD.ET_RECIPE else "sat_flip")):
        llr = PD.et_input(code, HOST_BATCH) if kind == "et" else PD.make_input(kind, HOST_BATCH, n)
        exp, _, _ = PD.oracle_decode(code, (kind, HOST_BATCH), llr, params, HOST_ITERS, early)
        got = d.decode_i8(llr, HOST_ITERS, params.product(early_term=int(early)))
        assert d.last_kernel == "host"
        diff = int((got != exp).sum())
        assert diff == 0, "%s early=%d: %d hard decisions differ from the oracle" % (kind, early, diff)


@pytest.mark.parametrize("early", [False, True], ids=["fixed", "early"])
@pytest.mark.parametrize("params", PD.GRID, ids=lambda p: p.id)
@pytest.mark.parametrize("code", HOST_CODES)
def test_host_decoder_equals_oracle(code, params, early):
    """The host decoder's default path (AVX2 where the CPU has it): a ragged
    batch of 37 (one 32-lane block and a partial one), 4 iterations, fixed
    and with early termination."""
    _host_vs_oracle(code, params, early)


@pytest.mark.parametrize("env", [{"LDPC_HOST_PORTABLE": "1"}, {"LDPC_HOST_LANES": "16"}], ids=["portable", "sse16"])
@pytest.mark.parametrize("params", PD.SUBSET, ids=lambda p: p.id)
@pytest.mark.parametrize("code", ["dvbs2_r1_2", "dvbs2_r8_9", "16200x7560"])
def test_host_portable_paths_equal_oracle(code, params, env, monkeypatch):
    """The per-lane portable loop and the 16-lane SSE4.1 blocks on a subset
    of the grid."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    _host_vs_oracle(code, params, False)
