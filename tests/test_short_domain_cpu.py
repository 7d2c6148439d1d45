"""The CPU side of the short-code domain tests (short_domain.py): the sixteen
plain .ldpc tables and the synthetic tables of every check degree 2 .. 32 on
the CPU checkers, over the full int8 LLR range and the parameter grid of
param_domain.py.

* the oracle against the reference's own SSE decoder (oracle/_ref, where it was
  built) on the five short codes it is built for -- four of them the two-group
  or degree-32 codes, where the later-group rule abs(min(c, msg_max)) covers
  most of the checks;
* the product's host decoder (device = -1) against the oracle on all sixteen
  tables and, through Code(Table), on the synthetic ones;
* the literals of short_domain.py (layer plans, packed launch shapes) against
  ldpc_code_layer_info and the launch rule restated once;
* the conditions the early-termination inputs must meet, on the oracle alone.

Every comparison is bit for bit.  test_gpu_short_domain.py rests on this file:
a mismatch it finds on the GPU is a kernel or dispatch bug, not a checker bug.
The host decoder's C-ABI entry returns hard decisions only; with early
termination a codeword's hard decisions freeze at the iteration it stops."""
import numpy as np
import pytest

import float_domain as FD
import oracle as O
import param_domain as PD
import short_domain as SD
from ldpcgputegra_amd import Code, Decoder, LdpcError, _lib, load_table
from ldpcgputegra_amd.codes import Table

REF_CODES = ["576x288", "1944x972", "2304x1152", "2048x384", "4000x2000"]
HOST_BATCH, HOST_ITERS = 37, 4
FIXED_INPUTS = ("u128", "sat_flip", "ties")
_decs = {}


def host(name, table=None):
    if name not in _decs:
        _decs[name] = Decoder(Code(table if table is not None else name), device=-1, max_batch=64)
    return _decs[name]


def test_inputs_are_what_they_say():
    """At the sizes used here: a batch of 32 codewords of the shortest code
    (6400 bytes) still holds every value of each input's range."""
    n = load_table("200x100").n
    u = PD.make_input("u128", 32, n)
    assert u.dtype == np.int8 and u.shape == (32, n) and len(np.unique(u)) == 256
    assert (np.abs(u.astype(np.int32)) > 31).mean() > 0.7                        # beyond channel.i8_table's range
    assert np.unique(PD.make_input("ext", 32, n)).tolist() == [-128, -127, -1, 0, 1, 127]
    t = PD.make_input("ties", 32, n)
    assert set(np.unique(t).tolist()) == {-127, 127} and 0.45 < (t == 127).mean() < 0.55
    s = PD.make_input("sat_flip", 32, n)
    assert set(np.unique(s).tolist()) == {-127, 127} and 0.02 < (s == 127).mean() < 0.06
    # the packed batches: the rows of the ragged last wave are no copies of earlier ones
    for code, batch, lanes, _ in SD.PACKED:
        x = PD.make_input("u128", batch, load_table(code).n)
        assert x.shape[0] % (64 // lanes) != 0
        assert not any(np.array_equal(x[-1], x[i]) for i in range(0, batch - 1, 997))


def test_tables_cover_the_shipped_codes():
    from ldpcgputegra_amd import codes
    shipped = [c for c in codes.available() if not c.startswith("dvbs2")]
    assert sorted(SD.SHORT_CODES) == sorted(shipped) and len(SD.SHORT_CODES) == 16
    assert set(SD.LAYER_PLAN) == set(SD.SHORT_CODES) == set(SD.KERNELS) == set(SD.AUTO)
    assert all(O.REF_CODE_DIRS.get(c) for c in REF_CODES)


@pytest.mark.parametrize("code", SD.SHORT_CODES)
def test_layer_plan(code):
    info = Code(code).layer_info()
    assert (info["n_layers"], info["max_width"]) == SD.LAYER_PLAN[code]
    assert info["lds_i8"] == (code in SD.LDS_CODES) == (7 in SD.KERNELS[code])
    preferred = info["lds_i8"] and load_table(code).m >= 8 * info["n_layers"]
    assert SD.AUTO[code] == ("lds" if preferred else "generic")


def test_packed_shapes_follow_from_the_layer_plans():
    """The literals of PACKED against the launch rule restated in
    short_domain.predicted_shape, and each batch the smallest with its shape."""
    assert len(set(SD.PACKED)) == len(SD.PACKED) == 9
    for code, batch, lanes, split in SD.PACKED:
        w = SD.LAYER_PLAN[code][1]
        assert SD.predicted_shape(w, batch) == (lanes, split), code
        assert lanes < 64 and batch % (64 // lanes) == 3 % (64 // lanes) != 0      # a partly empty last wave
        assert SD.predicted_shape(w, batch - 4)[0] == 2 * lanes, code      # one codeword fewer than the threshold
    # every combination of 2, 4, 8 codewords per wave with and without the split is there
    assert {(lanes, split) for _, _, lanes, split in SD.PACKED} == {(l, s) for l in (32, 16, 8) for s in (False, True)}
    # at a small batch: one codeword per wave, split iff 64 >= 2 * max_width
    for code in SD.LDS_CODES:
        w = SD.LAYER_PLAN[code][1]
        assert SD.predicted_shape(w, 32) == (64, w <= 32)
    assert {c for c in SD.LDS_CODES if SD.LAYER_PLAN[c][1] <= 32} == {"200x100", "648x324", "816x408", "1024x518",
                                                                       "1200x600"}


@pytest.mark.parametrize("Z", [SD.Z_SPLIT, SD.Z_LOOP])
@pytest.mark.parametrize("d", SD.DEGREES)
def test_synthetic_tables(d, Z):
    """Six layers of Z checks, the degrees d and max(2, d - 1), no variable
    twice in a check or in a layer; the table fits kernel 7's LDS."""
    t = SD.synthetic(d, Z)
    assert t.groups == [(d, 3 * Z), (max(2, d - 1), 3 * Z)] and t.n == 32 * Z and t.m == 6 * Z
    pos = 0
    for r in range(6):
        deg = t.groups[r // 3][0]
        layer = t.edge_var[pos:pos + deg * Z]
        pos += deg * Z
        assert len(np.unique(layer)) == deg * Z
    info = Code(t).layer_info()
    assert (info["n_layers"], info["max_width"], info["lds_i8"]) == (6, Z, True)
    assert SD.predicted_shape(Z, 32) == (64, Z == SD.Z_SPLIT)
    assert SD.synthetic(d, Z) is t


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


def _host_vs_oracle(name, params, early, table=None, fixed=FIXED_INPUTS):
    """As test_param_domain_cpu._host_vs_oracle.  Fixed iterations: `u128`,
    `sat_flip` and `ties`.  Early termination: `ext` (the syndrome on -128, 0
    and the saturations) and the saturated AWGN input of short_domain.et_input,
    on which codewords do stop (`sat_flip` for a code without a recipe)."""
    t = table if table is not None else load_table(name)
    d = host(name, table)
    for kind in (fixed if not early else ("ext", "et" if name in SD.ET_RECIPE else "sat_flip")):
        llr = SD.et_input(name, HOST_BATCH) if kind == "et" else PD.make_input(kind, HOST_BATCH, t.n)
        exp, _, _ = PD.oracle_decode(name, (kind, HOST_BATCH), llr, params, HOST_ITERS, early, table=t)
        got = d.decode_i8(llr, HOST_ITERS, params.product(early_term=int(early)))
        assert d.last_kernel == "host" and d.last_lds_shape == (0, False)
        diff = int((got != exp).sum())
        assert diff == 0, "%s early=%d: %d hard decisions differ from the oracle" % (kind, early, diff)


def _host_grid():
    return [(c, p) for c in SD.LDS_CODES for p in PD.GRID] + [(c, p) for c in SD.GENERIC_ONLY for p in PD.SUBSET]


@pytest.mark.parametrize("early", [False, True], ids=["fixed", "early"])
@pytest.mark.parametrize("code,params", _host_grid(), ids=lambda v: v if isinstance(v, str) else v.id)
def test_host_decoder_equals_oracle(code, params, early):
    """The host decoder's default path on every shipped short table: a ragged
    batch of 37, 4 iterations, fixed and with early termination."""
    _host_vs_oracle(code, params, early)


@pytest.mark.parametrize("env", [{"LDPC_HOST_PORTABLE": "1"}, {"LDPC_HOST_LANES": "16"}], ids=["portable", "sse16"])
@pytest.mark.parametrize("params", PD.SUBSET, ids=lambda p: p.id)
@pytest.mark.parametrize("code", ["648x324", "1200x600", "2048x384"])
def test_host_portable_paths_equal_oracle(code, params, env, monkeypatch):
    """The per-lane portable loop and the 16-lane SSE4.1 blocks: a two-group
    code whose later group is most of it, the narrowest layers, degree 32."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    _host_vs_oracle(code, params, False)


@pytest.mark.parametrize("early", [False, True], ids=["fixed", "early"])
@pytest.mark.parametrize("d", SD.DEGREES)
def test_host_decoder_on_synthetic_tables(d, early):
    """Code(Table) through ldpc_code_create, every check degree 2 .. 32 (and
    d - 1 in the later group): check_dispatch's case 3 and its runtime-degree
    path, which no shipped code reaches."""
    t = SD.synthetic(d, SD.Z_SPLIT)
    for params in SD.SWEEP_PARAMS:
        _host_vs_oracle(SD.synthetic_name(d, SD.Z_SPLIT), params, early, table=t, fixed=SD.SWEEP_INPUTS)


def test_degree_bound():
    """ldpc_code_create takes a check of degree 33 (degrees up to 64 are a
    valid table); a decoder context refuses it: the kernels and the host
    decoder are built for degrees up to 32."""
    t = Table(40, 2, [(32, 1), (33, 1)], np.concatenate([np.arange(32), np.arange(7, 40)]).astype(np.uint32))
    code = Code(t)
    assert code.max_deg == 33
    with pytest.raises(LdpcError) as e:
        Decoder(code, device=-1, max_batch=64)
    assert e.value.status == _lib.LDPC_EUNSUPPORTED and "check degree" in str(e.value)
    ok = Decoder(Code(Table(40, 1, [(32, 1)], np.arange(32, dtype=np.uint32))), device=-1, max_batch=64)
    assert ok.decode_i8(np.full((1, 40), -5, dtype=np.int8), 1).sum() == 0


@pytest.mark.parametrize("code", sorted(SD.ET_RECIPE))
def test_early_termination_inputs_saturate_and_stop(code):
    """short_domain.et_input, 64 codewords of either recipe: at least 10 % of
    the bytes are +-127; under either parameter set some codewords stop
    before the last of the 8 iterations and some do not."""
    for which in SD.ET_PARAMS:
        llr = SD.et_input(code, 64, which)
        assert llr.dtype == np.int8 and llr.shape == (64, load_table(code).n)
        assert (np.abs(llr.astype(np.int32)) == 127).mean() >= 0.10
        for params in SD.ET_PARAMS:
            _, _, eit = PD.oracle_decode(code, ("short_et", 64, which.id), llr, params, SD.ET_ITERS, early=True)
            assert eit.min() < SD.ET_ITERS and eit.max() == SD.ET_ITERS, (which.id, params.id, eit.tolist())


@pytest.mark.parametrize("params", SD.ET_PARAMS, ids=lambda p: p.id)
@pytest.mark.parametrize("row", SD.ET_ROWS, ids=SD.packed_id)
def test_early_termination_inputs_fill_the_packed_waves(row, params):
    """At the packed row's batch, with 64 / lanes consecutive codewords to a
    wave: some wave holds two different iters_used (`live` differs inside a
    wave, the syndrome ballot needs its per-codeword mask), some wave stops
    entirely before the last iteration (the wave-wide break), some never."""
    code, batch, lanes, _ = row
    llr = SD.et_input(code, batch, params)
    assert (np.abs(llr.astype(np.int32)) == 127).mean() >= 0.10
    _, _, eit = PD.oracle_decode(code, ("short_et", batch, params.id), llr, params, SD.ET_ITERS, early=True)
    cond = SD.et_conditions(eit, lanes, SD.ET_ITERS)
    assert all(cond.values()), cond


@pytest.mark.parametrize("row", SD.ET_ROWS_F32, ids=SD.packed_id)
def test_float_early_termination_inputs_fill_the_packed_waves(row):
    """The same conditions for the float leg: float_domain's "fine" input,
    plain min-sum, 8 iterations."""
    code, batch, lanes, _ = row
    _, _, eit = FD.oracle_on(code, batch, "fine", O.OMS, 0.0, SD.ET_ITERS_F32, early=True)
    cond = SD.et_conditions(eit, lanes, SD.ET_ITERS_F32)
    assert all(cond.values()), cond
