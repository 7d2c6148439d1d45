"""The CPU side of the float32 short-code tests (float_short_domain.py), on
which test_gpu_float_short.py rests:

* the coarse-grid inputs of every synthetic table hold the ties and zeros the
  min1 / min2 reductions are to meet (per table, floors 0.20 and 0.03);
* the oracle's serial float decode (oracle/ldpc_oracle.c oracle_decode_f32)
  equals an independent numpy float64 restatement (f32_ref.py) exactly under
  plain and offset min-sum, where nothing rounds; for normalised min-sum the
  oracle is the definition, as everywhere else;
* the product's host float decoder (device = -1) equals the oracle bit for bit
  on every table of both synthetic families;
* pins: float state fits kernel 7 at every (d, Z) of the degree sweep, which
  packed rows fit it and which shapes they give, and the conditions on the
  early-termination inputs, all on the oracle alone.
"""
import numpy as np
import pytest

import f32_ref as R
import float_domain as FD
import float_short_domain as FS
import ldsep_domain as ED
import oracle as O
import short_domain as SD
from ldpcgputegra_amd import Code, Decoder, default_params, load_table

TIES_FLOOR, ZEROS_FLOOR = 0.20, 0.03
REF_DEGREES = (2, 3, 7, 17, 31, 32)
REF_TABLES = [("short", d, Z) for Z in (SD.Z_SPLIT, SD.Z_LOOP) for d in REF_DEGREES] + \
             [("ep", d, rows, Z) for rows, Z in ED.SHAPES for d in (2, 8)]
ALL_TABLES = [("short", d, Z) for d, Z in FS.SHORT_TABLES] + [("ep",) + k for k in ED.ALL]
HOST_ALGOS = ("MS", "OMS0.5", "NMS0.75")


def table_of(key):
    """(Table, name, batch of the GPU file's inputs) of a ("short", d, Z) or ("ep", d, rows, Z) key"""
    if key[0] == "short":
        return FS.short_table(*key[1:]) + (FS.SWEEP_BATCH,)
    return FS.ep_table(*key[1:]) + (FS.EP_BATCH,)


def key_id(key):
    return table_of(key)[1]


def u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---- the inputs --------------------------------------------------------------

def test_inputs_are_what_they_say():
    t, name = FS.short_table(7, SD.Z_SPLIT)
    c = FS.make(t, name, 5, "coarse")
    assert c.dtype == np.float32 and c.shape == (5, t.n) and not c.flags.writeable
    assert FS.make(t, name, 5, "coarse") is c
    assert set(np.unique(c).tolist()) <= set(range(-4, 5)) and c.min() == -4 and (c == 0).any()
    assert not np.signbit(c[c == 0]).any() and c.mean() < -1.0
    # a smaller batch is a prefix of a larger one: the ldsep tests decode prefixes of one input
    assert np.array_equal(FS.make(t, name, 7, "coarse")[:5], c)
    z = FS.make(t, name, 5, "negzero")
    assert np.array_equal(z == 0, (c == 0) | (np.arange(t.n) % 7 == 0)[None, :]) and np.signbit(z[z == 0]).all()
    fine = FS.synthetic_input(t, name, 5, "fine")
    k = fine.astype(np.float64) / 0.5
    assert np.array_equal(k, np.rint(k)) and np.abs(k).max() == 16
    sub, big = FS.make(t, name, 5, "sub"), FS.make(t, name, 5, "big")
    assert ((sub == 0) == (fine == 0)).all() and (np.abs(sub[sub != 0]) < np.finfo(np.float32).tiny).all()
    assert np.array_equal(big.astype(np.float64) * 2.0 ** -100, fine)
    # the same recipe as float_domain's for a shipped table
    assert np.array_equal(FS.synthetic_input(load_table("648x324"), "648x324", 5), FD.make("648x324", 5, "coarse"))
    assert FS.beta_for("OMS0.5", "sub") == 0.5 * 2.0 ** -130 and FS.beta_for("NMS0.75", "coarse") == 0.75


@pytest.mark.parametrize("key", ALL_TABLES, ids=key_id)
def test_inputs_hold_ties_and_zeros(key):
    """float_domain.first_iteration_shares of the coarse input the GPU file
    decodes (5 codewords on the degree sweep, 7 on ldsep's tables): the share
    of checks whose two smallest |LLR| tie, and whose smallest is 0.  Measured
    minima over the tables: ties 0.289 (d = 7, Z = 12) and zeros 0.039 (d = 2,
    Z = 12) on the degree sweep, 0.259 and 0.123 on ldsep's; the fine grid
    gives 0.058 and 0.014 and is used for the scaled cases only."""
    t, name, batch = table_of(key)
    ties, zeros = FD.first_iteration_shares(t, FS.make(t, name, batch, "coarse"))
    print("%s: ties %.3f zeros %.3f" % (name, ties, zeros))
    assert ties >= TIES_FLOOR and zeros >= ZEROS_FLOOR, (ties, zeros)


# ---- the oracle against the float64 restatement ------------------------------

@pytest.mark.parametrize("algo", FS.EXACT_ALGOS)
@pytest.mark.parametrize("key", REF_TABLES, ids=key_id)
def test_oracle_equals_float64_restatement(key, algo):
    """3 iterations, and 8 with early termination, on the coarse input and on
    its -0.0 variant: hard decisions, soft output (as floats and bit for bit:
    the restatement negates a zero message where the oracle does) and
    iterations used."""
    t, name, batch = table_of(key)
    _, oalgo, beta = FS.ALGOS[algo]
    for kind in ("coarse", "negzero"):
        x = FS.make(t, name, batch, kind)
        for iters, early in ((FS.SWEEP_ITERS, False), (8, True)):
            exp = FS.oracle(t, name, batch, kind, algo, iters, early)
            got = R.decode(t, x, iters, R.NMS if oalgo == O.NMS else R.OMS, beta, early)
            where = "%s %s %s %d iterations early=%d" % (name, kind, algo, iters, early)
            assert np.array_equal(got[1], exp[1]) and np.array_equal(u32(got[1]), u32(exp[1])), where
            assert np.array_equal(got[0], exp[0]) and np.array_equal(got[2], exp[2]), where


def test_restatement_stops_codewords_apart():
    """The early-termination leg above is not vacuous: on a degree-8 ldsep
    table the restatement stops codewords at different iterations."""
    d, rows, Z = 8, 12, 27
    t, _ = FS.ep_table(d, rows, Z)
    got = R.decode(t, FS.ep_et_input(d, rows, Z), FS.EP_ET_ITERS, early=True)
    assert np.array_equal(got[2], FS.ep_et_oracle(d, rows, Z, "MS")[2]) and len(set(got[2].tolist())) >= 3
    assert (R.syndrome(t, got[0])[got[2] < FS.EP_ET_ITERS] == 0).all()


# ---- the host decoder against the oracle -------------------------------------

@pytest.mark.parametrize("key", ALL_TABLES, ids=key_id)
def test_host_float_decoder_vs_oracle(key):
    """Code(Table) on the host decoder, MS / OMS 0.5 / NMS 0.75, the coarse
    input and its -0.0 variant: the hard decisions of ldpc_decode_f32, and
    hard, soft (bit for bit) and iterations used of ldpc_decode_f32_soft, with
    and without early termination."""
    t, name, batch = table_of(key)
    dec = Decoder(Code(t), device=-1, max_batch=8)
    for algo in HOST_ALGOS:
        palgo, _, beta = FS.ALGOS[algo]
        for kind in ("coarse", "negzero"):
            x = FS.make(t, name, batch, kind)
            for iters, early in ((FS.SWEEP_ITERS, False), (8, True)):
                exp = FS.oracle(t, name, batch, kind, algo, iters, early)
                p = default_params(algo=palgo, beta=beta, early_term=int(early))
                where = "%s %s %s early=%d" % (name, kind, algo, early)
                assert np.array_equal(dec.decode_f32(x, iters, p), exp[0]), where
                hard, soft, its = dec.decode_f32_soft(x, iters, p)
                assert dec.last_kernel == "host"
                assert np.array_equal(hard, exp[0]) and np.array_equal(its, exp[2]), where
                assert np.array_equal(u32(soft), u32(exp[1])), "%s: %d soft values differ" % (
                    where, int((u32(soft) != u32(exp[1])).sum()))
    dec.close()


# ---- pins ---------------------------------------------------------------------

@pytest.mark.parametrize("d,Z", FS.SHORT_TABLES, ids=lambda v: str(v))
def test_float_state_fits_lds(d, Z):
    """lds_f32 of every table of the degree sweep against the literal
    NO_LDS_F32 the GPU file reads; the shape kernel 7 takes at the sweep's
    batch, restated."""
    info = Code(SD.synthetic(d, Z)).layer_info()
    assert (info["n_layers"], info["max_width"]) == (6, Z)
    assert info["lds_f32"] == ((d, Z) not in FS.NO_LDS_F32)
    assert SD.predicted_shape(Z, FS.SWEEP_BATCH) == (64, Z == SD.Z_SPLIT)


def test_ldsep_tables_are_taken_by_the_one_wave_kernel():
    """ldsep_domain.ALL: 28 tables in the two compiled shapes, none of them a
    table the several-wave form would take (ep_wide_info: no W)."""
    assert len(ED.ALL) == 28 and len(FS.SHORT_TABLES) == 62
    for d, rows, Z in ED.ALL:
        code = Code(ED.synthetic(d, rows, Z))
        info = code.layer_info()
        assert (info["n_layers"], info["max_width"]) == (rows, Z)
        assert code.ep_wide_info(FS.EP_BATCH)["waves"] == []
    assert sorted(b % 4 for b in FS.EP_BATCHES) == [0, 1, 1, 2, 3, 3] and max(FS.EP_BATCHES) == FS.EP_BATCH


def test_packed_rows_in_float():
    """Which packed rows kernel 7 takes in float, and their shapes."""
    for name, batch, lanes, split in FS.PACKED_F32:
        t = FS.packed_table(name)
        info = Code(t).layer_info()
        assert info["lds_f32"], name
        assert SD.predicted_shape(info["max_width"], batch) == (lanes, split), (name, batch)
        assert lanes < 64 and batch % (64 // lanes) != 0                             # a partly empty last wave
        assert SD.predicted_shape(info["max_width"], batch - 4)[0] == 2 * lanes      # the smallest batch of the shape
    for row in FS.PACKED_NO_F32:
        assert not Code(row[0]).layer_info()["lds_f32"], row
    assert sorted(FS.PACKED_F32_SHIPPED[:2] + FS.PACKED_NO_F32) == sorted(SD.PACKED)
    # shipped tables give (32, no split), (16, no split) and (32, split); every shape is there with the synthetic ones
    assert {r[2:] for r in FS.PACKED_F32_SHIPPED} == {(32, False), (16, False), (32, True)}
    assert {r[2:] for r in FS.PACKED_F32} == {(l, s) for l in (32, 16, 8) for s in (False, True)}
    for Z in (8, 4):      # the later group is of even degree: the split form runs with and without its padding lane
        assert SD.synthetic(FS.PACKED_SYN_D, Z).groups == [(7, 3 * Z), (6, 3 * Z)]


def test_packed_early_termination_input():
    """short_domain.et_conditions on the oracle's iterations used: a wave of
    two codewords that stop apart, a wave that stops, a wave that never does."""
    (name, batch, lanes, split), ebn0, iters = FS.PACKED_ET
    assert (name, batch, lanes, split) in FS.PACKED_F32 and split
    its = FS.packed_oracle(name, batch, "MS", iters, early=True, ebn0=ebn0)[2]
    print("%s @ %d: iterations used, codewords: %s" % (name, batch, np.bincount(its, minlength=iters + 1).tolist()))
    cond = SD.et_conditions(its, lanes, iters)
    assert all(cond.values()), cond


@pytest.mark.parametrize("key", sorted(FS.EP_ET), ids=lambda k: ED.synthetic_name(*k))
def test_ldsep_early_termination_inputs(key):
    """Within one workgroup of four codewords one stops early, one later and
    one never, under the algorithm float_short_domain.EP_ET names (and why)."""
    d, rows, Z = key
    assert d in FS.EP_ET_DEGREES and (rows, Z) in ED.SHAPES
    algo = FS.EP_ET[key][2]
    its = {a: FS.ep_et_oracle(d, rows, Z, a)[2] for a in HOST_ALGOS}
    print("%s: iterations used %s" % (ED.synthetic_name(*key), {a: v.tolist() for a, v in its.items()}))
    assert FS.ep_et_condition(its[algo]), its[algo].tolist()
    if d == 2:      # a forest of stars: plain min-sum always stops within two iterations, the stalled row stalls
        assert its["MS"].max() <= 2 and its["OMS0.5"][FS.EP_ET[key][3]] == FS.EP_ET_ITERS


def test_every_early_termination_table_is_listed():
    assert sorted(FS.EP_ET) == sorted((d, rows, Z) for rows, Z in ED.SHAPES for d in FS.EP_ET_DEGREES)


@pytest.mark.parametrize("key", ED.ALL, ids=lambda k: ED.synthetic_name(*k))
def test_ldsep_count_inputs_hold_errors(key):
    """The fused error count is compared on 2 and 3 codewords of the coarse
    input after 3 iterations of plain min-sum: some information bit is wrong
    in some codeword there, so the expected counts are not zero."""
    t, name = FS.ep_table(*key)
    hard = FS.oracle(t, name, FS.EP_BATCH, "coarse", "MS", FS.EP_ITERS)[0]
    for b in (2, 3):
        assert hard[:b, :t.k_info].sum() > 0
