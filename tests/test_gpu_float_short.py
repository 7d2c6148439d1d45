"""The float32 min-sum kernels of the short codes -- generic (1), lds (7) and
ldsep (9) -- at every check degree and launch shape they are built for, forced
one by one, against the oracle's serial float decode (oracle/ldpc_oracle.c
oracle_decode_f32).  The shipped tables that test_gpu_float_domain.py runs hold
check degrees 6, 7 and 8 only; the float code paths share nothing with the
int8 ones that test_gpu_short_domain.py sweeps.

The comparison is test_gpu_float_domain.assert_same on dyadic-grid inputs
(float_short_domain.py), where nothing rounds under plain and offset min-sum and
equality is the tolerance: generic and lds bit for bit, the sign of a zero
included; ldsep equal to the oracle as floats and bit for bit equal to the
oracle on the input + 0.0.  Under NMS 0.75 the kernels do the oracle's
operations on the oracle's operands, so the same holds.
test_float_short_cpu.py holds the oracle to a float64 restatement and the host
decoder to the oracle on the same tables and inputs, and pins the shapes.

* the degree sweep: short_domain.synthetic(d, Z), d = 2 .. 32; Z = 12 is two
  lanes per check on kernel 7 (lds_check_f32_split, with its padding lane at
  odd d), Z = 40 one lane per check; MS, OMS 0.5, OMS 4.0 and NMS 0.75; the
  coarse grid, -0.0 (after one iteration too, where the output still holds
  -0.0), and at d = 2, 3, 17, 32 the fine grid scaled into the subnormals and
  to 2^100; batch 5, 3 iterations, guard rows behind every output;
* kernel 7's packed shapes in float: 2, 4 and 8 codewords per wave, with and
  without the split, the last wave partly empty, and early termination with two
  codewords to a wave;
* ldsep on ldsep_domain.ALL: check degrees 2 .. 8 (up to six padding lanes per
  check, both parities of their number), one exactly full pass, a last pass of
  three checks and of one, four full passes; every tail of the 4-codeword
  workgroup; early termination with codewords of one workgroup stopping apart;
  the fused error count with waves past the batch."""
import numpy as np
import pytest

import float_short_domain as FS
import ldsep_domain as ED
import short_domain as SD
from ldpcgputegra_amd import Code, Decoder, default_params
from test_gpu_float_domain import assert_same

pytestmark = pytest.mark.gpu

HARD_FILL, SOFT_FILL, ITS_FILL = 9, 99.0, -7
SWEEP_ALGOS = ("MS", "OMS0.5", "OMS4", "NMS0.75")
SCALED_ALGOS = ("MS", "OMS0.5")      # on the scaled inputs the offset is scaled like the input; NMS would round there
EP_ALGOS = ("MS", "OMS0.5", "NMS0.75")


def _torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def run(dec, x, iters, params, extra=2):
    """(hard, soft, iters_used) of one device decode of the host array x, with `extra` guard rows behind every output"""
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


def params_of(algo, kind="coarse", early=False):
    return default_params(algo=FS.ALGOS[algo][0], beta=FS.beta_for(algo, kind), early_term=int(early))


# ---- families 1 and 7: every check degree ------------------------------------------

def sweep_cases(d):
    """(kind, iterations, algorithms) of one table of the degree sweep"""
    cases = [("coarse", FS.SWEEP_ITERS, SWEEP_ALGOS), ("negzero", FS.SWEEP_ITERS, SWEEP_ALGOS),
             ("negzero", 1, SWEEP_ALGOS)]
    if d in FS.SCALED_DEGREES:
        cases += [("sub", FS.SWEEP_ITERS, SCALED_ALGOS), ("big", FS.SWEEP_ITERS, SCALED_ALGOS)]
    return cases


@pytest.mark.parametrize("Z", [SD.Z_SPLIT, SD.Z_LOOP])
@pytest.mark.parametrize("d", SD.DEGREES)
def test_degree_sweep(d, Z):
    """Every instance of LDPC_DEG_CASES (generic) and LDPC_LDS_DEG_CASES (lds)
    in float: check degree d in the first three layers and max(2, d - 1) in the
    last three.  Z = 12: lds_check_f32_split, lanes 24 .. 63 idle; Z = 40:
    lds_check_f32, lanes 40 .. 63 idle."""
    t, name = FS.short_table(d, Z)
    kernels = (1,) if (d, Z) in FS.NO_LDS_F32 else (1, 7)
    decs = {k: Decoder(Code(t), max_batch=8, kernel=k) for k in kernels}
    for kind, iters, algos in sweep_cases(d):
        x = FS.make(t, name, FS.SWEEP_BATCH, kind)
        for algo in algos:
            exp = FS.oracle(t, name, FS.SWEEP_BATCH, kind, algo, iters)
            if kind == "negzero" and iters == 1:      # this is where a sign-bit test would differ from c < 0
                assert np.signbit(exp[1][exp[1] == 0]).any()
            if kind == "sub":                         # subnormals are kept: the soft output holds them
                assert ((exp[1] != 0) & (np.abs(exp[1]) < np.finfo(np.float32).tiny)).any()
            for k, dec in decs.items():
                got = run(dec, x, iters, params_of(algo, kind))
                where = "%s %s %s %d iterations kernel %d" % (name, kind, algo, iters, k)
                assert dec.last_kernel == Decoder.KERNEL_NAMES[k], where
                assert dec.last_lds_shape == ((64, Z == SD.Z_SPLIT) if k == 7 else (0, False)), where
                assert_same(got, exp, where, bitwise=True)
    for dec in decs.values():
        dec.close()


# ---- family 7: the packed launch shapes ----------------------------------------------

def packed_id(row):
    return "%s_b%d_l%d%s" % (row[0], row[1], row[2], "s" if row[3] else "")


@pytest.mark.parametrize("row", FS.PACKED_F32, ids=packed_id)
def test_packed_shapes_vs_oracle(row):
    """Kernel 7 in float with 2, 4 and 8 codewords per wave, split and not, on
    the fine grid: the launch took the row's shape; every codeword, those of the
    partly empty last wave included, equals the oracle's; the rows beyond the
    batch keep their sentinel."""
    name, batch, lanes, split = row
    dec = Decoder(Code(FS.packed_table(name)), max_batch=batch, kernel=7)
    x = FS.packed_input(name, batch)
    for algo in FS.PACKED_ALGOS:
        exp = FS.packed_oracle(name, batch, algo)
        got = run(dec, x, FS.PACKED_ITERS, params_of(algo), extra=64 // lanes)
        where = "%s batch %d %s" % (name, batch, algo)
        assert dec.last_kernel == "lds" and dec.last_lds_shape == (lanes, split), (where, dec.last_lds_shape)
        assert_same(got, exp, where, bitwise=True)
    dec.close()


def test_packed_split_early_termination():
    """Two codewords to a wave, two lanes per check, early termination: the
    syndrome ballot masked per codeword, `live` differing inside a wave, the
    wave-wide break (the conditions are test_float_short_cpu.py's)."""
    (name, batch, lanes, split), ebn0, iters = FS.PACKED_ET
    exp = FS.packed_oracle(name, batch, "MS", iters, early=True, ebn0=ebn0)
    assert all(SD.et_conditions(exp[2], lanes, iters).values())
    dec = Decoder(Code(name), max_batch=batch, kernel=7)
    got = run(dec, FS.packed_input(name, batch, ebn0), iters, params_of("MS", early=True), extra=64 // lanes)
    assert dec.last_kernel == "lds" and dec.last_lds_shape == (lanes, split), dec.last_lds_shape
    assert_same(got, exp, "%s batch %d early termination" % (name, batch), bitwise=True)
    dec.close()


# ---- family 9: the one-wave edge-parallel kernel --------------------------------------

def ep_decoder(t):
    """every switch off: family 9 is the float32 one-wave kernel"""
    dec = Decoder(Code(t), max_batch=8, kernel=9)
    assert not (dec.ep_wide or dec.f16_edge_parallel or dec.i8_edge_parallel or dec.f16_all_codes)
    return dec


def ep_compare(dec, x, exp, exp_pos, algo, kind, iters, where, early=False):
    """decode x[:b] for every b of EP_BATCHES and hold it to the oracle on x and on x + 0.0"""
    params = params_of(algo, kind, early)
    for b in FS.EP_BATCHES:
        got = run(dec, x[:b], iters, params)
        w = "%s batch %d" % (where, b)
        assert dec.last_kernel == "ldsep" and dec.last_ep_waves == 0 and dec.last_lds_shape == (0, False), w
        assert_same(got, tuple(a[:b] for a in exp), w, bitwise=False)
        assert_same(got, tuple(a[:b] for a in exp_pos), w + " vs the oracle on the input + 0.0", bitwise=True)


@pytest.mark.parametrize("d,rows,Z", ED.ALL, ids=[ED.synthetic_name(*k) for k in ED.ALL])
def test_ldsep_tables(d, rows, Z):
    """ldsep_decode<12, 4, *> and <11, 6, *>: 8 - d padding lanes per check on
    the sink V[N] (d - 1 in the later rows: both parities in every table), the
    empty check slots of Z = 8, 27 and 41 on V[N + 1]; batches 1 .. 5 and 7
    as prefixes of one input."""
    t, name = FS.ep_table(d, rows, Z)
    dec = ep_decoder(t)
    cases = [("coarse", FS.EP_ITERS, EP_ALGOS), ("negzero", FS.EP_ITERS, EP_ALGOS), ("negzero", 1, EP_ALGOS)]
    if d in FS.EP_SCALED_DEGREES:
        cases += [("sub", FS.EP_ITERS, SCALED_ALGOS), ("big", FS.EP_ITERS, SCALED_ALGOS)]
    for kind, iters, algos in cases:
        x = FS.make(t, name, FS.EP_BATCH, kind)
        for algo in algos:
            exp = exp_pos = FS.oracle(t, name, FS.EP_BATCH, kind, algo, iters)
            if kind == "negzero":
                exp_pos = FS.oracle(t, name, FS.EP_BATCH, kind, algo, iters, plus_zero=True)
                assert iters > 1 or np.signbit(exp[1][exp[1] == 0]).any()
            ep_compare(dec, x, exp, exp_pos, algo, kind, iters, "%s %s %s %d iterations" % (name, kind, algo, iters))
    dec.close()


@pytest.mark.parametrize("d,rows,Z", sorted(FS.EP_ET), ids=[ED.synthetic_name(*k) for k in sorted(FS.EP_ET)])
def test_ldsep_early_termination(d, rows, Z):
    """The inputs of float_short_domain.EP_ET: in one workgroup a codeword
    stops early, one later and one never (under the algorithm named there;
    test_float_short_cpu.py).  The syndrome reads the sinks as -inf: never 1."""
    t, name = FS.ep_table(d, rows, Z)
    x = FS.ep_et_input(d, rows, Z)
    assert FS.ep_et_condition(FS.ep_et_oracle(d, rows, Z, FS.EP_ET[(d, rows, Z)][2])[2])
    dec = ep_decoder(t)
    for algo in EP_ALGOS:
        exp = FS.ep_et_oracle(d, rows, Z, algo)
        ep_compare(dec, x, exp, exp, algo, "coarse", FS.EP_ET_ITERS, "%s early termination %s" % (name, algo),
                   early=True)
    dec.close()


@pytest.mark.parametrize("d,rows,Z", ED.ALL, ids=[ED.synthetic_name(*k) for k in ED.ALL])
def test_ldsep_fused_error_count(d, rows, Z, monkeypatch):
    """ldpc_decode_f32_count_async at batches 2 and 3: the waves past the
    batch skip the decode and stay for the workgroup's reduction.  Against
    numpy on the oracle's hard decisions, with and without a reference
    codeword array, the counters accumulating."""
    torch = _torch()
    monkeypatch.setenv("LDPC_FUSED_COUNT", "1")
    t, name = FS.ep_table(d, rows, Z)
    k = t.k_info
    x = FS.make(t, name, FS.EP_BATCH, "coarse")
    exp = FS.oracle(t, name, FS.EP_BATCH, "coarse", "MS", FS.EP_ITERS)
    ref = np.zeros((FS.EP_BATCH, t.n), dtype=np.uint8)
    ref[:, ::5] = 1
    dec = ep_decoder(t)
    counts = torch.zeros(2, dtype=torch.int64, device="cuda")
    want = np.zeros(2, dtype=np.int64)
    for b in (2, 3):
        for r in (None, ref):
            hard = torch.full((b + 2, t.n), HARD_FILL, dtype=torch.uint8, device="cuda")
            d_ref = None if r is None else torch.from_numpy(r[:b].copy()).cuda()
            dec.decode_count_device(torch.from_numpy(np.array(x[:b])).cuda(), hard, FS.EP_ITERS, k, counts, ref=d_ref,
                                    params=params_of("MS"))
            torch.cuda.synchronize()
            assert dec.last_kernel == "ldsep" and dec.last_ep_waves == 0
            h = hard.cpu().numpy()
            assert np.array_equal(h[:b], exp[0][:b]) and (h[b:] == HARD_FILL).all()
            diff = exp[0][:b, :k] ^ (0 if r is None else r[:b, :k])
            want += (int(diff.sum()), int(diff.any(axis=1).sum()))
            assert want[0] > 0
            assert counts.cpu().numpy().tolist() == want.tolist(), (name, b, r is None)
    dec.close()
