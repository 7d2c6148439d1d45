"""The edge-parallel int8 kernel over several waves on the GPU (`ldsepwi`: family
9 of the int8 decode on the longer QC codes, behind the i8_ep_wide switch)
against oracle.decode_i8, which test_i8_ep_wide_cpu.py ties to the host decoder
on the same tables and parameters.  "Equal" is always hard decisions, int8 soft
output and iters_used with zero differing elements, and guard rows behind every
output keep their fill.

* the synthetic tables of test_ep_wide_cpu.SYNTHETIC (ragged, idle and full
  waves; a last pass of four checks and of one; the largest Z) at check degrees
  2, 5 and 8 (six padding lanes; the odd flip; none), every compiled W forced by
  LDPC_EPW_WAVES, OMS 1 / MS / NMS 26 at batches 1 (a lone half), 2 and 5, 3
  iterations, full-range input with raw -128;
* the corners of the parameter domain (tests/test_gpu_i8_ep.py's) on the
  (12, 88) and (11, 105) tables;
* 1944x972, 1248x624 and 2304x1152 at every compiled W, 6 iterations, batch 5;
* the reference's golden vectors of 1944x972 and 2304x1152, through both
  host-buffer entry points; var_min = -128 falls back to family 7;
* early termination per half and per workgroup on the inputs
  test_i8_ep_wide_cpu fixes, at every W, the three algorithms, and batch 1;
* 0 iterations, an empty batch, 1-byte aligned slices of an odd batch,
  node-major input, the error counter;
* the switch off (the parent's answers) and on (the selection table of
  DESIGN.md section 7, row by row), alone and with every other switch on;
* a 648x324 decoder on `ldsepi` and a 1944x972 decoder on `ldsepwi` used alternately."""
import ctypes as C

import numpy as np
import pytest

import ldsep_domain as ED
import param_domain as PD
import struct_domain as ST
import test_i8_ep_wide_cpu as IW
from conftest import golden_cases, golden_inputs
from ldpcgputegra_amd import ALGO_BP, ALGO_MS, ALGO_NMS, ALGO_OMS, Code, Decoder, LdpcError, _lib, channel, \
    default_params, load_table

pytestmark = pytest.mark.gpu

BASIC = IW.BASIC
SYN_BATCHES = (1, 2, IW.SYN_BATCH)
SHIP_BATCH, SHIP_ITERS = 5, 6
SOFT_FILL, HARD_FILL, ITS_FILL = 0x55, 9, -7
GOLDEN = [c for c in golden_cases() if c["code"] in ("1944x972", "2304x1152")]


def _torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def _table(name):
    return ED.synthetic(*name) if isinstance(name, tuple) else load_table(name)


def _name(name):
    return ED.synthetic_name(*name) if isinstance(name, tuple) else name


def oracle_ref(name, key, x, p, iters, early=False):
    """(hard, soft, iters_used) of the oracle, computed once per case and read-only"""
    return PD.oracle_decode(_name(name), key, x, p, iters, early=early, table=_table(name))


def rows_of(ref, batch):
    return tuple(a[:batch] for a in ref)


def as_device(x):
    return _torch().from_numpy(np.array(x)).cuda()


def assert_ldsepwi(dec, w=None):
    assert dec.last_kernel == "ldsep" and dec.last_skipped is None
    assert dec.last_lds_shape == (0, False) and dec.last_et_stage == 0
    assert dec.last_ep_waves in ((2, 4) if w is None else (w,)), (dec.last_ep_waves, w)


def run_i8(dec, d_llr, iters, params, w=None, extra=2):
    """decode_i8_device with guard rows behind every output; asserts the launch was ldsepwi (on w waves)"""
    torch = _torch()
    B, n = d_llr.shape
    d_hard = torch.full((B + extra, n), HARD_FILL, dtype=torch.uint8, device="cuda")
    d_soft = torch.full((B + extra, n), SOFT_FILL, dtype=torch.int8, device="cuda")
    d_its = torch.full((B + extra,), ITS_FILL, dtype=torch.int32, device="cuda")
    dec.decode_i8_device(d_llr, d_hard, iters, params=params, soft=d_soft, iters_used=d_its)
    torch.cuda.synchronize()
    assert_ldsepwi(dec, w)
    hard, soft, its = d_hard.cpu().numpy(), d_soft.cpu().numpy(), d_its.cpu().numpy()
    assert (hard[B:] == HARD_FILL).all() and (soft[B:] == SOFT_FILL).all() and (its[B:] == ITS_FILL).all(), \
        "rows beyond the batch written"
    return hard[:B], soft[:B], its[:B]


def assert_equal(got, exp, where):
    for g, e, what in zip(got, exp, ("hard", "soft", "iters_used")):
        assert g.dtype == e.dtype and g.shape == e.shape, (where, what, g.dtype, e.dtype, g.shape, e.shape)
        bad = np.flatnonzero((g != e).ravel())
        assert bad.size == 0, "%s: %s differs in %d of %d places, first at %d: %r vs %r" % (
            where, what, bad.size, g.size, bad[0], g.ravel()[bad[0]], e.ravel()[bad[0]])


def _status(fn):
    with pytest.raises(LdpcError) as e:
        fn()
    return e.value.status, str(e.value)


# ---- synthetic tables -------------------------------------------------------------

SYN_CASES = [(d, rows, Z) for rows, Z in sorted(IW.SYNTHETIC) for d in IW.DEGREES]


@pytest.mark.parametrize("d,rows,Z", SYN_CASES, ids=[ED.synthetic_name(*k) for k in SYN_CASES])
def test_synthetic_tables(d, rows, Z, monkeypatch):
    name = (d, rows, Z)
    t = ED.synthetic(*name)
    x = PD.make_input("u128", IW.SYN_BATCH, t.n)
    assert (x == -128).any()
    dev = as_device(x)
    dec = Decoder(Code(t), max_batch=8, kernel=9, i8_ep_wide=True)
    assert dec.i8_ep_wide is True and dec.ep_wide is False and dec.i8_edge_parallel is False
    for w in IW.SYNTHETIC[(rows, Z)][1]:
        monkeypatch.setenv("LDPC_EPW_WAVES", str(w))
        for p in BASIC:
            exp = oracle_ref(name, ("u128", IW.SYN_BATCH), x, p, IW.SYN_ITERS)
            for batch in SYN_BATCHES:
                got = run_i8(dec, dev[:batch], IW.SYN_ITERS, p.product(), w)
                assert_equal(got, rows_of(exp, batch), "%s W %d %s batch %d" % (_name(name), w, p.id, batch))
    dec.close()


CORNER_CASES = [(d, rows, Z) for rows, Z in IW.CORNER_TABLES for d in IW.DEGREES]


@pytest.mark.parametrize("d,rows,Z", CORNER_CASES, ids=[ED.synthetic_name(*k) for k in CORNER_CASES])
def test_parameter_corners(d, rows, Z, monkeypatch):
    """var_min = -64 and 0 are where the padding lanes show (tests/test_gpu_i8_ep.py); degree 2 has six padding
    lanes per check, Z = 105 a last pass of one check, half of each table uses the later-group rule."""
    import test_gpu_i8_ep
    assert IW.CORNERS == test_gpu_i8_ep.CORNERS
    name = (d, rows, Z)
    t = ED.synthetic(*name)
    dec = Decoder(Code(t), max_batch=8, kernel=9, i8_ep_wide=True)
    for kind in ("ext", "ties"):
        x = PD.make_input(kind, IW.SYN_BATCH, t.n)
        dev = as_device(x)
        for w in IW.SYNTHETIC[(rows, Z)][1]:
            monkeypatch.setenv("LDPC_EPW_WAVES", str(w))
            for p in IW.CORNERS:
                exp = oracle_ref(name, (kind, IW.SYN_BATCH), x, p, IW.SYN_ITERS)
                for batch in SYN_BATCHES:
                    got = run_i8(dec, dev[:batch], IW.SYN_ITERS, p.product(), w)
                    assert_equal(got, rows_of(exp, batch), "%s %s W %d %s batch %d" % (_name(name), kind, w, p.id, batch))
    dec.close()


# ---- the shipped tables -----------------------------------------------------------

def awgn_input(name, batch, ebn0=1.5):
    t = load_table(name)
    return channel.awgn_i8_host(t.n, batch, seed=1, table=channel.i8_table(channel.sigma_from_ebn0(ebn0, t.k_info / t.n)))


@pytest.mark.parametrize("name", sorted(IW.SHIPPED))
def test_shipped_tables(name, monkeypatch):
    t = load_table(name)
    dec = Decoder(Code(name), max_batch=8, kernel=9, i8_ep_wide=True)
    for w in IW.SHIPPED[name][2]:
        monkeypatch.setenv("LDPC_EPW_WAVES", str(w))
        for key, x in (("u128", PD.make_input("u128", SHIP_BATCH, t.n)), ("awgn15", awgn_input(name, SHIP_BATCH))):
            dev = as_device(x)
            for p in BASIC:
                got = run_i8(dec, dev, SHIP_ITERS, p.product(), w)
                assert_equal(got, oracle_ref(name, (key, SHIP_BATCH), x, p, SHIP_ITERS), "%s W %d %s %s" % (name, w, key, p.id))
    dec.close()


@pytest.mark.parametrize("case", GOLDEN, ids=[c["name"] for c in GOLDEN])
def test_golden_cases(case, monkeypatch):
    """The reference's recorded hard decisions, through the two host-buffer entry points"""
    monkeypatch.delenv("LDPC_EPW_WAVES", raising=False)
    assert len([c for c in GOLDEN if c["code"] == "1944x972"]) == 28
    assert len([c for c in GOLDEN if c["code"] == "2304x1152"]) >= 4
    llr, hard = golden_inputs(case)
    algo = {0: ALGO_OMS, 1: ALGO_NMS}[case["algo"]]
    p = default_params(algo=algo, offset=case["param"], factor=case["param"], var_min=case["var_min"],
                       msg_max=case["msg_max"], msg_min=-case["msg_max"])
    dec = Decoder(Code(case["code"]), max_batch=case["batch"], i8_ep_wide=True)
    auto = Code(case["code"]).i8_ep_wide_info(case["batch"])["waves_auto"]
    got = dec.decode_i8(llr, case["iters"], p)
    if case["var_min"] < -127:      # outside the kernel's domain: the parent's choice, which says what it passed over
        assert case["name"] == "1944x972_stress128_vmin128_it10"
        assert dec.last_kernel == "lds" and dec.last_skipped == "ldsep" and dec.last_ep_waves == 0
    elif auto:
        assert_ldsepwi(dec, auto)
    else:                           # the rule hands this batch back
        assert dec.last_kernel == "lds" and dec.last_skipped is None and dec.last_ep_waves == 0
    assert np.array_equal(got, hard), case["name"]
    dec.set_kernel(9)
    if case["var_min"] < -127:
        st, msg = _status(lambda: dec.decode_i8(llr, case["iters"], p))
        assert st == _lib.LDPC_EUNSUPPORTED and "not applicable" in msg, msg
    else:
        for w in IW.SHIPPED[case["code"]][2]:
            monkeypatch.setenv("LDPC_EPW_WAVES", str(w))
            assert np.array_equal(dec.decode_i8(llr, case["iters"], p), hard), (case["name"], w)
            assert_ldsepwi(dec, w)
            out = np.zeros_like(hard)
            dec.decode_i8_host_async(np.ascontiguousarray(llr), out, case["iters"], p)
            dec.synchronize()
            assert_ldsepwi(dec, w)
            assert np.array_equal(out, hard), (case["name"], w)
    dec.close()


# ---- early termination ------------------------------------------------------------

@pytest.mark.parametrize("code", sorted(IW.ET_POINT))
def test_early_termination(code, monkeypatch):
    torch = _torch()
    x = IW.et_input(code)
    dev = as_device(x)
    dec = Decoder(Code(code), max_batch=16, kernel=9, i8_ep_wide=True)
    for w in IW.SHIPPED[code][2]:
        monkeypatch.setenv("LDPC_EPW_WAVES", str(w))
        for algo in sorted(IW.ET_PARAMS):
            p = IW.ET_PARAMS[algo]
            exp = IW.et_oracle(code, algo)
            assert exp[2].tolist() == IW.ET_ITERS_USED[code][algo]
            for batch in (IW.ET_BATCH, IW.ET_BATCH - 1, 1):      # a lone last half; none; a lone half alone
                got = run_i8(dec, dev[:batch], IW.ET_ITERS, p.product(early_term=1), w)
                assert_equal(got, rows_of(exp, batch), "%s early termination %s W %d batch %d" % (code, algo, w, batch))
            # no iters_used array
            hard = torch.full((IW.ET_BATCH, x.shape[1]), HARD_FILL, dtype=torch.uint8, device="cuda")
            soft = torch.full((IW.ET_BATCH, x.shape[1]), SOFT_FILL, dtype=torch.int8, device="cuda")
            dec.decode_i8_device(dev, hard, IW.ET_ITERS, params=p.product(early_term=1), soft=soft)
            torch.cuda.synchronize()
            assert_ldsepwi(dec, w)
            assert np.array_equal(hard.cpu().numpy(), exp[0]) and np.array_equal(soft.cpu().numpy(), exp[1])
    dec.close()


def test_zero_iterations_and_empty_batch(monkeypatch):
    name = "1944x972"
    t = load_table(name)
    x = PD.make_input("ext", 5, t.n)      # raw -128 LLRs among them
    dec = Decoder(Code(name), max_batch=8, kernel=9, i8_ep_wide=True)
    for w in IW.SHIPPED[name][2]:
        monkeypatch.setenv("LDPC_EPW_WAVES", str(w))
        for early in (False, True):
            hard, soft, its = run_i8(dec, as_device(x), 0, default_params(early_term=int(early)), w)
            assert np.array_equal(soft, x) and np.array_equal(hard, (x > 0).astype(np.uint8)) and not its.any()
            assert_equal((hard, soft, its), oracle_ref(name, ("ext", 5), x, BASIC[0], 0, early=early), "0 iterations")
        # one iteration: a variable no check of the first layers touched keeps nothing raw that the oracle does not
        assert_equal(run_i8(dec, as_device(x), 1, BASIC[0].product(), w), oracle_ref(name, ("ext", 5), x, BASIC[0], 1),
                     "1 iteration")
    p = default_params()
    before = (dec.last_kernel, dec.last_ep_waves)
    assert _lib.lib().ldpc_decode_i8_async(dec._ctx, None, None, None, None, None, 0, 3, C.byref(p)) == _lib.LDPC_OK
    assert (dec.last_kernel, dec.last_ep_waves) == before
    dec.close()


# ---- the buffer contract ----------------------------------------------------------

@pytest.mark.parametrize("w", (2, 4))
@pytest.mark.parametrize("batch", (1, 3, 9))
def test_buffer_contract(batch, w, monkeypatch):
    """Input, hard and soft are slices starting 1 byte into larger buffers, iters_used 4 bytes in; everything outside
    the [batch] rows keeps its fill.  An odd batch leaves the last pair half empty."""
    torch = _torch()
    monkeypatch.setenv("LDPC_EPW_WAVES", str(w))
    name = "1248x624"
    t = load_table(name)
    n, rows = t.n, 12
    x = PD.make_input("u128", batch, n)
    p = PD.Params("NMS", 26, -127, 31)
    dec = Decoder(Code(t), max_batch=rows, kernel=9, i8_ep_wide=True)
    buf_in = torch.full((rows * n + 3,), SOFT_FILL, dtype=torch.int8, device="cuda")
    buf_soft = torch.full((rows * n + 3,), SOFT_FILL, dtype=torch.int8, device="cuda")
    buf_hard = torch.full((rows * n + 3,), HARD_FILL, dtype=torch.uint8, device="cuda")
    buf_its = torch.full((rows + 2,), ITS_FILL, dtype=torch.int32, device="cuda")
    d_in = buf_in[1:1 + batch * n].view(batch, n)
    d_in.copy_(as_device(x))
    assert d_in.data_ptr() % 2 == 1
    d_soft = buf_soft[1:1 + batch * n].view(batch, n)
    d_hard = buf_hard[1:1 + batch * n].view(batch, n)
    d_its = buf_its[1:1 + batch]
    assert d_soft.data_ptr() % 2 == 1 and d_hard.data_ptr() % 2 == 1
    dec.decode_i8_device(d_in, d_hard, 2, params=p.product(), soft=d_soft, iters_used=d_its)
    torch.cuda.synchronize()
    assert_ldsepwi(dec, w)
    soft, hard, its = buf_soft.cpu().numpy(), buf_hard.cpu().numpy(), buf_its.cpu().numpy()
    assert soft[0] == SOFT_FILL and (soft[1 + batch * n:] == SOFT_FILL).all()
    assert hard[0] == HARD_FILL and (hard[1 + batch * n:] == HARD_FILL).all()
    assert its[0] == ITS_FILL and (its[1 + batch:] == ITS_FILL).all()
    inp = buf_in.cpu().numpy()
    assert inp[0] == SOFT_FILL and (inp[1 + batch * n:] == SOFT_FILL).all()
    assert np.array_equal(inp[1:1 + batch * n].reshape(batch, n), x), "the input was written"
    exp = oracle_ref(name, ("contract", batch), x, p, 2)
    got = (hard[1:1 + batch * n].reshape(batch, n), soft[1:1 + batch * n].reshape(batch, n), its[1:1 + batch])
    assert_equal(got, exp, "batch %d on unaligned slices" % batch)
    # hard decisions alone: no soft output, no iteration counts
    only = torch.full((batch + 1, n), HARD_FILL, dtype=torch.uint8, device="cuda")
    dec.decode_i8_device(d_in, only[:batch], 2, params=p.product(early_term=1))
    torch.cuda.synchronize()
    assert_ldsepwi(dec, w)
    only = only.cpu().numpy()
    assert (only[batch] == HARD_FILL).all()
    assert np.array_equal(only[:batch], oracle_ref(name, ("contract", batch), x, p, 2, early=True)[0])
    dec.close()


def test_node_major_input(monkeypatch):
    torch = _torch()
    monkeypatch.delenv("LDPC_EPW_WAVES", raising=False)
    name = "1944x972"
    t = load_table(name)
    batch, ld = 9, 16
    x = PD.make_input("u128", batch, t.n)
    p = BASIC[0]
    exp = oracle_ref(name, ("u128", batch), x, p, 3)
    nm = torch.full((t.n, ld), SOFT_FILL, dtype=torch.int8, device="cuda")
    nm[:, :batch] = as_device(x).t()
    dec = Decoder(Code(name), max_batch=16, kernel=9, i8_ep_wide=True)
    hard = torch.full((batch + 1, t.n), HARD_FILL, dtype=torch.uint8, device="cuda")
    soft = torch.full((batch + 1, t.n), SOFT_FILL, dtype=torch.int8, device="cuda")
    its = torch.full((batch + 1,), ITS_FILL, dtype=torch.int32, device="cuda")
    dec.decode_i8_nm_device(nm, hard[:batch], 3, batch=batch, params=p.product(), soft=soft[:batch],
                            iters_used=its[:batch])
    torch.cuda.synchronize()
    assert_ldsepwi(dec)
    h, s, i = hard.cpu().numpy(), soft.cpu().numpy(), its.cpu().numpy()
    assert (h[batch] == HARD_FILL).all() and (s[batch] == SOFT_FILL).all() and i[batch] == ITS_FILL
    assert_equal((h[:batch], s[:batch], i[:batch]), exp, "node-major input")
    assert_equal(run_i8(dec, as_device(x), 3, p.product()), exp, "frame-major input")
    dec.close()


@pytest.mark.parametrize("w", (2, 4))
def test_error_counter(w, monkeypatch):
    """A decode with an error counter attached counts what count_errors_device counts on the same hard decisions,
    against a reference codeword array and without"""
    torch = _torch()
    monkeypatch.setenv("LDPC_EPW_WAVES", str(w))
    name = "1944x972"
    t = load_table(name)
    batch, k = 13, t.k_info
    x = awgn_input(name, batch)
    dev = as_device(x)
    exp = oracle_ref(name, ("awgn15", batch), x, BASIC[0], 4)
    dec = Decoder(Code(name), max_batch=16, kernel=9, i8_ep_wide=True)
    ref = torch.from_numpy((PD.make_input("ties", batch, t.n) > 0).astype(np.uint8)).cuda()
    for r in (None, ref):
        hard = torch.full((batch, t.n), HARD_FILL, dtype=torch.uint8, device="cuda")
        fused = torch.tensor([3, 5], dtype=torch.int64, device="cuda")      # the counts are added to
        dec.decode_count_device(dev, hard, 4, k, fused, ref=r, params=BASIC[0].product())
        torch.cuda.synchronize()
        assert_ldsepwi(dec, w)
        assert np.array_equal(hard.cpu().numpy(), exp[0])
        apart = torch.tensor([3, 5], dtype=torch.int64, device="cuda")
        dec.count_errors_device(hard, k, apart, ref=r)
        torch.cuda.synchronize()
        bits = exp[0][:, :k] ^ (0 if r is None else ref.cpu().numpy()[:, :k])
        want = [3 + int(bits.sum()), 5 + int(bits.any(axis=1).sum())]
        assert fused.cpu().tolist() == apart.cpu().tolist() == want
        assert want[1] > 5
    dec.close()


# ---- selection and status ---------------------------------------------------------

def test_switch_off_is_the_parents_selection(monkeypatch):
    torch = _torch()
    monkeypatch.delenv("LDPC_EPW_WAVES", raising=False)
    name = "1944x972"
    t = load_table(name)
    x = PD.make_input("u128", 3, t.n)
    dev = as_device(x)
    exp = oracle_ref(name, ("u128", 3), x, BASIC[0], 2)[0]
    hard = torch.full((3, t.n), HARD_FILL, dtype=torch.uint8, device="cuda")

    def off(dec):
        assert dec.i8_ep_wide is False
        assert dec.kernel == 0
        dec.decode_i8_device(dev, hard, 2)
        torch.cuda.synchronize()
        assert dec.last_kernel == "lds" and dec.last_skipped is None and dec.last_lds_shape[0] > 0
        assert dec.last_ep_waves == 0
        assert np.array_equal(hard.cpu().numpy(), exp)
        st, _ = _status(lambda: dec.set_kernel(9))      # refused at set_kernel
        assert st == _lib.LDPC_EUNSUPPORTED and dec.kernel == 0

    dec = Decoder(Code(name), max_batch=64)
    off(dec)
    dec.set_i8_ep_wide(True)      # on and off again: the parent's answers are back
    assert dec.i8_ep_wide is True
    dec.set_kernel(9)
    dec.decode_i8_device(dev, hard, 2)
    torch.cuda.synchronize()
    assert_ldsepwi(dec)
    assert np.array_equal(hard.cpu().numpy(), exp)
    dec.set_i8_ep_wide(False)
    st, msg = _status(lambda: dec.decode_i8_device(dev, hard, 2))      # a forced 9 no longer fits
    assert st == _lib.LDPC_EUNSUPPORTED and "not applicable" in msg, msg
    dec.set_kernel(0)
    off(dec)
    dec.close()


@pytest.mark.parametrize("others", (False, True), ids=("alone", "with_the_other_switches"))
def test_switch_on_selection(others, monkeypatch):
    torch = _torch()
    monkeypatch.delenv("LDPC_EPW_WAVES", raising=False)
    name = "1944x972"
    t = load_table(name)
    code = Code(name)
    x = PD.make_input("u128", 4, t.n)
    dev = as_device(x)
    inside, outside = BASIC[0], PD.Params("OMS", 1, -128, 31)
    exp_in = oracle_ref(name, ("u128", 4), x, inside, 2)
    exp_out = oracle_ref(name, ("u128", 4), x, outside, 2)
    hard = torch.zeros((4, t.n), dtype=torch.uint8, device="cuda")
    soft = torch.zeros((4, t.n), dtype=torch.int8, device="cuda")
    its = torch.zeros((4,), dtype=torch.int32, device="cuda")
    dec = Decoder(code, max_batch=64, i8_ep_wide=True, ep_wide=others, f16_all_codes=others)
    assert dec.i8_edge_parallel is False and dec.f16_edge_parallel is False      # refused on this code: they stay off
    # automatic, inside the domain: the rule decides
    auto = code.i8_ep_wide_info(4)["waves_auto"]
    assert auto == IW.rule(12, 11, 0b10100, 4)[0] * IW.rule(12, 11, 0b10100, 4)[1]
    if auto:
        assert_equal(run_i8(dec, dev, 2, inside.product(), auto), exp_in, "automatic")
    else:      # the rule hands the batch back: the choice with the switch off
        dec.decode_i8_device(dev, hard, 2, params=inside.product(), soft=soft, iters_used=its)
        torch.cuda.synchronize()
        assert dec.last_kernel == "lds" and dec.last_skipped is None and dec.last_ep_waves == 0
        assert_equal((hard.cpu().numpy(), soft.cpu().numpy(), its.cpu().numpy()), exp_in, "automatic, handed back")
    # automatic, outside the domain: the parent's choice, which says what it passed over
    dec.decode_i8_device(dev, hard, 2, params=outside.product(), soft=soft, iters_used=its)
    torch.cuda.synchronize()
    assert dec.last_kernel == "lds" and dec.last_skipped == "ldsep" and dec.last_lds_shape[0] > 0
    assert dec.last_ep_waves == 0
    assert_equal((hard.cpu().numpy(), soft.cpu().numpy(), its.cpu().numpy()), exp_out, "var_min -128, automatic")
    # forced 9: ldsepwi whatever the rule says; outside the domain refused
    dec.set_kernel(9)
    assert_equal(run_i8(dec, dev, 2, inside.product()), exp_in, "forced 9")
    st, msg = _status(lambda: dec.decode_i8_device(dev, hard, 2, params=outside.product()))
    assert st == _lib.LDPC_EUNSUPPORTED and "not applicable" in msg, msg
    assert_equal(run_i8(dec, dev, 2, inside.product()), exp_in, "forced 9 after the refusal")
    # LDPC_EPW_WAVES: a W outside the int8 mask is refused before anything is recorded
    for w in ("3", "8", "1"):
        monkeypatch.setenv("LDPC_EPW_WAVES", w)
        st, _ = _status(lambda: dec.decode_i8_device(dev, hard, 2, params=inside.product()))
        assert st == _lib.LDPC_EUNSUPPORTED and dec.last_ep_waves in (2, 4)
    monkeypatch.delenv("LDPC_EPW_WAVES")
    # a float32 decode on the same context follows ep_wide only
    y = torch.from_numpy(np.array(ST.f32_input(4, t.n))).cuda()
    ms = default_params(algo=ALGO_MS)
    if others:
        dec.decode_f32_device(y, hard, 2, params=ms)
        torch.cuda.synchronize()
        assert dec.last_kernel == "ldsep" and dec.last_ep_waves == code.ep_wide_info(4)["waves_auto"] != 0
    else:
        st, msg = _status(lambda: dec.decode_f32_device(y, hard, 2, params=ms))
        assert st == _lib.LDPC_EUNSUPPORTED and "not applicable" in msg, msg
    dec.set_kernel(0)
    dec.decode_f32_device(y, hard, 2, params=ms)
    torch.cuda.synchronize()
    assert (dec.last_kernel, dec.last_ep_waves) == (("ldsep", code.ep_wide_info(4)["waves_auto"]) if others else ("lds", 0))
    # every other forced family: unchanged
    for k, family in ((7, "lds"), (1, "generic")):
        dec.set_kernel(k)
        dec.decode_i8_device(dev, hard, 2, params=inside.product())
        torch.cuda.synchronize()
        assert dec.last_kernel == family and dec.last_skipped is None and dec.last_ep_waves == 0
        assert np.array_equal(hard.cpu().numpy(), exp_in[0]), k
    # parameter checking is unchanged
    dec.set_kernel(0)
    assert _status(lambda: dec.decode_i8_device(dev, hard, 2, params=default_params(algo=ALGO_BP)))[0] == \
        _lib.LDPC_EUNSUPPORTED
    assert _status(lambda: dec.decode_i8_device(dev, hard, 2, params=default_params(var_min=-129)))[0] == \
        _lib.LDPC_EINVAL
    assert _status(lambda: dec.decode_i8_device(dev, hard, 2, params=default_params(offset=256)))[0] == _lib.LDPC_EINVAL
    dec.close()


def test_waves_outside_the_mask(monkeypatch):
    t = load_table("2304x1152")
    dev = as_device(PD.make_input("u128", 2, t.n))
    hard = _torch().zeros((2, t.n), dtype=_torch().uint8, device="cuda")
    dec = Decoder(Code("2304x1152"), max_batch=8, kernel=9, i8_ep_wide=True)
    for w in ("2", "3", "8", "1"):
        monkeypatch.setenv("LDPC_EPW_WAVES", w)
        st, _ = _status(lambda: dec.decode_i8_device(dev, hard, 2))
        assert st == _lib.LDPC_EUNSUPPORTED and dec.last_ep_waves == 0, w
    monkeypatch.setenv("LDPC_EPW_WAVES", "4")
    dec.decode_i8_device(dev, hard, 2)
    _torch().cuda.synchronize()
    assert_ldsepwi(dec, 4)
    dec.close()


@pytest.mark.parametrize("name", ("648x324", "200x100", "dvbs2_r1_2"))
def test_switch_refused_without_a_wide_plan(name):
    dec = Decoder(Code(name), max_batch=8)
    for flag in (True, False):
        st, _ = _status(lambda: dec.set_i8_ep_wide(flag))
        assert st == _lib.LDPC_EUNSUPPORTED
        assert dec.i8_ep_wide is False
    dec.close()
    st, _ = _status(lambda: Decoder(Code(name), max_batch=8, i8_ep_wide=True))
    assert st == _lib.LDPC_EUNSUPPORTED


# ---- context reuse ----------------------------------------------------------------

def test_decoders_used_alternately(monkeypatch):
    monkeypatch.delenv("LDPC_EPW_WAVES", raising=False)
    short = Decoder(Code("648x324"), max_batch=64, i8_edge_parallel=True)
    wide = Decoder(Code("1944x972"), max_batch=64, kernel=9, i8_ep_wide=True)
    ts, tw = load_table("648x324"), load_table("1944x972")
    xs, xw = PD.make_input("u128", 37, ts.n), PD.make_input("u128", 37, tw.n)
    ds, dw = as_device(xs), as_device(xw)
    p = BASIC[0]
    es = oracle_ref("648x324", ("u128", 37), xs, p, 6)
    ew = oracle_ref("1944x972", ("u128", 37), xw, p, 6)
    torch = _torch()
    for rnd, (batch, w, kernel) in enumerate(((37, "2", 9), (5, "4", 9), (1, "2", 7), (37, "4", 9), (9, None, 9))):
        hard = torch.full((batch, ts.n), HARD_FILL, dtype=torch.uint8, device="cuda")
        soft = torch.full((batch, ts.n), SOFT_FILL, dtype=torch.int8, device="cuda")
        its = torch.full((batch,), ITS_FILL, dtype=torch.int32, device="cuda")
        short.decode_i8_device(ds[:batch], hard, 6, params=p.product(), soft=soft, iters_used=its)
        torch.cuda.synchronize()
        assert (short.last_kernel, short.last_ep_waves) == ("ldsep", 0)
        assert_equal((hard.cpu().numpy(), soft.cpu().numpy(), its.cpu().numpy()), rows_of(es, batch), "648x324 round %d" % rnd)
        if w:
            monkeypatch.setenv("LDPC_EPW_WAVES", w)
        else:
            monkeypatch.delenv("LDPC_EPW_WAVES", raising=False)
        wide.set_kernel(kernel)
        hard = torch.full((batch, tw.n), HARD_FILL, dtype=torch.uint8, device="cuda")
        soft = torch.full((batch, tw.n), SOFT_FILL, dtype=torch.int8, device="cuda")
        its = torch.full((batch,), ITS_FILL, dtype=torch.int32, device="cuda")
        wide.decode_i8_device(dw[:batch], hard, 6, params=p.product(), soft=soft, iters_used=its)
        torch.cuda.synchronize()
        assert wide.last_kernel == ("ldsep" if kernel == 9 else "lds")
        assert wide.last_ep_waves == (0 if kernel == 7 else int(w) if w else IW.rule(12, 11, 0b10100, batch)[0])
        assert_equal((hard.cpu().numpy(), soft.cpu().numpy(), its.cpu().numpy()), rows_of(ew, batch), "1944x972 round %d" % rnd)
    short.close()
    wide.close()
