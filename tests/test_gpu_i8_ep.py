"""The edge-parallel int8 kernel on the GPU (`ldsepi`: family 9 of the int8
decode, behind the i8_edge_parallel switch) against oracle.decode_i8, which
test_i8_ep_cpu.py ties to the host decoder on the same domain.  "Equal" is always
hard decisions, int8 soft output and iters_used with zero differing elements.

* every table of ldsep_domain (check degrees 2 .. 8: padding lanes; Z = 8, 27,
  32 in the 12 x 4 shape and Z = 41 in the 11 x 6 shape: full, ragged and empty
  passes; half of each table under the later-group rule) x OMS / MS / NMS at
  batches 1, 2, 7, 9 and 17: a lone half, one pair, a ragged workgroup with an
  odd tail, a second workgroup holding a lone half, several workgroups; guard
  rows behind every output;
* on the d = 2, 5, 8 tables the corners of the parameter domain, var_min = -64
  and var_min = 0 among them: where an int8 sink would fail;
* the shipped 648x324 and 576x288 tables, the reference's golden vectors;
* early termination per half, 0 iterations, an empty batch;
* the buffer contract on 1-byte aligned slices of odd batches, node-major input,
  the error counter;
* selection with the switch off (the parent's answers) and on."""
import ctypes as C

import numpy as np
import pytest

import ldsep_domain as ED
import oracle as O
import param_domain as PD
import struct_domain as ST
from conftest import golden_cases, golden_inputs
from ldpcgputegra_amd import ALGO_BP, ALGO_MS, ALGO_NMS, ALGO_OMS, Code, Decoder, LdpcError, _lib, channel, \
    default_params, load_table
from test_i8_ep_cpu import ET_BATCH, ET_CODE, ET_ITERS, ET_ITERS_USED, ET_PARAMS, et_input

pytestmark = pytest.mark.gpu

BATCHES = (1, 2, 7, 9, 17)
BASIC = [PD.Params("OMS", 1, -127, 31), PD.Params("MS", 0, -127, 31), PD.Params("NMS", 26, -127, 31)]
CORNERS = [PD.Params("OMS", 63, -127, 63), PD.Params("OMS", 5, -127, 0), PD.Params("OMS", 3, -127, 127),
           PD.Params("OMS", 255, -127, 127), PD.Params("NMS", 64, -127, 63), PD.Params("NMS", 255, -127, 127),
           PD.Params("OMS", 1, -64, 31), PD.Params("OMS", 1, 0, 31)]
HAZARD_TABLES = [(d, rows, Z) for rows, Z in ED.SHAPES for d in (2, 5, 8)]
SOFT_FILL, HARD_FILL, ITS_FILL = 0x55, 9, -7
GOLDEN_576 = [c for c in golden_cases() if c["code"] == "576x288"]


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
    """the first `batch` codewords of a reference (codewords decode independently)"""
    return tuple(a[:batch] for a in ref)


def as_device(x):
    return _torch().from_numpy(np.array(x)).cuda()


def run_i8(dec, d_llr, iters, params, extra=2):
    """decode_i8_device with guard rows behind every output; asserts the launch was ldsepi"""
    torch = _torch()
    B, n = d_llr.shape
    d_hard = torch.full((B + extra, n), HARD_FILL, dtype=torch.uint8, device="cuda")
    d_soft = torch.full((B + extra, n), SOFT_FILL, dtype=torch.int8, device="cuda")
    d_its = torch.full((B + extra,), ITS_FILL, dtype=torch.int32, device="cuda")
    dec.decode_i8_device(d_llr, d_hard, iters, params=params, soft=d_soft, iters_used=d_its)
    torch.cuda.synchronize()
    assert_ldsepi(dec)
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


def assert_ldsepi(dec):
    assert dec.last_kernel == "ldsep" and dec.last_skipped is None
    assert dec.last_lds_shape == (0, False) and dec.last_ep_waves == 0 and dec.last_et_stage == 0


def _status(fn):
    with pytest.raises(LdpcError) as e:
        fn()
    return e.value.status, str(e.value)


# ---- degrees x shapes x batches ---------------------------------------------------

@pytest.mark.parametrize("d,rows,Z", ED.ALL, ids=[ED.synthetic_name(*k) for k in ED.ALL])
def test_every_table(d, rows, Z):
    name = (d, rows, Z)
    t = ED.synthetic(*name)
    x = PD.make_input("u128", max(BATCHES), t.n)
    dev = as_device(x)
    dec = Decoder(Code(t), max_batch=max(BATCHES), i8_edge_parallel=True)
    assert dec.i8_edge_parallel is True and dec.f16_edge_parallel is False and dec.ep_wide is False
    for p in BASIC:
        exp = oracle_ref(name, ("u128", max(BATCHES)), x, p, 3)
        for batch in BATCHES:
            got = run_i8(dec, dev[:batch], 3, p.product())
            assert_equal(got, rows_of(exp, batch), "%s %s batch %d" % (_name(name), p.id, batch))
    dec.close()


@pytest.mark.parametrize("d,rows,Z", HAZARD_TABLES, ids=[ED.synthetic_name(*k) for k in HAZARD_TABLES])
def test_parameter_corners(d, rows, Z):
    """The var_min entries are where the padding lanes show: with an int8 sink,
    var_min = -64 would put |sink| below live magnitudes and var_min = 0 would
    lose the odd-degree flip; degree 2 has six padding lanes per check, Z = 27
    and 41 have empty slots, half of each table uses the later-group rule."""
    name = (d, rows, Z)
    t = ED.synthetic(*name)
    dec = Decoder(Code(t), max_batch=max(BATCHES), i8_edge_parallel=True)
    for kind in ("ext", "ties"):
        x = PD.make_input(kind, max(BATCHES), t.n)
        dev = as_device(x)
        for p in CORNERS:
            exp = oracle_ref(name, (kind, max(BATCHES)), x, p, 3)
            for batch in BATCHES:
                got = run_i8(dec, dev[:batch], 3, p.product())
                assert_equal(got, rows_of(exp, batch), "%s %s %s batch %d" % (_name(name), kind, p.id, batch))
    dec.close()


# ---- the shipped tables -----------------------------------------------------------

def awgn_input(name, batch):
    t = load_table(name)
    return channel.awgn_i8_host(t.n, batch, seed=1, table=channel.i8_table(channel.sigma_from_ebn0(1.5, t.k_info / t.n)))


@pytest.mark.parametrize("kernel", (0, 9))
@pytest.mark.parametrize("name", ("648x324", "576x288"))
def test_shipped_tables(name, kernel):
    t = load_table(name)
    dec = Decoder(Code(name), max_batch=17, kernel=kernel, i8_edge_parallel=True)
    for key, x in (("u128", PD.make_input("u128", 17, t.n)), ("awgn15", awgn_input(name, 17))):
        dev = as_device(x)
        for p in BASIC:
            got = run_i8(dec, dev, 20, p.product())
            assert_equal(got, oracle_ref(name, (key, 17), x, p, 20), "%s kernel %d %s %s" % (name, kernel, key, p.id))
    dec.close()


@pytest.mark.parametrize("case", GOLDEN_576, ids=[c["name"] for c in GOLDEN_576])
def test_golden_cases(case):
    """The reference's recorded hard decisions, through the host-buffer entry point"""
    assert len(GOLDEN_576) == 28
    llr, hard = golden_inputs(case)
    algo = {0: ALGO_OMS, 1: ALGO_NMS}[case["algo"]]
    p = default_params(algo=algo, offset=case["param"], factor=case["param"], var_min=case["var_min"],
                       msg_max=case["msg_max"], msg_min=-case["msg_max"])
    dec = Decoder(Code("576x288"), max_batch=case["batch"], i8_edge_parallel=True)
    got = dec.decode_i8(llr, case["iters"], p)
    if case["var_min"] >= -127:
        assert_ldsepi(dec)
    else:      # outside the kernel's domain: the automatic choice is the parent's, and says what it passed over
        assert dec.last_kernel == "lds" and dec.last_skipped == "ldsep"
    assert np.array_equal(got, hard), case["name"]
    if case["var_min"] >= -127:      # the asynchronous host-buffer entry point takes the same dispatch
        out = np.zeros_like(hard)
        dec.decode_i8_host_async(np.ascontiguousarray(llr), out, case["iters"], p)
        dec.synchronize()
        assert_ldsepi(dec)
        assert np.array_equal(out, hard), case["name"]
    dec.close()


# ---- early termination ------------------------------------------------------------

@pytest.mark.parametrize("algo", sorted(ET_PARAMS))
def test_early_termination(algo):
    torch = _torch()
    p = ET_PARAMS[algo]
    x = et_input()
    dev = as_device(x)
    exp = oracle_ref(ET_CODE, "i8ep_et", x, p, ET_ITERS, early=True)
    assert exp[2].tolist() == ET_ITERS_USED[algo]
    dec = Decoder(Code(ET_CODE), max_batch=ET_BATCH, i8_edge_parallel=True)
    for batch in (ET_BATCH, ET_BATCH - 1, 1):      # a lone last half; none; a lone half alone
        got = run_i8(dec, dev[:batch], ET_ITERS, p.product(early_term=1))
        assert_equal(got, rows_of(exp, batch), "early termination %s, batch %d" % (algo, batch))
    # no iters_used array
    hard = torch.full((ET_BATCH, x.shape[1]), HARD_FILL, dtype=torch.uint8, device="cuda")
    soft = torch.full((ET_BATCH, x.shape[1]), SOFT_FILL, dtype=torch.int8, device="cuda")
    dec.decode_i8_device(dev, hard, ET_ITERS, params=p.product(early_term=1), soft=soft)
    torch.cuda.synchronize()
    assert_ldsepi(dec)
    assert np.array_equal(hard.cpu().numpy(), exp[0]) and np.array_equal(soft.cpu().numpy(), exp[1])
    dec.close()


def test_zero_iterations_and_empty_batch():
    name = "648x324"
    t = load_table(name)
    x = PD.make_input("ext", 5, t.n)      # raw -128 LLRs among them
    dec = Decoder(Code(name), max_batch=8, i8_edge_parallel=True)
    for early in (False, True):
        hard, soft, its = run_i8(dec, as_device(x), 0, default_params(early_term=int(early)))
        assert np.array_equal(soft, x) and np.array_equal(hard, (x > 0).astype(np.uint8)) and not its.any()
        assert_equal((hard, soft, its), oracle_ref(name, ("ext", 5), x, BASIC[0], 0, early=early), "0 iterations")
    # one iteration: a variable no check of the first layers touched keeps nothing raw that the oracle does not
    assert_equal(run_i8(dec, as_device(x), 1, BASIC[0].product()), oracle_ref(name, ("ext", 5), x, BASIC[0], 1),
                 "1 iteration")
    p = default_params()
    before = dec.last_kernel
    assert _lib.lib().ldpc_decode_i8_async(dec._ctx, None, None, None, None, None, 0, 3, C.byref(p)) == _lib.LDPC_OK
    assert dec.last_kernel == before
    dec.close()


# ---- the buffer contract ----------------------------------------------------------

@pytest.mark.parametrize("batch", (1, 3, 9))
def test_buffer_contract(batch):
    """Input, hard and soft are slices starting 1 byte into larger buffers,
    iters_used 4 bytes in; everything outside the [batch] rows keeps its fill.
    An odd batch leaves the last pair half empty."""
    torch = _torch()
    name = "576x288"
    t = load_table(name)
    n, rows = t.n, 12
    x = PD.make_input("u128", batch, n)
    p = PD.Params("NMS", 26, -127, 31)
    dec = Decoder(Code(t), max_batch=rows, kernel=9, i8_edge_parallel=True)
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
    assert_ldsepi(dec)
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
    assert_ldsepi(dec)
    only = only.cpu().numpy()
    assert (only[batch] == HARD_FILL).all()
    assert np.array_equal(only[:batch], oracle_ref(name, ("contract", batch), x, p, 2, early=True)[0])
    dec.close()


def test_node_major_input():
    torch = _torch()
    name = "648x324"
    t = load_table(name)
    batch, ld = 9, 16
    x = PD.make_input("u128", batch, t.n)
    p = BASIC[0]
    exp = oracle_ref(name, ("u128", batch), x, p, 3)
    nm = torch.full((t.n, ld), SOFT_FILL, dtype=torch.int8, device="cuda")
    nm[:, :batch] = as_device(x).t()
    dec = Decoder(Code(name), max_batch=16, i8_edge_parallel=True)
    hard = torch.full((batch + 1, t.n), HARD_FILL, dtype=torch.uint8, device="cuda")
    soft = torch.full((batch + 1, t.n), SOFT_FILL, dtype=torch.int8, device="cuda")
    its = torch.full((batch + 1,), ITS_FILL, dtype=torch.int32, device="cuda")
    dec.decode_i8_nm_device(nm, hard[:batch], 3, batch=batch, params=p.product(), soft=soft[:batch],
                            iters_used=its[:batch])
    torch.cuda.synchronize()
    assert_ldsepi(dec)
    h, s, i = hard.cpu().numpy(), soft.cpu().numpy(), its.cpu().numpy()
    assert (h[batch] == HARD_FILL).all() and (s[batch] == SOFT_FILL).all() and i[batch] == ITS_FILL
    assert_equal((h[:batch], s[:batch], i[:batch]), exp, "node-major input")
    assert_equal(run_i8(dec, as_device(x), 3, p.product()), exp, "frame-major input")
    dec.close()


def test_error_counter():
    """A decode with an error counter attached counts what count_errors_device
    counts on the same hard decisions, against a reference codeword and without"""
    torch = _torch()
    name = "648x324"
    t = load_table(name)
    batch, k = 17, t.k_info
    x = awgn_input(name, batch)
    dev = as_device(x)
    exp = oracle_ref(name, ("awgn15", batch), x, BASIC[0], 4)
    dec = Decoder(Code(name), max_batch=batch, i8_edge_parallel=True)
    ref = torch.from_numpy((PD.make_input("ties", batch, t.n) > 0).astype(np.uint8)).cuda()
    for r in (None, ref):
        hard = torch.full((batch, t.n), HARD_FILL, dtype=torch.uint8, device="cuda")
        fused = torch.tensor([3, 5], dtype=torch.int64, device="cuda")      # the counts are added to
        dec.decode_count_device(dev, hard, 4, k, fused, ref=r, params=BASIC[0].product())
        torch.cuda.synchronize()
        assert_ldsepi(dec)
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

def test_switch_off_is_the_parents_selection():
    torch = _torch()
    name = "648x324"
    t = load_table(name)
    x = PD.make_input("u128", 3, t.n)
    dev = as_device(x)
    exp = oracle_ref(name, ("u128", 3), x, BASIC[0], 2)[0]
    hard = torch.full((3, t.n), HARD_FILL, dtype=torch.uint8, device="cuda")

    def off(dec):
        assert dec.i8_edge_parallel is False
        dec.set_kernel(0)
        dec.decode_i8_device(dev, hard, 2)
        torch.cuda.synchronize()
        assert dec.last_kernel == "lds" and dec.last_skipped is None and dec.last_lds_shape[0] > 0
        assert np.array_equal(hard.cpu().numpy(), exp)
        dec.set_kernel(9)
        st, msg = _status(lambda: dec.decode_i8_device(dev, hard, 2))
        assert st == _lib.LDPC_EUNSUPPORTED and "not applicable" in msg, msg
        dec.set_kernel(0)

    dec = Decoder(Code(name), max_batch=64)
    off(dec)
    dec.set_i8_edge_parallel(True)      # on and off again: the parent's answers are back
    assert dec.i8_edge_parallel is True
    dec.decode_i8_device(dev, hard, 2)
    torch.cuda.synchronize()
    assert_ldsepi(dec)
    assert np.array_equal(hard.cpu().numpy(), exp)
    dec.set_i8_edge_parallel(False)
    off(dec)
    dec.close()


@pytest.mark.parametrize("others", (False, True), ids=("alone", "with_the_other_switches"))
def test_switch_on_selection(others):
    torch = _torch()
    name = "648x324"
    t = load_table(name)
    x = PD.make_input("u128", 4, t.n)
    dev = as_device(x)
    inside, outside = BASIC[0], PD.Params("OMS", 1, -128, 31)
    exp_in = oracle_ref(name, ("u128", 4), x, inside, 2)
    exp_out = oracle_ref(name, ("u128", 4), x, outside, 2)
    hard = torch.zeros((4, t.n), dtype=torch.uint8, device="cuda")
    dec = Decoder(Code(name), max_batch=64, i8_edge_parallel=True, f16_edge_parallel=others, f16_all_codes=others,
                  ep_wide=others)
    for k in (0, 9):
        dec.set_kernel(k)
        assert_equal(run_i8(dec, dev, 2, inside.product()), exp_in, "kernel %d" % k)
    # outside the domain: automatic falls back to the parent's choice, forced 9 is refused
    dec.set_kernel(0)
    soft = torch.zeros((4, t.n), dtype=torch.int8, device="cuda")
    its = torch.zeros((4,), dtype=torch.int32, device="cuda")
    dec.decode_i8_device(dev, hard, 2, params=outside.product(), soft=soft, iters_used=its)
    torch.cuda.synchronize()
    assert dec.last_kernel == "lds" and dec.last_skipped == "ldsep" and dec.last_lds_shape[0] > 0
    assert_equal((hard.cpu().numpy(), soft.cpu().numpy(), its.cpu().numpy()), exp_out, "var_min -128, automatic")
    dec.set_kernel(9)
    st, msg = _status(lambda: dec.decode_i8_device(dev, hard, 2, params=outside.product()))
    assert st == _lib.LDPC_EUNSUPPORTED and "not applicable" in msg, msg
    assert_equal(run_i8(dec, dev, 2, inside.product()), exp_in, "forced 9 after the refusal")
    # every other forced family: unchanged
    for k, family in ((7, "lds"), (1, "generic")):
        dec.set_kernel(k)
        dec.decode_i8_device(dev, hard, 2, params=inside.product())
        torch.cuda.synchronize()
        assert dec.last_kernel == family and dec.last_skipped is None
        assert np.array_equal(hard.cpu().numpy(), exp_in[0]), k
    # parameter checking is unchanged
    dec.set_kernel(0)
    assert _status(lambda: dec.decode_i8_device(dev, hard, 2, params=default_params(algo=ALGO_BP)))[0] == \
        _lib.LDPC_EUNSUPPORTED
    assert _status(lambda: dec.decode_i8_device(dev, hard, 2, params=default_params(var_min=-129)))[0] == \
        _lib.LDPC_EINVAL
    assert _status(lambda: dec.decode_i8_device(dev, hard, 2, params=default_params(offset=256)))[0] == _lib.LDPC_EINVAL
    dec.close()


@pytest.mark.parametrize("name", ("200x100", "dvbs2_r1_2"))
def test_switch_refused_where_the_family_does_not_fit(name):
    dec = Decoder(Code(name), max_batch=8)
    for flag in (True, False):
        st, _ = _status(lambda: dec.set_i8_edge_parallel(flag))
        assert st == _lib.LDPC_EUNSUPPORTED
        assert dec.i8_edge_parallel is False
    dec.close()
    st, _ = _status(lambda: Decoder(Code(name), max_batch=8, i8_edge_parallel=True))
    assert st == _lib.LDPC_EUNSUPPORTED


def test_switch_refused_on_the_longer_qc_code():
    """1944x972 is a table of the several-wave kernel only: refused whatever ep_wide says"""
    for wide in (False, True):
        dec = Decoder(Code("1944x972"), max_batch=8, ep_wide=wide)
        st, _ = _status(lambda: dec.set_i8_edge_parallel(True))
        assert st == _lib.LDPC_EUNSUPPORTED and dec.i8_edge_parallel is False
        dec.close()
    st, _ = _status(lambda: Decoder(Code("1944x972"), max_batch=8, ep_wide=True, i8_edge_parallel=True))
    assert st == _lib.LDPC_EUNSUPPORTED


def test_other_element_types_around_ldsepi():
    """An ldsepi decode allocates and leaves nothing: float32, binary16 and BP
    decodes on the same context before and after it equal the host decoder's."""
    torch = _torch()
    name = "648x324"
    t = load_table(name)
    y = np.array(ST.f32_input(9, t.n))
    h16 = y.astype(np.float16)
    q = PD.make_input("u128", 9, t.n)
    host = Decoder(Code(name), device=-1, max_batch=9)
    ref32 = host.decode_f32(y, 3, default_params(algo=ALGO_MS))
    refbp = host.decode_f32(y, 3, default_params(algo=ALGO_BP))
    ref16 = host.decode_f16(h16, 3, default_params(algo=ALGO_MS))
    host.close()
    exp8 = oracle_ref(name, ("u128", 9), q, BASIC[0], 3)
    dec = Decoder(Code(name), max_batch=16, i8_edge_parallel=True, f16_edge_parallel=True)
    hard = torch.zeros((9, t.n), dtype=torch.uint8, device="cuda")
    d_y = torch.from_numpy(y).cuda()
    d_h = torch.from_numpy(h16.view(np.int16)).cuda().view(torch.float16)

    def others():
        dec.decode_f32_device(d_y, hard, 3, params=default_params(algo=ALGO_MS))
        torch.cuda.synchronize()
        assert dec.last_kernel == "ldsep" and np.array_equal(hard.cpu().numpy(), ref32)
        dec.decode_f32_device(d_y, hard, 3, params=default_params(algo=ALGO_BP))
        torch.cuda.synchronize()
        assert dec.last_kernel == "lds" and np.array_equal(hard.cpu().numpy(), refbp)
        dec.decode_f16_device(d_h, hard, 3, params=default_params(algo=ALGO_MS))
        torch.cuda.synchronize()
        assert dec.last_kernel == "ldsep" and np.array_equal(hard.cpu().numpy(), ref16)

    others()
    assert_equal(run_i8(dec, as_device(q), 3, BASIC[0].product()), exp8, "between the others")
    others()
    assert_equal(run_i8(dec, as_device(q), 3, BASIC[0].product()), exp8, "after the others")
    dec.close()
