"""The int8 kernels of the short codes -- generic (1), lds (7) and the
automatic choice -- on the sixteen plain .ldpc tables and on synthetic tables
of every check degree 2 .. 32 (short_domain.py), over the whole LLR range
(|LLR| up to 127, -128, checks whose edges all tie at 127) and the parameter
grid of param_domain.py: hard decisions, soft output and iterations used bit
for bit against the oracle.  test_short_domain_cpu.py shows that the oracle
equals the reference's own decoder on five of these codes and the host decoder
on all of them, so a mismatch here is a kernel or dispatch bug.

What the inputs reach that the AWGN inputs (|LLR| <= 31 = msg_max) do not: the
later-group rule abs(min(c, msg_max)) differs from min(abs(c), msg_max) only
for a contribution below -msg_max, and the later group is most of 576x288,
648x324, 1024x518, 1200x600, 1248x624, 1944x972, 2304x1152 and half of every
synthetic table.

Kernel 7's launch shape depends on the batch: lanes per codeword grow from
the code's own (8 .. 64 by its widest layer) while the launch has fewer than
2048 waves, and two lanes share a check once there are twice as many lanes as
checks in the widest layer.  Every test on kernel 7 asserts the shape the
launch took (Decoder.last_lds_shape), so a change of the heuristic cannot move
these tests off the shapes they exist for unnoticed:

* batch 32: one codeword per wave; split for the five narrow-layer codes and
  the Z = 12 synthetic tables, lanes looping over the checks for the others;
* short_domain.PACKED: 2, 4 and 8 codewords per wave, with and without the
  split, at the smallest batches with those shapes (4099 .. 16387, which is
  why this file alone goes that high), the last wave partly empty;
* early termination in the packed shapes: the syndrome ballot masked per
  codeword, `live` differing inside a wave, the wave-wide break."""
import numpy as np
import pytest

import float_domain as FD
import oracle as O
import param_domain as PD
import short_domain as SD
from ldpcgputegra_amd import ALGO_MS, Code, Decoder, default_params, load_table
from test_gpu_float_domain import assert_same
from test_gpu_parity import kernels_for

pytestmark = pytest.mark.gpu

BATCH, ITERS = 32, 4
SWEEP_ITERS, PACKED_ITERS = 3, 3
PACKED_INPUTS = ("u128", "ties")
_decoders = {}
_device_inputs = {}


def _torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def decoder(name, kernel, max_batch=64, table=None):
    key = (name, kernel, max_batch)
    if key not in _decoders:
        _decoders[key] = Decoder(Code(table if table is not None else name), max_batch=max_batch, kernel=kernel)
    return _decoders[key]


def device_input(kind, batch, n):
    if (kind, batch, n) not in _device_inputs:
        _device_inputs[(kind, batch, n)] = _torch().from_numpy(PD.make_input(kind, batch, n).copy()).cuda()
    return _device_inputs[(kind, batch, n)]


def run(dec, d_llr, iters, params, batch=None, extra=0, node_major=False):
    """(hard, soft, iters_used) of one device decode into buffers of
    batch + extra rows filled with sentinels."""
    torch = _torch()
    B = batch or d_llr.shape[0]
    n = dec.code.n
    d_hard = torch.full((B + extra, n), 9, dtype=torch.uint8, device="cuda")
    d_soft = torch.full((B + extra, n), 99, dtype=torch.int8, device="cuda")
    d_its = torch.full((B + extra,), -7, dtype=torch.int32, device="cuda")
    if node_major:
        dec.decode_i8_nm_device(d_llr, d_hard, iters, batch=B, params=params, soft=d_soft, iters_used=d_its)
    else:
        dec.decode_i8_device(d_llr, d_hard, iters, params=params, soft=d_soft, iters_used=d_its)
    torch.cuda.synchronize()
    hard, soft, its = d_hard.cpu().numpy(), d_soft.cpu().numpy(), d_its.cpu().numpy()
    assert (hard[B:] == 9).all() and (soft[B:] == 99).all() and (its[B:] == -7).all(), "rows beyond the batch written"
    return hard[:B], soft[:B], its[:B]


def assert_equal(got, exp, where):
    """hard, soft and iterations used against the oracle's, bit for bit."""
    for g, e, what in zip((got[1], got[0], got[2]), (exp[1], exp[0], exp[2]), ("soft", "hard", "iters_used")):
        assert g.shape == e.shape, (where, what, g.shape, e.shape)
        diff = g != e
        assert not diff.any(), "%s: %d %s values differ from the oracle in %d codewords, the first codeword %d" % (
            where, int(diff.sum()), what, int(diff.reshape(len(g), -1).any(axis=1).sum()),
            int(np.argmax(diff.reshape(len(g), -1).any(axis=1))))


def test_tables_match_the_codes():
    for code in SD.SHORT_CODES:
        assert kernels_for(code) == SD.KERNELS[code], code


def _small_grid():
    return [(c, p) for c in SD.LDS_CODES for p in PD.GRID] + [(c, p) for c in SD.GENERIC_ONLY for p in PD.SUBSET]


@pytest.mark.parametrize("code,params", _small_grid(), ids=lambda v: v if isinstance(v, str) else v.id)
def test_forced_kernels_vs_oracle(code, params):
    """Every kernel family of the code, forced, and the automatic choice, on
    the four full-range inputs, batch 32, 4 iterations.  No kernel refuses a
    grid point: generic and lds take everything check_params lets through, so
    an LdpcError fails the test."""
    n = load_table(code).n
    width = SD.LAYER_PLAN[code][1]
    for kind in PD.INPUTS:
        exp = PD.oracle_on(code, kind, BATCH, params, ITERS)
        assert (exp[2] == ITERS).all()
        for k in SD.KERNELS[code] + [0]:
            dec = decoder(code, k)
            got = run(dec, device_input(kind, BATCH, n), ITERS, params.product(), extra=2)
            name = Decoder.KERNEL_NAMES[k] if k else SD.AUTO[code]
            where = "%s %s %s kernel %d (%s)" % (code, params.id, kind, k, dec.last_kernel)
            assert dec.last_kernel == name and dec.last_skipped is None, where
            assert dec.last_lds_shape == ((64, 64 >= 2 * width) if name == "lds" else (0, False)), where
            assert_equal(got, exp, where)


@pytest.mark.parametrize("Z", [SD.Z_SPLIT, SD.Z_LOOP])
@pytest.mark.parametrize("d", SD.DEGREES)
def test_synthetic_degree_sweep(d, Z):
    """Code(Table): check degree d in the first group and max(2, d - 1) in the
    later one, so every instance of LDPC_DEG_CASES / LDPC_LDS_DEG_CASES runs
    with and without the later-group rule.  Z = 12: two lanes per check (the
    odd degrees with their padding lane), lanes 24 .. 63 idle; Z = 40: one
    lane per check, lanes 40 .. 63 idle."""
    t = SD.synthetic(d, Z)
    name = SD.synthetic_name(d, Z)
    for params in SD.SWEEP_PARAMS:
        for kind in SD.SWEEP_INPUTS:
            exp = SD.oracle_synthetic(d, Z, kind, BATCH, params, SWEEP_ITERS)
            for k in (1, 7):
                dec = decoder(name, k, table=t)
                got = run(dec, device_input(kind, BATCH, t.n), SWEEP_ITERS, params.product(), extra=2)
                where = "%s %s %s kernel %d" % (name, params.id, kind, k)
                assert dec.last_kernel == Decoder.KERNEL_NAMES[k], where
                assert dec.last_lds_shape == ((64, Z == SD.Z_SPLIT) if k == 7 else (0, False)), where
                assert_equal(got, exp, where)
    for k in (1, 7):
        _decoders.pop((name, k, 64)).close()


@pytest.mark.parametrize("params", PD.SUBSET, ids=lambda p: p.id)
@pytest.mark.parametrize("row", SD.PACKED, ids=SD.packed_id)
def test_packed_shapes_vs_oracle(row, params):
    """Kernel 7 with 2, 4 and 8 codewords per wave, split and not: the launch
    took the row's shape; every codeword, those of the partly empty last wave
    included, equals the oracle's; the rows beyond the batch of an oversized
    output keep their sentinel."""
    code, batch, lanes, split = row
    n = load_table(code).n
    dec = decoder(code, 7, max_batch=batch)
    for kind in PACKED_INPUTS:
        exp = PD.oracle_on(code, kind, batch, params, PACKED_ITERS)
        got = run(dec, device_input(kind, batch, n), PACKED_ITERS, params.product(), extra=64 // lanes)
        where = "%s batch %d %s %s" % (code, batch, params.id, kind)
        assert dec.last_kernel == "lds" and dec.last_lds_shape == (lanes, split), (where, dec.last_lds_shape)
        assert_equal(got, exp, where)


@pytest.mark.parametrize("params", SD.ET_PARAMS, ids=lambda p: p.id)
@pytest.mark.parametrize("row", SD.ET_ROWS, ids=SD.packed_id)
def test_packed_early_termination_vs_oracle(row, params):
    """Early termination with several codewords to a wave, on the saturated
    AWGN input of short_domain.et_input (test_short_domain_cpu.py: waves whose
    codewords stop at different iterations, waves that stop entirely, waves
    that never stop): iterations used, soft and hard output equal the oracle's."""
    code, batch, lanes, split = row
    llr = SD.et_input(code, batch, params)
    exp = PD.oracle_decode(code, ("short_et", batch, params.id), llr, params, SD.ET_ITERS, early=True)
    assert all(SD.et_conditions(exp[2], lanes, SD.ET_ITERS).values())
    dec = decoder(code, 7, max_batch=batch)
    got = run(dec, _torch().from_numpy(llr.copy()).cuda(), SD.ET_ITERS, params.product(early_term=1), extra=64 // lanes)
    assert dec.last_kernel == "lds" and dec.last_lds_shape == (lanes, split), dec.last_lds_shape
    assert_equal(got, exp, "%s batch %d %s early termination" % (code, batch, params.id))


@pytest.mark.parametrize("row", SD.ET_ROWS_F32, ids=SD.packed_id)
def test_packed_float_early_termination_vs_oracle(row):
    """The same in float: float_domain's "fine" input (dyadic, so the
    comparison is equality, the sign of a zero included, as in
    test_gpu_float_domain.py), plain min-sum, kernel 7 forced."""
    torch = _torch()
    code, batch, lanes, split = row
    x = FD.make(code, batch, "fine")
    exp = FD.oracle_on(code, batch, "fine", O.OMS, 0.0, SD.ET_ITERS_F32, early=True)
    assert all(SD.et_conditions(exp[2], lanes, SD.ET_ITERS_F32).values())
    dec = decoder(code, 7, max_batch=batch)
    d_hard = torch.full((batch, x.shape[1]), 9, dtype=torch.uint8, device="cuda")
    d_soft = torch.full((batch, x.shape[1]), 99.0, dtype=torch.float32, device="cuda")
    d_its = torch.full((batch,), -7, dtype=torch.int32, device="cuda")
    dec.decode_f32_device(torch.from_numpy(x.copy()).cuda(), d_hard, SD.ET_ITERS_F32,
                          params=default_params(algo=ALGO_MS, beta=0.0, early_term=1), soft=d_soft, iters_used=d_its)
    torch.cuda.synchronize()
    assert dec.last_kernel == "lds" and dec.last_lds_shape == (lanes, split), dec.last_lds_shape
    assert_same((d_hard.cpu().numpy(), d_soft.cpu().numpy(), d_its.cpu().numpy()), exp,
                "%s batch %d float early termination" % (code, batch), bitwise=True)


NM_PARAMS = [PD.CONTROL, PD.Params("OMS", 3, -127, 127)]


@pytest.mark.parametrize("params", NM_PARAMS, ids=lambda p: p.id)
@pytest.mark.parametrize("code,batch,ld,shape", [("816x408", 8195, 8200, (16, False)), ("1248x624", 37, 50, (64, False))])
def test_node_major_through_lds(code, batch, ld, shape, params):
    """ldpc_decode_i8_nm_async on kernel 7 (the input is transposed to
    frame-major scratch first): node-major [N][ld], the columns beyond the
    batch hold junk; a packed shape and a small one."""
    n = load_table(code).n
    exp = PD.oracle_on(code, "u128", batch, params, PACKED_ITERS)
    nm = np.full((n, ld), 77, dtype=np.int8)
    nm[:, :batch] = PD.make_input("u128", batch, n).T
    dec = decoder(code, 7, max_batch=batch)
    got = run(dec, _torch().from_numpy(nm).cuda(), PACKED_ITERS, params.product(), batch=batch, extra=3,
              node_major=True)
    assert dec.last_kernel == "lds" and dec.last_lds_shape == shape, dec.last_lds_shape
    assert_equal(got, exp, "%s node-major batch %d ld %d %s" % (code, batch, ld, params.id))


@pytest.mark.parametrize("kernel,code,batches,shapes", [
    (7, "200x100", (8195, 5, 8195), ((16, False), (64, True), (16, False))),
    (1, "648x324", (64, 3, 64), ((0, False),) * 3)], ids=["lds", "generic"])
def test_context_reuse_across_shapes(kernel, code, batches, shapes):
    """One context decodes a large batch, a small one and the large one again
    (kernel 7: packed, one codeword per wave split, packed), with different
    inputs and parameters: no state leaks between the shapes."""
    n = load_table(code).n
    dec = Decoder(Code(code), max_batch=max(batches), kernel=kernel)
    steps = zip(batches, shapes, ("u128", "ties", "u128"), (PD.CONTROL, PD.Params("OMS", 3, -127, 127), PD.CONTROL))
    for batch, shape, kind, params in steps:
        exp = PD.oracle_on(code, kind, batch, params, PACKED_ITERS)
        got = run(dec, device_input(kind, batch, n), PACKED_ITERS, params.product(), extra=1)
        assert dec.last_kernel == Decoder.KERNEL_NAMES[kernel] and dec.last_lds_shape == shape, dec.last_lds_shape
        assert_equal(got, exp, "%s kernel %d batch %d" % (code, kernel, batch))
    dec.close()
