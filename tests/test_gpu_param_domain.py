"""The staircase (DVB-S2) int8 kernels over the whole LLR range and the
parameter domain the C-ABI accepts (param_domain.py): coop3_decode<7 | 10 | 14 |
22 | 27 | 30>, coop, windowed2, windowed and generic, forced one by one, on
full-range inputs (|LLR| up to 127, -128, checks whose edges all tie at 127)
and on OMS / MS / NMS parameters at and beyond the bounds of the four
*_params_ok predicates -- hard and soft output bit for bit against the oracle,
hard decisions against the reference's own SSE decoder where it is built
(r1/2, r8/9, r9/10).  test_param_domain_cpu.py shows the two checkers agree
over this domain, so a mismatch here is a kernel or dispatch bug.

Shape: batch 32, 4 iterations.  The codes are N = 64800 by construction, a
coop3 workgroup is 16 codewords, 32 is ragged against the 64-codeword pitch:
two workgroups must be as correct as a chip full of them.

A forced kernel may answer LDPC_EUNSUPPORTED "not applicable" only for the
(kernel, parameters) pairs of NOT_APPLICABLE, a table written from reading
coop_params_ok, coop3_params_ok, windowed_params_ok and windowed2_params_ok --
not built by calling them: a test that quietly skipped everything would hide a
failure."""
import numpy as np
import pytest

import oracle as O
import param_domain as PD
from ldpcgputegra_amd import Code, Decoder, LdpcError, _lib, default_params, load_table
from test_gpu_parity import kernels_for

pytestmark = pytest.mark.gpu

CODES = ["dvbs2_r1_2", "dvbs2_r2_3", "dvbs2shape_r3_4", "dvbs2shape_r5_6", "dvbs2_r8_9", "dvbs2_r9_10"]   # degree 7 .. 30
SHORT = "16200x7560"                                                                                         # generic only
BATCH, ITERS = 32, 4
# kernel families per code (what kernels_for gives, pinned here so none drops out unnoticed): windowed (2) is
# built for first-group degrees 7 and 10 only, coop (5) for 7 .. 22, windowed2 (3) and coop3 (8) for all six;
# 16200x7560 has no window plan and runs the generic kernel
KERNELS = {"dvbs2_r1_2": [1, 2, 3, 5, 8], "dvbs2_r2_3": [1, 2, 3, 5, 8], "dvbs2shape_r3_4": [1, 3, 5, 8],
           "dvbs2shape_r5_6": [1, 3, 5, 8], "dvbs2_r8_9": [1, 3, 8], "dvbs2_r9_10": [1, 3, 8], SHORT: [1]}

# kernels that refuse a parameter set (every other forced kernel must run):
#   windowed  (2): var_min -127 .. 0, msg_max 0 .. 127, OMS offset 0 .. 127, NMS factor 0 .. 255, MS
#   windowed2 (3), coop (5): OMS / MS only, var_min -127, msg_max 0 .. 63, OMS offset 0 .. 63
#   coop3     (8): as coop, and NMS with var_min -127, msg_max 0 .. 63, factor 0 .. 64
#   generic   (1): everything check_params lets through
_P = PD.Params
NOT_APPLICABLE = {
    _P("OMS", 0, -127, 63): set(), _P("OMS", 63, -127, 63): set(), _P("OMS", 31, -127, 31): set(),
    _P("OMS", 32, -127, 31): set(), _P("OMS", 5, -127, 0): set(), _P("OMS", 0, -127, 1): set(),
    _P("OMS", 1, -127, 31): set(), _P("MS", 0, -127, 31): set(), _P("MS", 0, -127, 63): set(),
    _P("NMS", 0, -127, 63): {3, 5}, _P("NMS", 1, -127, 63): {3, 5}, _P("NMS", 32, -127, 63): {3, 5},
    _P("NMS", 33, -127, 63): {3, 5}, _P("NMS", 64, -127, 63): {3, 5}, _P("NMS", 64, -127, 31): {3, 5},
    _P("OMS", 3, -127, 127): {3, 5, 8}, _P("OMS", 1, -128, 31): {2, 3, 5, 8}, _P("OMS", 64, -127, 63): {3, 5, 8},
    _P("OMS", 1, -64, 31): {3, 5, 8}, _P("NMS", 65, -127, 63): {3, 5, 8}, _P("NMS", 255, -127, 127): {3, 5, 8},
}

_decoders = {}
_device_inputs = {}


def decoder(code, kernel):
    if (code, kernel) not in _decoders:
        _decoders[(code, kernel)] = Decoder(Code(code), max_batch=64, kernel=kernel)
    return _decoders[(code, kernel)]


def _torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def device_input(kind, n):
    if (kind, n) not in _device_inputs:
        _device_inputs[(kind, n)] = _torch().from_numpy(PD.make_input(kind, BATCH, n).copy()).cuda()
    return _device_inputs[(kind, n)]


def run(dec, d_llr, iters, params, nm_batch=None):
    """(hard, soft, iters_used) of one device decode; LdpcError passes through."""
    torch = _torch()
    B = nm_batch or d_llr.shape[0]
    n = dec.code.n
    d_hard = torch.full((B, n), 9, dtype=torch.uint8, device="cuda")
    d_soft = torch.full((B, n), 99, dtype=torch.int8, device="cuda")
    d_its = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    if nm_batch:
        dec.decode_i8_nm_device(d_llr, d_hard, iters, batch=B, params=params, soft=d_soft, iters_used=d_its)
    else:
        dec.decode_i8_device(d_llr, d_hard, iters, params=params, soft=d_soft, iters_used=d_its)
    torch.cuda.synchronize()
    return d_hard.cpu().numpy(), d_soft.cpu().numpy(), d_its.cpu().numpy()


def assert_equal(got, exp, what, where):
    diff = int((got != exp).sum())
    assert diff == 0, "%s: %d %s values differ from the oracle" % (where, diff, what)


def test_tables_cover_the_grid():
    assert set(NOT_APPLICABLE) == set(PD.GRID)
    assert all(not NOT_APPLICABLE[p] - {3, 5} for p in PD.IN_DOMAIN)           # in the domain: coop3 and windowed run,
    assert all(not NOT_APPLICABLE[p] for p in PD.IN_DOMAIN if p.algo != "NMS")  # and for OMS / MS every kernel
    assert all(8 in NOT_APPLICABLE[p] for p in PD.OUT_OF_DOMAIN)
    for code in CODES + [SHORT]:
        assert kernels_for(code) == KERNELS[code], code


@pytest.mark.parametrize("params", PD.GRID, ids=lambda p: p.id)
@pytest.mark.parametrize("code", CODES + [SHORT])
def test_forced_kernels_vs_oracle(code, params):
    """Every kernel family of the code, forced, on the four full-range inputs:
    soft and hard output equal the oracle's; exactly the kernels of
    NOT_APPLICABLE refuse.  Inside the fast kernels' domain the automatic
    choice (kernel 0) runs too and is coop3 with nothing skipped; outside it,
    test_dispatch_boundary checks the fallback."""
    n = load_table(code).n
    refused, ran = set(), set()
    auto = [0] if code != SHORT and params in PD.IN_DOMAIN else []
    for kind in PD.INPUTS:
        exp_hard, exp_soft, _ = PD.oracle_on(code, kind, BATCH, params, ITERS)
        if O.ref_available(code):
            ref = PD.ref_decode(code, PD.make_input(kind, BATCH, n), params, ITERS)
            assert_equal(exp_hard, ref, "reference hard", kind)
        for k in KERNELS[code] + auto:
            dec = decoder(code, k)
            try:
                hard, soft, its = run(dec, device_input(kind, n), ITERS, params.product())
            except LdpcError as e:
                assert e.status == _lib.LDPC_EUNSUPPORTED and "not applicable" in str(e), (k, str(e))
                refused.add(k)
                continue
            ran.add(k)
            where = "%s kernel %d (%s)" % (kind, k, dec.last_kernel)
            assert_equal(soft, exp_soft, "soft", where)
            assert_equal(hard, exp_hard, "hard", where)
            assert (its == ITERS).all(), where
            if k:
                assert dec.last_kernel == Decoder.KERNEL_NAMES[k], where
            else:
                assert dec.last_kernel == "coop3" and dec.last_skipped is None, where
    assert refused == NOT_APPLICABLE[params] & set(KERNELS[code]), (sorted(refused), sorted(ran))
    assert ran == set(KERNELS[code] + auto) - refused


@pytest.mark.parametrize("params", PD.OUT_OF_DOMAIN, ids=lambda p: p.id)
@pytest.mark.parametrize("code", ["dvbs2_r1_2", "dvbs2_r8_9"])
def test_dispatch_boundary(code, params):
    """Outside the fast kernels' domain the automatic choice falls back, says
    which kernel it skipped and equals the oracle (what
    test_fast_kernel_fallback_is_reported shows for msg_max = 100); coop3
    forced raises; default parameters afterwards run coop3 again."""
    n = load_table(code).n
    d_llr = device_input("ext", n)
    exp_hard, exp_soft, _ = PD.oracle_on(code, "ext", BATCH, params, ITERS)
    dec = decoder(code, 0)
    hard, soft, _ = run(dec, d_llr, ITERS, params.product())
    assert dec.last_kernel in ("windowed", "generic") and dec.last_skipped == "coop3"   # none of the 63-bound kernels
    assert_equal(soft, exp_soft, "soft", dec.last_kernel)
    assert_equal(hard, exp_hard, "hard", dec.last_kernel)
    with pytest.raises(LdpcError) as e:
        run(decoder(code, 8), d_llr, ITERS, params.product())
    assert e.value.status == _lib.LDPC_EUNSUPPORTED
    run(dec, d_llr, ITERS, PD.CONTROL.product())
    assert dec.last_kernel == "coop3" and dec.last_skipped is None


# ---- early termination under non-default parameters ------------------------

ET_BATCH, ET_ITERS = 32, 16
ET_PARAMS = [PD.Params("OMS", 4, -127, 63), PD.Params("MS", 0, -127, 63), PD.Params("NMS", 64, -127, 63)]
# the input is param_domain.et_input: the recipe per code (Eb/N0 margin, scale-and-clip) is recorded there


def et_oracle(code, params):
    """The oracle's early-terminated decode of the saturated input, after checking
    on the oracle alone that the input converges, spreads and saturates."""
    llr = PD.et_input(code, ET_BATCH)
    eh, es, eit = PD.oracle_decode(code, ("et", ET_BATCH), llr, params, ET_ITERS, early=True)
    assert eit.min() < ET_ITERS
    assert eit.max() > eit.min()
    assert (np.abs(llr.astype(np.int32)) == 127).mean() >= 0.10
    return llr, eh, es, eit


@pytest.mark.parametrize("params", ET_PARAMS, ids=lambda p: p.id)
@pytest.mark.parametrize("code", CODES)
def test_coop3_early_termination_vs_oracle(code, params):
    """coop3's in-kernel early termination (one launch) on a saturated input:
    iterations used, soft and hard output equal the oracle's."""
    llr, eh, es, eit = et_oracle(code, params)
    dec = decoder(code, 8)
    hard, soft, its = run(dec, _torch().from_numpy(llr.copy()).cuda(), ET_ITERS, params.product(early_term=1))
    assert dec.last_kernel == "coop3" and dec.last_et_stage == 0
    assert np.array_equal(its, eit), (its.tolist(), eit.tolist())
    assert_equal(soft, es, "soft", "coop3 ET")
    assert_equal(hard, eh, "hard", "coop3 ET")


def test_coop3_staged_early_termination_vs_oracle(monkeypatch):
    """Staged early termination (compaction of the codewords still decoding)
    on a two-lanes-per-check code under plain MS, msg_max 63, forced at this
    small batch as in test_r23_staged_early_termination_vs_oracle."""
    code, params = "dvbs2_r8_9", ET_PARAMS[1]
    llr, eh, es, eit = et_oracle(code, params)
    k1 = int(np.percentile(eit, 30))
    assert 0 < k1 < ET_ITERS and (eit > k1).any()
    monkeypatch.setenv("LDPC_COOP3_ET_STAGE_MIN", "0")
    monkeypatch.setenv("LDPC_COOP3_ET_K", str(k1))
    monkeypatch.setenv("LDPC_COOP3_ET_STEP", "3")
    dec = decoder(code, 8)
    hard, soft, its = run(dec, _torch().from_numpy(llr.copy()).cuda(), ET_ITERS, params.product(early_term=1))
    assert dec.last_kernel == "coop3" and dec.last_et_stage == k1
    assert np.array_equal(its, eit), (its.tolist(), eit.tolist())
    assert_equal(soft, es, "soft", "coop3 staged ET")
    assert_equal(hard, eh, "hard", "coop3 staged ET")


# ---- the other entry points ------------------------------------------------

@pytest.mark.parametrize("code", ["dvbs2_r1_2", "dvbs2_r9_10"])
def test_node_major_entry_vs_oracle(code):
    """ldpc_decode_i8_nm_async, node-major input [N][50] (the unaligned byte
    path; the columns beyond the batch hold junk), OMS offset 63, msg_max 63,
    the `ext` input, every kernel family."""
    torch = _torch()
    params, ld = PD.Params("OMS", 63, -127, 63), 50
    n = load_table(code).n
    exp_hard, exp_soft, _ = PD.oracle_on(code, "ext", BATCH, params, ITERS)
    nm = np.full((n, ld), 77, dtype=np.int8)
    nm[:, :BATCH] = PD.make_input("ext", BATCH, n).T
    d_nm = torch.from_numpy(nm).cuda()
    for k in KERNELS[code] + [0]:
        dec = decoder(code, k)
        hard, soft, _ = run(dec, d_nm, ITERS, params.product(), nm_batch=BATCH)
        where = "kernel %d (%s)" % (k, dec.last_kernel)
        assert dec.last_kernel == Decoder.KERNEL_NAMES[k or 8], where
        assert_equal(soft, exp_soft, "soft", where)
        assert_equal(hard, exp_hard, "hard", where)


def test_mixed_decoder_vs_oracle():
    """MixedDecoder over r1/2, shaped r3/4 and shaped r5/6 (degrees 7, 14,
    22), the saturated `sat_flip` input, default parameters: every codeword
    equals the oracle's decode under its own code."""
    torch = _torch()
    from ldpcgputegra_amd.decoder import MixedDecoder
    names = ["dvbs2_r1_2", "dvbs2shape_r3_4", "dvbs2shape_r5_6"]
    llr = PD.make_input("sat_flip", BATCH, 64800)
    ids = (np.arange(BATCH, dtype=np.int32) * 7 + 1) % 3            # 11 / 11 / 10 codewords, interleaved
    mx = MixedDecoder(names, max_batch=64)
    d_hard = torch.full((BATCH, 64800), 9, dtype=torch.uint8, device="cuda")
    d_its = torch.full((BATCH,), -7, dtype=torch.int32, device="cuda")
    mx.decode_i8_device(device_input("sat_flip", 64800), d_hard, ids, ITERS, params=default_params(), iters_used=d_its)
    torch.cuda.synchronize()
    assert mx.last_kernels() == ["coop3"] * 3
    hard, its = d_hard.cpu().numpy(), d_its.cpu().numpy()
    mx.close()
    for c, name in enumerate(names):
        sel = np.where(ids == c)[0]
        assert sel.size >= 10
        eh, _, _ = PD.oracle_decode(name, ("sat_flip", BATCH, "mixed", c), llr[sel], PD.CONTROL, ITERS)
        assert_equal(hard[sel], eh, "hard", name)
        assert (its[sel] == ITERS).all(), name
