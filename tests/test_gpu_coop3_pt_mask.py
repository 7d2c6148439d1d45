"""coop3 (kernel 8) after the slab-wave trim of DESIGN.md §8 r09: the packed
unsigned saturating subtract for max(min - offset, 0) (chain_consts,
post_finish, the tail check), eps * m_x by one packed multiply, and the pre's
pass-through block run in steady periods only by the slab waves the plan's
mask names (Coop3Args::pt_mask).

DVB-S2 r1/2: hard decisions, soft output and iterations used, bit for bit
against the oracle, at batches 1, 16, 17 and 37 (one 16-codeword group, a
group edge, a ragged last group) and 1, 2 and 3 iterations, on full-range LLRs
(-128 and 127 present), OMS offset 0, 1 and 2 and NMS factor 24 -- each decode
run twice, with the computed mask and with LDPC_COOP3_PT_ALL=1 (every wave
runs the block, as before the mask): the two results must be identical.  The
same again with early termination on (the ET kernels share the pre), and one
input whose codewords do stop early.  The changed helpers are shared by every
degree: r2/3 (first-group degree 10), the shaped r3/4 (14) and r8/9 (27: two
lanes per check, sink entries) at batch 17, 2 iterations, OMS offset 1 and NMS.

The oracle decodes the 37 codewords once per (mode, iterations, early); the
smaller batches are its first rows (codewords decode independently)."""
import numpy as np
import pytest

import param_domain as PD
from ldpcgputegra_amd import Code, Decoder, load_table

pytestmark = pytest.mark.gpu
R12 = "dvbs2_r1_2"
BATCHES = (1, 16, 17, 37)
MODES = {"oms0": PD.Params("OMS", 0, -127, 31), "oms1": PD.Params("OMS", 1, -127, 31),
         "oms2": PD.Params("OMS", 2, -127, 31), "nms24": PD.Params("NMS", 24, -127, 63)}
OTHER = ("dvbs2_r2_3", "dvbs2shape_r3_4", "dvbs2_r8_9")
ET_ITERS = 16

_dec = {}


def decoder(code):
    if code not in _dec:
        _dec[code] = Decoder(Code(code), max_batch=64, kernel=8)
    return _dec[code]


def run(code, llr, iters, params):
    """(hard, soft, iters_used) of one device decode of the host array llr."""
    import torch
    assert torch.cuda.is_available()
    dec = decoder(code)
    B, n = llr.shape
    d_hard = torch.full((B, n), 9, dtype=torch.uint8, device="cuda")
    d_soft = torch.full((B, n), 99, dtype=torch.int8, device="cuda")
    d_its = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    dec.decode_i8_device(torch.from_numpy(np.array(llr)).cuda(), d_hard, iters, params=params, soft=d_soft,
                         iters_used=d_its)
    torch.cuda.synchronize()
    assert dec.last_kernel == "coop3"
    return d_hard.cpu().numpy(), d_soft.cpu().numpy(), d_its.cpu().numpy()


def both_masks(monkeypatch, code, llr, iters, params):
    """The decode with the plan's mask and with every wave running the
    pass-through block: identical, returned once."""
    monkeypatch.delenv("LDPC_COOP3_PT_ALL", raising=False)
    a = run(code, llr, iters, params)
    monkeypatch.setenv("LDPC_COOP3_PT_ALL", "1")
    b = run(code, llr, iters, params)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    return a


@pytest.mark.parametrize("early", [False, True], ids=["fixed", "et"])
@pytest.mark.parametrize("iters", [1, 2, 3])
@pytest.mark.parametrize("batch", BATCHES)
@pytest.mark.parametrize("mode", sorted(MODES))
def test_r12_grid_vs_oracle(monkeypatch, mode, batch, iters, early):
    params = MODES[mode]
    llr = PD.make_input("u128", max(BATCHES), load_table(R12).n)
    assert llr.min() == -128 and llr.max() == 127
    eh, es, eit = PD.oracle_on(R12, "u128", max(BATCHES), params, iters, early=early)
    hard, soft, its = both_masks(monkeypatch, R12, llr[:batch], iters, params.product(early_term=int(early)))
    assert np.array_equal(soft, es[:batch])
    assert np.array_equal(hard, eh[:batch])
    assert np.array_equal(its, eit[:batch]) if early else (its == iters).all()


def test_r12_early_termination_that_stops(monkeypatch):
    """Batch 37, 16 iterations, an input whose codewords converge after
    different numbers of iterations: frozen codewords pass through the same
    pre, with either mask."""
    llr = PD.et_input(R12, 37)
    eh, es, eit = PD.oracle_decode(R12, ("et", 37), llr, PD.CONTROL, ET_ITERS, early=True)
    assert eit.min() < ET_ITERS and eit.max() > eit.min()
    hard, soft, its = both_masks(monkeypatch, R12, llr, ET_ITERS, PD.CONTROL.product(early_term=1))
    assert np.array_equal(its, eit), (its.tolist(), eit.tolist())
    assert np.array_equal(hard, eh) and np.array_equal(soft, es)


@pytest.mark.parametrize("mode", ["oms1", "nms24"])
@pytest.mark.parametrize("code", OTHER)
def test_other_degrees_vs_oracle(monkeypatch, code, mode):
    params = MODES[mode]
    llr = PD.make_input("u128", 17, load_table(code).n)
    eh, es, _ = PD.oracle_on(code, "u128", 17, params, 2)
    hard, soft, its = both_masks(monkeypatch, code, llr, 2, params.product())
    assert np.array_equal(soft, es)
    assert np.array_equal(hard, eh)
    assert (its == 2).all()
