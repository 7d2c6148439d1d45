"""DVB-S2 r1/2 on coop3 (kernel 8, coop3_decode<7, 6, 2, ..>) where its slab
waves were trimmed: the pre's u16 reads of the information
edges (one line-cache address per edge), the post's paired packing of the new
V (ds_write_b16 / _d16_hi) -- and the places a trim of the first / last
iteration or of the step's side kernels would break first: a context reused
for a second decode, early termination in one launch and staged, and the
error count of ldpc_decode_i8_count_async (a separate launch on kernel 8; a
count folded into the output transpose measured slower and was not kept,
LDPC_FUSED_COUNT still only switches the float kernel's).

Shapes: batches 1, 16, 17 and 37 (one 16-codeword group, a group edge, a
ragged last group) at 1, 2 and 3 iterations (first = last, no middle, one
middle iteration), OMS offset 1 on full-range LLRs (-128 and 127 present) and
NMS factor 24 -- hard and soft output bit for bit against the oracle, hard
decisions against the reference's own SSE decoder where it is built.  The
oracle decodes the 37 codewords once per (mode, iterations); the smaller
batches are its first rows (codewords decode independently)."""
import numpy as np
import pytest

import oracle as O
import param_domain as PD
from ldpcgputegra_amd import Code, Decoder, load_table

CODE = "dvbs2_r1_2"
BATCHES = (1, 16, 17, 37)
MODES = {"oms1_fullrange": (PD.Params("OMS", 1, -127, 31), "u128"),
         "nms24": (PD.Params("NMS", 24, -127, 63), "u128")}
# modelled extra LDS bank cycles per iteration and workgroup of the r1/2 line-cache plan on the parent of the u16
# reads (Code("dvbs2_r1_2").coop3_lc_banks()["swizzled"]): a u16 read touches the dword the
# dword read did, so the plan and its model are unchanged
PARENT_LC_BANK_EXTRA = 920

_dec = {}


def _torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def decoder(tag="shared"):
    if tag not in _dec:
        _dec[tag] = Decoder(Code(CODE), max_batch=64, kernel=8)
    return _dec[tag]


def run(dec, llr, iters, params):
    """(hard, soft, iters_used) of one device decode of the host array llr."""
    torch = _torch()
    B, n = llr.shape
    d_hard = torch.full((B, n), 9, dtype=torch.uint8, device="cuda")
    d_soft = torch.full((B, n), 99, dtype=torch.int8, device="cuda")
    d_its = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    dec.decode_i8_device(torch.from_numpy(np.array(llr)).cuda(), d_hard, iters, params=params,
                         soft=d_soft, iters_used=d_its)
    torch.cuda.synchronize()
    assert dec.last_kernel == "coop3"
    return d_hard.cpu().numpy(), d_soft.cpu().numpy(), d_its.cpu().numpy()


def test_line_cache_bank_model_not_worse_than_parent():
    """1(a), no GPU: the pre's u16 read of an information edge's pair is in
    the dword the parent's ds_read_b32 read (two lanes on one dword: a
    broadcast), so the planner's bank model still describes it and reports
    no more extra cycles than on the parent."""
    b = Code(CODE).coop3_lc_banks()
    assert 0 < b["swizzled"] <= PARENT_LC_BANK_EXTRA


@pytest.mark.gpu
@pytest.mark.parametrize("iters", [1, 2, 3])
@pytest.mark.parametrize("batch", BATCHES)
@pytest.mark.parametrize("mode", sorted(MODES))
def test_grid_vs_oracle(mode, batch, iters):
    params, kind = MODES[mode]
    n = load_table(CODE).n
    llr = PD.make_input(kind, max(BATCHES), n)
    assert llr.min() == -128 and llr.max() == 127
    eh, es, _ = PD.oracle_on(CODE, kind, max(BATCHES), params, iters)
    hard, soft, its = run(decoder(), llr[:batch], iters, params.product())
    assert np.array_equal(soft, es[:batch])
    assert np.array_equal(hard, eh[:batch])
    assert (its == iters).all()
    if batch % 16 == 0 and O.ref_available(CODE):
        assert np.array_equal(PD.ref_decode(CODE, llr[:batch], params, iters), hard)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", sorted(MODES))
def test_reused_context_ignores_stale_messages(mode):
    """Decode A for 5 iterations, then B for 2 on the same context: B's result
    equals B's on a fresh context (and the oracle's), bit for bit -- the
    messages A left behind are not B's first-iteration messages."""
    params, _ = MODES[mode]
    n = load_table(CODE).n
    A, B = PD.make_input("u128", 17, n), PD.make_input("ext", 17, n)
    dec = Decoder(Code(CODE), max_batch=64, kernel=8)
    run(dec, A, 5, params.product())
    h1, s1, _ = run(dec, B, 2, params.product())
    dec.close()
    fresh = Decoder(Code(CODE), max_batch=64, kernel=8)
    h2, s2, _ = run(fresh, B, 2, params.product())
    fresh.close()
    assert np.array_equal(s1, s2) and np.array_equal(h1, h2)
    eh, es, _ = PD.oracle_on(CODE, "ext", 17, params, 2)
    assert np.array_equal(s1, es) and np.array_equal(h1, eh)


ET_ITERS = 16


def _et_case(batch):
    llr = PD.et_input(CODE, batch)
    eh, es, eit = PD.oracle_decode(CODE, ("et", batch), llr, PD.CONTROL, ET_ITERS, early=True)
    assert eit.min() < ET_ITERS and eit.max() > eit.min()
    return llr, eh, es, eit


@pytest.mark.gpu
def test_in_kernel_early_termination_vs_oracle():
    """One launch, batch 37: hard decisions and iterations used per codeword."""
    llr, eh, es, eit = _et_case(37)
    dec = decoder()
    hard, soft, its = run(dec, llr, ET_ITERS, PD.CONTROL.product(early_term=1))
    assert dec.last_et_stage == 0
    assert np.array_equal(its, eit), (its.tolist(), eit.tolist())
    assert np.array_equal(hard, eh) and np.array_equal(soft, es)


@pytest.mark.gpu
def test_staged_early_termination_vs_oracle(monkeypatch):
    """Staged early termination forced at batch 37 (the stage threshold
    lowered as test_gpu_parity's staged tests do): the later launches start
    at iter_base > 0 and must read the messages the first stage left."""
    llr, eh, es, eit = _et_case(37)
    k1 = int(np.percentile(eit, 30))
    assert 0 < k1 < ET_ITERS and (eit > k1).any()
    monkeypatch.setenv("LDPC_COOP3_ET_STAGE_MIN", "0")
    monkeypatch.setenv("LDPC_COOP3_ET_K", str(k1))
    monkeypatch.setenv("LDPC_COOP3_ET_STEP", "3")
    dec = decoder()
    hard, soft, its = run(dec, llr, ET_ITERS, PD.CONTROL.product(early_term=1))
    assert dec.last_et_stage == k1
    assert np.array_equal(its, eit), (its.tolist(), eit.tolist())
    assert np.array_equal(hard, eh) and np.array_equal(soft, es)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [32400, 32391], ids=["k_mult16", "k_odd"])
def test_decode_count_equals_known_errors(k, monkeypatch):
    """Batch 17, 3 iterations: the saturated AWGN input of the all-zero word
    (it decodes clean) with two codewords replaced by uniform noise (they
    fail).  Without a reference: the errors against the all-zero codeword,
    counted on the host from the hard decisions.  With one: the decoder's
    own output with 7 bits flipped in 3 codewords, one of them at k (outside
    the counted range) -- 6 bit errors, 3 frame errors.  The count adds into
    counts that start non-zero, twice in a row on one context, with
    LDPC_FUSED_COUNT at its default and at 0 (any count fused into a kernel-8
    side kernel has to give what the separate count launch gives)."""
    torch = _torch()
    t = load_table(CODE)
    assert t.k_info == 32400
    B, iters = 17, 3
    llr = PD.et_input(CODE, B).copy()
    llr[[3, 16]] = PD.make_input("u128", B, t.n)[[3, 16]]   # two codewords of noise: these fail
    params = PD.CONTROL.product()
    dec = decoder()
    plain, _, _ = run(dec, llr, iters, params)
    ref = plain.copy()
    flips = [(0, 0), (0, 31), (0, k - 1), (5, 64), (5, k), (16, 16199), (16, k - 17)]
    for b, i in flips:
        ref[b, i] ^= 1
    bad0 = plain[:, :k] != 0
    assert 0 < bad0.any(axis=1).sum() < B, "wanted clean and failing codewords against the all-zero word"
    expect = {None: (int(bad0.sum()), int(bad0.any(axis=1).sum())), "ref": (6, 3)}
    d_llr = torch.from_numpy(llr.copy()).cuda()
    d_ref = torch.from_numpy(ref).cuda()
    start = [1000, 7]
    for r in (None, "ref"):
        got = {}
        for fused in ("1", "0"):
            monkeypatch.setenv("LDPC_FUSED_COUNT", fused)
            cnt = torch.tensor(start, dtype=torch.int64, device="cuda")
            hard = torch.empty((B, t.n), dtype=torch.uint8, device="cuda")
            for _ in range(2):
                dec.decode_count_device(d_llr, hard, iters, k, cnt, ref=d_ref if r else None, params=params)
            torch.cuda.synchronize()
            assert dec.last_kernel == "coop3"
            assert np.array_equal(hard.cpu().numpy(), plain)
            got[fused] = cnt.tolist()
        be, fe = expect[r]
        assert got["1"] == got["0"] == [start[0] + 2 * be, start[1] + 2 * fe], (r, got, expect[r])
