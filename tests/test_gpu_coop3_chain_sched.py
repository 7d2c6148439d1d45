"""The order in which coop3's waves issue their instructions is tuned by hand:
where the chain wave reads a block's constants and waits for them
(chain_window3: one or, at degree 10, two blocks of 8 steps ahead), and the
degree-7 post running new_v of its six edges stage by stage
(LDPC_C3_POST_STAGE7).  Such changes only reorder instructions, so everything
here is bit for bit against the oracle (soft output and hard decisions):

* every step position: each chain variant (OMS / NMS, constants one block
  ahead / two at degree 10) over codes of 6, 4, 4 and 2 blocks of 8 steps per
  window, at 1 iteration (a constant read too early or used before it landed
  shows at once) and 2 (non-zero messages); a mismatch is reported as the
  first parity row that differs = (window, chain step);
* repeatable: four launches on one input give identical outputs (a wait that
  is missing only sometimes shows as a difference between launches);
* the edges of the LLR range: ties and both clamps in the restaged post."""
import numpy as np
import pytest

import oracle as O
from ldpcgputegra_amd import ALGO_NMS, Code, Decoder, channel, default_params, load_table

pytestmark = pytest.mark.gpu
# code -> (Eb/N0, checks per window S, window distance): G3<D0>::S / DIST of coop3_kernel.h
CODES = {"dvbs2_r1_2": (1.0, 48, 1), "dvbs2_r2_3": (1.9, 32, 1), "dvbs2shape_r3_4": (2.35, 32, 1),
         "dvbs2_r9_10": (4.4, 16, 2)}
ALGOS = {"oms1": (O.OMS, 1, dict()), "nms24": (O.NMS, 24, dict(algo=ALGO_NMS, factor=24))}


@pytest.fixture(scope="module")
def decoders():
    made = {}

    def get(CODE, max_batch=64):
        if (CODE, max_batch) not in made:
            made[CODE, max_batch] = Decoder(Code(CODE), max_batch=max_batch, kernel=8)
        return made[CODE, max_batch]
    yield get
    for d in made.values():
        d.close()


def _run(dec, llr, iters, params):
    import torch
    B, n = llr.shape
    d_hard = torch.empty((B, n), dtype=torch.uint8, device="cuda")
    d_soft = torch.empty((B, n), dtype=torch.int8, device="cuda")
    dec.decode_i8_device(torch.from_numpy(llr).cuda(), d_hard, iters, params=params, soft=d_soft)
    torch.cuda.synchronize()
    assert dec.last_kernel == "coop3"
    return d_hard.cpu().numpy(), d_soft.cpu().numpy()


def _llr(CODE, B, seed):
    t = load_table(CODE)
    return channel.awgn_i8_host(t.n, B, seed=seed, table=channel.i8_table(channel.sigma_from_ebn0(CODES[CODE][0], t.k_info / t.n)))


def _where(CODE, soft, exp):
    """The first parity row that differs as (codeword, window, chain step):
    parity row j is written by chain step j - first of the window holding
    check j."""
    t = load_table(CODE)
    k = t.n - t.m
    bad = np.argwhere(soft[:, k:] != exp[:, k:])
    if bad.size == 0:
        return "no parity row differs; %d information values do" % int((soft != exp).sum())
    j = int(bad[:, 1].min())
    cw = int(bad[bad[:, 1] == j][0, 0])
    _, S, dist = CODES[CODE]
    plan = Code(CODE).coop_plan(S=S, R=4, dist=dist)
    for u, (first, count) in enumerate(plan["windows"]):
        if first <= j < first + count:
            return "first differing parity row %d (codeword %d): window %d, chain step %d" % (j, cw, u, j - first)
    return "first differing parity row %d (codeword %d): the tail check, window %d" % (j, cw, plan["tail"])


@pytest.mark.parametrize("iters", [1, 2])
@pytest.mark.parametrize("batch", [16, 17])
@pytest.mark.parametrize("algo", list(ALGOS))
@pytest.mark.parametrize("CODE", list(CODES))
def test_every_chain_step_position_vs_oracle(decoders, CODE, algo, batch, iters):
    t = load_table(CODE)
    oalgo, oparam, kw = ALGOS[algo]
    llr = _llr(CODE, batch, 100 + batch)
    eh, es, _ = O.decode_i8(t, llr, iters, oalgo, oparam, return_soft=True, threads=O.host_threads())
    h, s = _run(decoders(CODE), llr, iters, default_params(**kw))
    if not np.array_equal(s, es):
        pytest.fail(_where(CODE, s, es))
    assert np.array_equal(h, eh)


def test_four_launches_on_one_input_are_identical(decoders):
    CODE, B, iters = "dvbs2_r1_2", 512, 10
    t = load_table(CODE)
    llr = _llr(CODE, B, 7)
    dec = decoders(CODE, 512)
    runs = [_run(dec, llr, iters, default_params()) for _ in range(4)]
    for i in range(1, 4):
        assert np.array_equal(runs[i][1], runs[0][1]), "launch %d: %s" % (i, _where(CODE, runs[i][1], runs[0][1]))
        assert np.array_equal(runs[i][0], runs[0][0]), i
    eh, es, _ = O.decode_i8(t, llr[:64], iters, return_soft=True, threads=O.host_threads())
    if not np.array_equal(runs[0][1][:64], es):
        pytest.fail(_where(CODE, runs[0][1][:64], es))
    assert np.array_equal(runs[0][0][:64], eh)


@pytest.mark.parametrize("pattern", ["plus127", "minus127", "zero", "alternating"])
@pytest.mark.parametrize("CODE", ["dvbs2_r1_2", "dvbs2_r2_3"])
def test_llr_range_edges_vs_oracle(decoders, CODE, pattern):
    """All +127 / all -127 (both clamps), all 0 (every minimum tied) and
    +127 / -127 alternating along the codeword, 3 iterations."""
    t = load_table(CODE)
    B, iters = 16, 3
    llr = np.zeros((B, t.n), dtype=np.int8)
    if pattern == "plus127":
        llr[:] = 127
    elif pattern == "minus127":
        llr[:] = -127
    elif pattern == "alternating":
        llr[:, 0::2] = 127
        llr[:, 1::2] = -127
    eh, es, _ = O.decode_i8(t, llr, iters, return_soft=True, threads=O.host_threads())
    h, s = _run(decoders(CODE), llr, iters, default_params())
    if not np.array_equal(s, es):
        pytest.fail(_where(CODE, s, es))
    assert np.array_equal(h, eh)
