"""ldpc_sim -BP: the float chain with belief propagation and the true-LLR
channel (norm = 2 / sigma^2), counted against the same frames decoded through
the Python binding."""
import numpy as np
import pytest

from ldpcgputegra_amd import ALGO_BP, Code, Decoder, channel, default_params
from test_sim_driver import points, run

EBN0, SEED, BATCH, FRAMES, ITERS = 2.0, 3, 256, 768, 10
COMMON = ["-code", "648x324", "-iter", str(ITERS), "-min", str(EBN0), "-max", str(EBN0), "-seed", str(SEED),
          "-frames", str(FRAMES), "-batch", str(BATCH), "-fer", "1000000"]


@pytest.mark.gpu
def test_bp_counts_what_the_binding_counts():
    """One point, three batches, the -fer limit out of reach: the simulator's
    frames are codewords 0 .. FRAMES - 1 of the all-zero codeword on the float
    channel with normalize=True, which the binding draws and decodes too."""
    import torch
    r = run(COMMON + ["-BP"])
    assert r.returncode == 0, r.stderr
    assert "| BP | chain f32 |" in r.stdout
    (p,) = points(r.stdout)
    assert p["algo"] == "BP" and p["chain"] == "f32" and p["frames"] == FRAMES
    dec = Decoder(Code("648x324"), max_batch=BATCH)
    n, k = dec.code.n, dec.code.k_info
    sigma = channel.sigma_from_ebn0(EBN0, k / n)
    y = torch.empty((BATCH, n), dtype=torch.float32, device="cuda")
    hard = torch.empty((BATCH, n), dtype=torch.uint8, device="cuda")
    be = fe = 0
    for first in range(0, FRAMES, BATCH):
        dec.awgn_f32_device(y, first, SEED, sigma, normalize=True)
        dec.decode_f32_device(y, hard, ITERS, params=default_params(algo=ALGO_BP))
        h = hard.cpu().numpy()[:, :k]
        be += int(h.sum())
        fe += int(h.any(axis=1).sum())
    assert dec.last_kernel == "lds"
    assert (p["frame_errors"], p["bit_errors"]) == (fe, be)
    assert fe > 0                                         # the point leaves frame errors to compare
    # the first batch on the host: the same frames, the same decode
    llr = channel.awgn_f32_host(n, BATCH, SEED, sigma, normalize=True)
    hh = Decoder(Code("648x324"), device=-1, max_batch=BATCH).decode_f32(llr, ITERS, default_params(algo=ALGO_BP))
    dec.awgn_f32_device(y, 0, SEED, sigma, normalize=True)
    dec.decode_f32_device(y, hard, ITERS, params=default_params(algo=ALGO_BP))
    assert np.array_equal(hard.cpu().numpy(), hh)
    dec.close()


@pytest.mark.gpu
def test_other_algorithms_are_named_too():
    r = run(COMMON + ["-f32", "-MS"])
    assert r.returncode == 0, r.stderr
    (p,) = points(r.stdout)
    assert p["algo"] == "MS" and p["chain"] == "f32"


def test_bp_excludes_the_int8_chains():
    """A usage error before any GPU work: runs without a GPU."""
    r = run(["-code", "648x324", "-BP", "-f32q"])
    assert r.returncode == 2
    assert "-BP" in r.stderr and "-f32q" in r.stderr
