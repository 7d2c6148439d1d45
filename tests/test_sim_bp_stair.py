"""ldpc_sim -BP -bpstair: belief propagation on the staircase kernel counts
the frames the Python binding counts with the switch on, and what -BP alone
(the any-H kernel) counts."""
import pytest

from ldpcgputegra_amd import ALGO_BP, Code, Decoder, channel, default_params
from test_sim_driver import points, run

EBN0, SEED, BATCH, FRAMES, ITERS = 1.0, 3, 16, 48, 3
COMMON = ["-code", "dvbs2_r1_2", "-iter", str(ITERS), "-min", str(EBN0), "-max", str(EBN0), "-seed", str(SEED),
          "-frames", str(FRAMES), "-batch", str(BATCH), "-fer", "1000000", "-BP"]


@pytest.mark.gpu
def test_bpstair_counts_what_the_binding_and_plain_bp_count():
    """One point, three batches of 16 frames, 3 iterations at 1.0 dB (every
    frame is still in error, thousands of bit errors to compare)."""
    import torch
    r = run(COMMON + ["-bpstair"])
    assert r.returncode == 0, r.stderr
    (p,) = points(r.stdout)
    assert p["algo"] == "BP" and p["chain"] == "f32" and p["frames"] == FRAMES and p["bp_staircase"] is True
    r1 = run(COMMON)
    assert r1.returncode == 0, r1.stderr
    (p1,) = points(r1.stdout)
    assert p1["bp_staircase"] is False and p1["frames"] == FRAMES
    dec = Decoder(Code("dvbs2_r1_2"), max_batch=BATCH, bp_staircase=True)
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
    assert dec.last_kernel == "stairf"
    assert (p["frame_errors"], p["bit_errors"]) == (fe, be)
    assert (p1["frame_errors"], p1["bit_errors"]) == (fe, be)
    assert fe > 0 and be > 0
    dec.close()


def test_bpstair_needs_bp():
    """A usage error before any GPU work: runs without a GPU."""
    for extra in ([], ["-f32"], ["-f32", "-MS"]):
        r = run(["-code", "dvbs2_r1_2", "-bpstair"] + extra)
        assert r.returncode == 2
        assert "-bpstair" in r.stderr and "-BP" in r.stderr
