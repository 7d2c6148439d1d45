"""ldpc_sim -f16: float channel -> binary16 conversion -> binary16 decode ->
error count.  One small run (dvbs2_r1_2, 64 frames) counts exactly the bit and
frame errors the binding's chain counts on the same channel samples; -f16 with
-f32, -f32q or -BP is a usage error."""
import numpy as np
import pytest

from ldpcgputegra_amd import ALGO_NMS, Code, Decoder, channel, default_params
from test_sim_driver import points, run

pytestmark = pytest.mark.gpu

CODE, FRAMES, ITERS, EBN0, BETA, SEED = "dvbs2_r1_2", 64, 8, 1.0, 0.8125, 5


def binding_counts(early):
    import torch
    code = Code(CODE)
    n, k = code.n, code.k_info
    sigma = channel.sigma_from_ebn0(EBN0, k / n)
    dec = Decoder(code, max_batch=FRAMES)
    y = torch.empty((FRAMES, n), dtype=torch.float32, device="cuda")
    h = torch.empty((FRAMES, n), dtype=torch.float16, device="cuda")
    hard = torch.empty((FRAMES, n), dtype=torch.uint8, device="cuda")
    counts = torch.zeros(2, dtype=torch.int64, device="cuda")
    dec.awgn_f32_device(y, 0, SEED, sigma)
    dec.convert_f16_device(y, h)
    dec.decode_f16_device(h, hard, ITERS, params=default_params(algo=ALGO_NMS, beta=BETA, early_term=int(early)))
    dec.count_errors_device(hard, k, counts)
    torch.cuda.synchronize()
    assert dec.last_kernel == "stairf"
    # the conversion on the device is the host's
    assert np.array_equal(h.cpu().numpy().view(np.uint16), channel.convert_f16_host(y.cpu().numpy()).view(np.uint16))
    be, fe = (int(v) for v in counts.cpu().numpy())
    dec.close()
    return be, fe


@pytest.mark.parametrize("early", (False, True), ids=("full", "et"))
def test_f16_counts_what_the_binding_counts(early):
    r = run(["-code", CODE, "-f16", "-NMS", "26", "-beta", str(BETA), "-iter", str(ITERS), "-min", str(EBN0), "-max",
             str(EBN0), "-seed", str(SEED), "-frames", str(FRAMES), "-batch", str(FRAMES), "-fer", "1000000"] +
            (["-et"] if early else []))
    assert r.returncode == 0, r.stderr
    (p,) = points(r.stdout)
    assert p["chain"] == "f16" and p["algo"] == "NMS" and p["frames"] == FRAMES
    be, fe = binding_counts(early)
    assert (p["bit_errors"], p["frame_errors"]) == (be, fe)
    assert 0 < fe < FRAMES or be > 0, "the point leaves nothing to compare"


@pytest.mark.parametrize("other", ("-f32", "-f32q", "-BP"))
def test_f16_excludes_the_other_chains(other):
    r = run(["-code", CODE, "-f16", other])
    assert r.returncode == 2
    assert "-f16" in r.stderr
