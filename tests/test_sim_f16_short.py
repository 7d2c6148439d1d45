"""ldpc_sim -f16 -f16all: the binary16 chain on a code without a staircase.  One
small run (648x324, 64 frames) counts exactly the bit and frame errors the
binding's chain counts on the same channel samples; without -f16all the code is
refused, and -f16all without -f16 is a usage error."""
import pytest

from ldpcgputegra_amd import ALGO_OMS, Code, Decoder, channel, default_params
from test_sim_driver import points, run

pytestmark = pytest.mark.gpu

CODE, FRAMES, ITERS, EBN0, BETA, SEED = "648x324", 64, 8, 1.5, 0.375, 5


def binding_counts(early, kernel):
    import torch
    code = Code(CODE)
    n, k = code.n, code.k_info
    sigma = channel.sigma_from_ebn0(EBN0, k / n)
    dec = Decoder(code, max_batch=FRAMES, kernel=kernel, f16_all_codes=True)
    y = torch.empty((FRAMES, n), dtype=torch.float32, device="cuda")
    h = torch.empty((FRAMES, n), dtype=torch.float16, device="cuda")
    hard = torch.empty((FRAMES, n), dtype=torch.uint8, device="cuda")
    counts = torch.zeros(2, dtype=torch.int64, device="cuda")
    dec.awgn_f32_device(y, 0, SEED, sigma)
    dec.convert_f16_device(y, h)
    dec.decode_f16_device(h, hard, ITERS, params=default_params(algo=ALGO_OMS, beta=BETA, early_term=int(early)))
    dec.count_errors_device(hard, k, counts)
    torch.cuda.synchronize()
    assert dec.last_kernel == ("generic" if kernel == 1 else "lds")
    be, fe = (int(v) for v in counts.cpu().numpy())
    dec.close()
    return be, fe


def _args(early, kernel, switch=True):
    return ["-code", CODE, "-f16"] + (["-f16all"] if switch else []) + \
        ["-OMS", "1", "-beta", str(BETA), "-iter", str(ITERS), "-min", str(EBN0), "-max", str(EBN0), "-seed", str(SEED),
         "-frames", str(FRAMES), "-batch", str(FRAMES), "-fer", "1000000", "-kernel", str(kernel)] + \
        (["-et"] if early else [])


@pytest.mark.parametrize("early,kernel", ((False, 0), (True, 0), (True, 1)), ids=("full", "et", "et_generic"))
def test_f16all_counts_what_the_binding_counts(early, kernel):
    r = run(_args(early, kernel))
    assert r.returncode == 0, r.stderr
    (p,) = points(r.stdout)
    assert p["chain"] == "f16" and p["algo"] == "OMS" and p["frames"] == FRAMES and p["f16_all_codes"] is True
    be, fe = binding_counts(early, kernel)
    assert (p["bit_errors"], p["frame_errors"]) == (be, fe)
    assert 0 < fe < FRAMES or be > 0, "the point leaves nothing to compare"


def test_without_the_switch_the_code_is_refused():
    r = run(_args(False, 0, switch=False))
    assert r.returncode != 0 and "staircase" in r.stderr


def test_f16all_needs_f16():
    r = run(["-code", CODE, "-f16all"])
    assert r.returncode == 2
    assert "-f16all" in r.stderr and "-f16" in r.stderr
