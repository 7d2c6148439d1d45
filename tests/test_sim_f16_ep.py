"""ldpc_sim -f16 -f16ep: the binary16 chain on the edge-parallel kernel of the
short QC codes.  One small run (648x324, 64 frames) counts exactly the bit and
frame errors the binding's chain counts on the same channel samples, with and
without -f16all; -f16ep without -f16 is a usage error."""
import pytest

from ldpcgputegra_amd import ALGO_OMS, Code, Decoder, channel, default_params
from test_sim_driver import points, run

pytestmark = pytest.mark.gpu

CODE, FRAMES, ITERS, EBN0, BETA, SEED = "648x324", 64, 8, 1.5, 0.375, 5
_counts = {}


def binding_counts(early):
    if early not in _counts:
        import torch
        code = Code(CODE)
        n, k = code.n, code.k_info
        sigma = channel.sigma_from_ebn0(EBN0, k / n)
        dec = Decoder(code, max_batch=FRAMES, f16_edge_parallel=True)
        y = torch.empty((FRAMES, n), dtype=torch.float32, device="cuda")
        h = torch.empty((FRAMES, n), dtype=torch.float16, device="cuda")
        hard = torch.empty((FRAMES, n), dtype=torch.uint8, device="cuda")
        counts = torch.zeros(2, dtype=torch.int64, device="cuda")
        dec.awgn_f32_device(y, 0, SEED, sigma)
        dec.convert_f16_device(y, h)
        dec.decode_f16_device(h, hard, ITERS, params=default_params(algo=ALGO_OMS, beta=BETA, early_term=int(early)))
        dec.count_errors_device(hard, k, counts)
        torch.cuda.synchronize()
        assert dec.last_kernel == "ldsep"
        _counts[early] = tuple(int(v) for v in counts.cpu().numpy())
        dec.close()
    return _counts[early]


def _args(early, all_codes, kernel):
    return ["-code", CODE, "-f16", "-f16ep"] + (["-f16all"] if all_codes else []) + \
        ["-OMS", "1", "-beta", str(BETA), "-iter", str(ITERS), "-min", str(EBN0), "-max", str(EBN0), "-seed", str(SEED),
         "-frames", str(FRAMES), "-batch", str(FRAMES), "-fer", "1000000", "-kernel", str(kernel)] + \
        (["-et"] if early else [])


@pytest.mark.parametrize("early,all_codes,kernel", ((False, False, 0), (True, False, 9), (True, True, 0)),
                         ids=("full", "et_forced", "et_f16all"))
def test_f16ep_counts_what_the_binding_counts(early, all_codes, kernel):
    r = run(_args(early, all_codes, kernel))
    assert r.returncode == 0, r.stderr
    (p,) = points(r.stdout)
    assert p["chain"] == "f16" and p["algo"] == "OMS" and p["frames"] == FRAMES
    assert p["f16_edge_parallel"] is True and p["f16_all_codes"] is all_codes
    be, fe = binding_counts(early)
    assert (p["bit_errors"], p["frame_errors"]) == (be, fe)
    assert 0 < fe < FRAMES or be > 0, "the point leaves nothing to compare"


def test_f16ep_needs_f16():
    r = run(["-code", CODE, "-f16ep"])
    assert r.returncode == 2
    assert "-f16ep" in r.stderr and "-f16" in r.stderr
