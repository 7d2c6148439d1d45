"""ldpc_sim -f32 -epwide: the float chain with the longer QC codes on `ldsepw`,
the edge-parallel kernel spread over several waves.  One small run (1944x972, 64
frames) counts exactly the bit and frame errors the binding's chain counts on
the same channel samples, with the automatic choice and with family 9 forced,
and the JSON line names the switch; -epwide without -f32, or with -BP, is a
usage error."""
import pytest

from ldpcgputegra_amd import ALGO_OMS, Code, Decoder, channel, default_params
from test_sim_driver import points, run

pytestmark = pytest.mark.gpu

CODE, FRAMES, ITERS, EBN0, BETA, SEED = "1944x972", 64, 8, 1.2, 0.375, 5
_counts = {}


def binding_counts(early):
    if early not in _counts:
        import torch
        code = Code(CODE)
        n, k = code.n, code.k_info
        sigma = channel.sigma_from_ebn0(EBN0, k / n)
        dec = Decoder(code, max_batch=FRAMES, kernel=9, ep_wide=True)
        y = torch.empty((FRAMES, n), dtype=torch.float32, device="cuda")
        hard = torch.empty((FRAMES, n), dtype=torch.uint8, device="cuda")
        counts = torch.zeros(2, dtype=torch.int64, device="cuda")
        dec.awgn_f32_device(y, 0, SEED, sigma)
        dec.decode_f32_device(y, hard, ITERS, params=default_params(algo=ALGO_OMS, beta=BETA, early_term=int(early)))
        dec.count_errors_device(hard, k, counts)
        torch.cuda.synchronize()
        assert dec.last_kernel == "ldsep" and dec.last_ep_waves in (2, 4)
        _counts[early] = tuple(int(v) for v in counts.cpu().numpy())
        dec.close()
    return _counts[early]


def _args(early, kernel, epwide=True):
    return ["-code", CODE, "-f32"] + (["-epwide"] if epwide else []) + \
        ["-OMS", "1", "-beta", str(BETA), "-iter", str(ITERS), "-min", str(EBN0), "-max", str(EBN0), "-seed", str(SEED),
         "-frames", str(FRAMES), "-batch", str(FRAMES), "-fer", "1000000", "-kernel", str(kernel)] + \
        (["-et"] if early else [])


@pytest.mark.parametrize("early,kernel", ((False, 0), (True, 9), (False, 9)), ids=("full_auto", "et_forced", "full_forced"))
def test_epwide_counts_what_the_binding_counts(early, kernel):
    r = run(_args(early, kernel))
    assert r.returncode == 0, r.stderr
    (p,) = points(r.stdout)
    assert p["chain"] == "f32" and p["algo"] == "OMS" and p["frames"] == FRAMES
    assert p["ep_wide"] is True and p["f16_edge_parallel"] is False
    be, fe = binding_counts(early)
    assert (p["bit_errors"], p["frame_errors"]) == (be, fe)
    assert 0 < fe < FRAMES or be > 0, "the point leaves nothing to compare"


def test_without_the_switch():
    """the JSON line says so, the counts are the same (one float contract), and a forced 9 is refused as before"""
    r = run(_args(False, 0, epwide=False))
    assert r.returncode == 0, r.stderr
    (p,) = points(r.stdout)
    assert p["ep_wide"] is False
    assert (p["bit_errors"], p["frame_errors"]) == binding_counts(False)
    r = run(_args(False, 9, epwide=False))
    assert r.returncode != 0 and "kernel 9" in r.stderr


def test_epwide_usage_errors():
    r = run(["-code", CODE, "-epwide"])
    assert r.returncode == 2 and "-epwide" in r.stderr and "-f32" in r.stderr
    r = run(["-code", CODE, "-BP", "-epwide"])
    assert r.returncode == 2 and "-epwide" in r.stderr
