"""ldpc_sim -i8epw: the int8 chain on the edge-parallel int8 kernel over several
waves.  One small run (1944x972, 64 frames) counts exactly the bit and frame
errors the binding's chain counts on the same channel samples with the switch
on (and with it off: one contract), with and without -et, automatic and
-kernel 9; -i8epw with -f32, -f16 or -BP is a usage error."""
import pytest

from ldpcgputegra_amd import Code, Decoder, channel, default_params
from test_sim_driver import points, run

pytestmark = pytest.mark.gpu

CODE, FRAMES, ITERS, EBN0, SEED = "1944x972", 64, 8, 1.5, 5
_counts = {}


def binding_counts(early):
    """(bit errors, frame errors) of awgn_i8_device -> decode_i8_device -> count_errors_device, the same on
    ldsepwi and on family 7"""
    if early not in _counts:
        import torch
        code = Code(CODE)
        n, k = code.n, code.k_info
        table = channel.i8_table(channel.sigma_from_ebn0(EBN0, k / n))
        out = []
        for on, family in ((True, "ldsep"), (False, "lds")):
            dec = Decoder(code, max_batch=FRAMES, i8_ep_wide=on, kernel=9 if on else 0)
            llr = torch.empty((FRAMES, n), dtype=torch.int8, device="cuda")
            hard = torch.empty((FRAMES, n), dtype=torch.uint8, device="cuda")
            counts = torch.zeros(2, dtype=torch.int64, device="cuda")
            dec.awgn_i8_device(llr, 0, SEED, table)
            dec.decode_i8_device(llr, hard, ITERS, params=default_params(early_term=int(early)))
            dec.count_errors_device(hard, k, counts)
            torch.cuda.synchronize()
            assert dec.last_kernel == family and (dec.last_ep_waves != 0) == on
            out.append(tuple(int(v) for v in counts.cpu().numpy()))
            dec.close()
        assert out[0] == out[1], "ldsepwi and family 7 count different errors"
        _counts[early] = out[0]
    return _counts[early]


def _args(early, kernel):
    return ["-code", CODE, "-i8epw", "-OMS", "1", "-iter", str(ITERS), "-min", str(EBN0), "-max", str(EBN0),
            "-seed", str(SEED), "-frames", str(FRAMES), "-batch", str(FRAMES), "-fer", "1000000",
            "-kernel", str(kernel)] + (["-et"] if early else [])


@pytest.mark.parametrize("early,kernel", ((False, 0), (False, 9), (True, 0), (True, 9)),
                         ids=("full_auto", "full_forced", "et_auto", "et_forced"))
def test_i8epw_counts_what_the_binding_counts(early, kernel):
    r = run(_args(early, kernel))
    assert r.returncode == 0, r.stderr
    (p,) = points(r.stdout)
    assert p["chain"] == "i8" and p["algo"] == "OMS" and p["frames"] == FRAMES
    assert p["i8_ep_wide"] is True and p["i8_edge_parallel"] is False and p["ep_wide"] is False
    be, fe = binding_counts(early)
    assert (p["bit_errors"], p["frame_errors"]) == (be, fe)
    assert 0 < fe < FRAMES or be > 0, "the point leaves nothing to compare"


def test_kernel_9_needs_the_switch():
    r = run([a for a in _args(False, 9) if a != "-i8epw"])
    assert r.returncode != 0


@pytest.mark.parametrize("flag", ("-f32", "-f16", "-BP"))
def test_i8epw_excludes_the_float_chains(flag):
    r = run(["-code", CODE, "-i8epw", flag])
    assert r.returncode == 2
    assert "-i8epw" in r.stderr and flag in r.stderr
