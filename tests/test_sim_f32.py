"""ldpc_sim's float chains: -f32 (float channel -> float decode with the fused
error count) and -f32q (float channel -> quantiser -> int8 decode, the
reference's chain stage by stage), beside the default chain that draws the
quantised LLRs directly.  All three see the same noise."""
import pytest

from awgn_f32_domain import SIM_EBN0, SIM_FRAMES, SIM_SEED
from test_sim_driver import points, run

pytestmark = pytest.mark.gpu


def test_f32_waterfall():
    r = run(["-code", "648x324", "-f32", "-MS", "-iter", "20", "-min", "1", "-max", "3", "-pas", "1",
             "-frames", "8192", "-batch", "1024"])
    assert r.returncode == 0, r.stderr
    pts = points(r.stdout)
    assert [round(p["ebn0"], 2) for p in pts] == [1.0, 2.0, 3.0]
    for p in pts:
        assert p["chain"] == "f32"
        assert 0 <= p["frame_errors"] <= p["frames"]
        assert p["bit_errors"] >= p["frame_errors"]
    ber = [p["bit_errors"] / p["frames"] for p in pts]
    assert ber[0] > ber[1] >= ber[2] and ber[0] > 0     # the waterfall


def test_f32q_counts_what_the_default_chain_counts():
    """Fixed frames (the -fer limit is out of reach), one point, and a seed for
    which test_awgn_f32_cpu.test_sim_seed_has_no_cell_edge_sample shows the two
    host twins agree on every byte of these frames: the device chains are
    bit-equal to them, so the two decodes see the same LLRs."""
    common = ["-code", "648x324", "-iter", "20", "-min", str(SIM_EBN0), "-max", str(SIM_EBN0), "-seed",
              str(SIM_SEED), "-frames", str(SIM_FRAMES), "-batch", "1024", "-fer", "1000000"]
    got = {}
    for chain, flag in (("i8", []), ("f32q", ["-f32q"])):
        r = run(common + flag)
        assert r.returncode == 0, r.stderr
        (p,) = points(r.stdout)
        assert p["chain"] == chain and p["frames"] == SIM_FRAMES
        got[chain] = (p["frames"], p["frame_errors"], p["bit_errors"])
    assert got["f32q"] == got["i8"]
    assert got["i8"][1] > 0                              # the point leaves frame errors to compare


# dvbs2_r1_2 at 1.3 dB, the float default (OMS, beta 0.15), 20 iterations, 1024 fresh codewords: the first run
# gave 0 frame errors (plain MS, -MS, is below its threshold there: 1024 of 1024)
FRESH_FE_FIRST_RUN = 0
FRESH_FE_BOUND = 2


def test_f32_fresh_codewords_early_termination():
    r = run(["-code", "dvbs2_r1_2", "-f32", "-encoder", "-fresh", "-et", "-iter", "20", "-min", "1.3", "-max", "1.3",
             "-frames", "1024", "-batch", "1024"])
    assert r.returncode == 0, r.stderr
    (p,) = points(r.stdout)
    assert p["chain"] == "f32" and p["frames"] == 1024
    assert p["frame_errors"] <= FRESH_FE_BOUND
    assert p["bit_errors"] >= p["frame_errors"]


def test_f32_and_f32q_exclude_each_other():
    r = run(["-code", "648x324", "-f32", "-f32q"])
    assert r.returncode == 2
    assert "-f32 " in r.stderr and "-f32q" in r.stderr
