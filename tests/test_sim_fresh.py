"""ldpc_sim -encoder -fresh: new information bits, encoded on the GPU, for
every frame (the reference's per-frame chain, code/x86/main_p.cpp:431-445)."""
import pytest

from test_sim_driver import points, run

pytestmark = pytest.mark.gpu


def test_sim_fresh_codewords_early_termination():
    r = run(["-code", "dvbs2_r1_2", "-min", "1.3", "-max", "1.3", "-iter", "50", "-fer", "10", "-frames", "4096",
             "-batch", "4096", "-encoder", "-fresh", "-et"])
    assert r.returncode == 0, r.stderr
    (p,) = points(r.stdout)
    assert p["frames"] >= 4096
    assert p["frame_errors"] <= 4                      # the pooled run's bound at this point


def test_sim_fresh_needs_encoder():
    r = run(["-code", "dvbs2_r1_2", "-min", "1.3", "-max", "1.3", "-fresh"])
    assert r.returncode == 2
    assert "-fresh" in r.stderr and "-encoder" in r.stderr


def test_sim_fresh_unsupported_code():
    r = run(["-code", "576x288", "-min", "1", "-max", "1", "-iter", "2", "-encoder", "-fresh"])
    assert r.returncode != 0
    assert "not built from a DVB-S2 table" in r.stderr
