"""bench.py's command line: a plain run is the timed steps only (no CPU
baseline), --full adds the baselines, --dump-outputs writes what the last
timed step left."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NAMES = ("hard", "hard_rows", "hard_weight", "counts")


def test_dump_outputs_whole_and_sampled(tmp_path):
    """dump_outputs on host tensors: a batch that fits is written whole, a
    larger one as the same seeded sample of whole codewords every time; every
    file is float32 / float64 and the set stays under 64 MB."""
    import torch
    import bench
    n = 64800
    keep = bench.DUMP_HARD_BYTES // (4 * n)
    g = torch.Generator().manual_seed(7)
    for b, sub in ((5, "small"), (keep + 37, "large")):
        hard = torch.randint(0, 2, (b, n), dtype=torch.uint8, generator=g)
        d = str(tmp_path / sub)
        bench.dump_outputs(d, hard, {"counts": np.array([3, 1])})
        got = {k: np.load(os.path.join(d, k + ".npy")) for k in NAMES}
        assert sorted(os.listdir(d)) == sorted(k + ".npy" for k in NAMES)
        assert all(v.dtype in (np.float32, np.float64) for v in got.values())
        assert sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d)) <= 64 * 10**6
        rows = got["hard_rows"].astype(np.int64)
        assert rows.size == min(b, keep) and np.all(np.diff(rows) > 0) and rows[0] >= 0 and rows[-1] < b
        assert np.array_equal(got["hard"], hard.numpy()[rows])
        assert np.array_equal(got["hard_weight"], hard.numpy().sum(axis=1, dtype=np.int64))
        assert got["counts"].tolist() == [3.0, 1.0]
        bench.dump_outputs(d + "_again", hard, {"counts": np.array([3, 1])})
        assert np.array_equal(np.load(os.path.join(d + "_again", "hard_rows.npy")), got["hard_rows"])


def _run(args):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"] + args,
                         capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    return json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])


def test_cpu_baselines_only_with_full(monkeypatch):
    """A plain run times no CPU baseline whatever --cpu-seconds says; --full
    keeps the budget (8 s by default); --steps is the number of timed steps."""
    import bench
    for argv, secs in (([], 0.0), (["--cpu-seconds", "3"], 0.0), (["--full"], 8.0),
                       (["--full", "--cpu-seconds", "3"], 3.0), (["--full", "--cpu-seconds", "0"], 0.0)):
        monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "3"] + argv)
        a = bench.parse()
        assert a.cpu_seconds == secs and a.full == ("--full" in argv)
        assert (a.steps, a.warmup, a.dump_outputs) == (7, 3, None)


@pytest.mark.gpu
def test_plain_run_dumps_what_the_last_step_computed(tmp_path):
    """48 DVB-S2 r1/2 codewords, 5 iterations, 2 timed steps, no --full: no
    CPU baseline in the line, and the dumped hard decisions are those of the
    oracle on the same inputs (regenerated here from the seed, as bench.py's
    ranks do); ones per codeword and the error counters (the ones in the
    information bits of the all-zero codeword, once per timed step) agree."""
    import torch
    import oracle as O
    from ldpcgputegra_amd import Code, Decoder, channel, load_table
    t = load_table("dvbs2_r1_2")
    B, iters, steps = 48, 5, 2
    line = _run(["--batch", str(B), "--iters", str(iters), "--steps", str(steps), "--warmup", "1",
                 "--dump-outputs", str(tmp_path)])
    assert line["cpu_baseline"] is None and "cpu_baseline_product_host" not in line
    assert line["steps"] == steps and line["warmup"] == 1 and line["ms_per_step"] > 0
    assert line["unit"] == "Mbit/s" and line["dtype"] == "int8" and line["higher_is_better"] is True
    assert line["value"] == pytest.approx(B * t.n / line["ms_per_step"] / 1e3, rel=1e-3)
    got = {k: np.load(str(tmp_path / (k + ".npy"))) for k in NAMES}
    assert sorted(os.listdir(str(tmp_path))) == sorted(k + ".npy" for k in NAMES)
    assert all(v.dtype in (np.float32, np.float64) for v in got.values())
    dec = Decoder(Code("dvbs2_r1_2"), max_batch=B)
    llr = torch.empty((B, t.n), dtype=torch.int8, device="cuda")
    table = channel.i8_table(channel.sigma_from_ebn0(1.0, t.k_info / t.n), 8, 31)
    dec.awgn_i8_device(llr, first_cw=0, seed=2024, table=table)
    torch.cuda.synchronize()
    dec.close()
    exp = O.decode_i8(t, llr.cpu().numpy(), iters, threads=O.host_threads())
    assert np.array_equal(got["hard"], exp.astype(np.float32))
    assert np.array_equal(got["hard_rows"], np.arange(B))
    assert np.array_equal(got["hard_weight"], exp.sum(axis=1, dtype=np.int64))
    info = exp[:, :t.k_info].sum(axis=1, dtype=np.int64)
    assert info.sum() > 0
    assert got["counts"].tolist() == [steps * info.sum(), steps * (info > 0).sum()]
    assert line["ber"] == got["counts"][0] / (steps * B * t.k_info) and line["fer"] == got["counts"][1] / (steps * B)
