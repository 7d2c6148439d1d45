#!/usr/bin/env python3
"""What the float channel costs on the device (awgn_f32_k, csrc/layout.hip), as
one JSON line, also written to profiles/awgn_f32_rate.json.  For 648x324 and
DVB-S2 r1/2 at batch 4096: the awgn_f32 launch timed with device events (ms and
GB/s of the 4 N B bytes it writes, against the HBM peak) with awgn_i8 beside it,
and the float ldpc_sim step -- count reset, [channel,] 20-iteration MS decode
with the fused error count, counters read back -- on a prepared buffer and with
the channel drawn every step, alternated in one run.  The one gate: for DVB-S2
r1/2 the step with the channel takes at most 1.05 x the step without it.

--without-channel runs only the step on a prepared buffer, which touches no
code of the float channel: the same leg can be timed on a build that predates
it (both figures go into the JSON by hand, "step_without_channel_second_visit").

GPU box:  python tools/awgn_f32_rate.py [--batch 4096] [--launches 50] [--steps 20]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ldpcgputegra_amd import Code, Decoder, _lib, channel, default_params  # noqa: E402

PEAK_GBS = 8000.0   # MI355X HBM3E
ITERS = 20
CODES = ("648x324", "dvbs2_r1_2")


def timed(torch, launch, n):
    """ms per launch: device events around n back-to-back launches."""
    for _ in range(5):
        launch()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(n):
        launch()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / n


def rate(ms, nbytes):
    gbs = nbytes / ms / 1e6
    return dict(ms=round(ms, 4), bytes=int(nbytes), gb_per_s=round(gbs, 1), of_peak=round(gbs / PEAK_GBS, 4))


def kernels(torch, name, B, launches):
    code = Code(name)
    n, k = code.n, code.k_info
    dec = Decoder(code, max_batch=B)
    sigma = channel.sigma_from_ebn0(1.0, k / n)
    table = channel.i8_table(sigma)
    y = torch.empty((B, n), dtype=torch.float32, device="cuda")
    llr = torch.empty((B, n), dtype=torch.int8, device="cuda")
    out = dict(awgn_f32=rate(timed(torch, lambda: dec.awgn_f32_device(y, 0, 1, sigma), launches), 4 * B * n),
               awgn_i8=rate(timed(torch, lambda: dec.awgn_i8_device(llr, 0, 1, table), launches), B * n))
    dec.close()
    return out


def steps(torch, name, B, n_steps, ebn0, with_channel):
    """Median ms of the float step without the channel (a prepared buffer) and,
    if with_channel, with it; the two alternate."""
    code = Code(name)
    n, k = code.n, code.k_info
    dec = Decoder(code, max_batch=B)
    sigma = channel.sigma_from_ebn0(ebn0, k / n)
    p = default_params(algo=_lib.ALGO_MS, beta=0.0)
    g = torch.Generator(device="cuda")
    g.manual_seed(1)
    prepared = torch.randn((B, n), generator=g, dtype=torch.float32, device="cuda") * sigma - 1.0
    y = torch.empty((B, n), dtype=torch.float32, device="cuda")
    hard = torch.empty((B, n), dtype=torch.uint8, device="cuda")
    cnt = torch.zeros(2, dtype=torch.int64, device="cuda")

    def step(drawn, no):
        t = time.perf_counter()
        cnt.zero_()
        llr = prepared
        if drawn:
            llr = y
            dec.awgn_f32_device(y, no * B, 1, sigma)
        dec.decode_count_device(llr, hard, ITERS, k, cnt, params=p)
        c = cnt.cpu().tolist()
        return (time.perf_counter() - t) * 1e3, c

    legs = (False, True) if with_channel else (False,)
    for no in range(3):
        for drawn in legs:
            step(drawn, no)
    ms = {leg: [] for leg in legs}
    fe = {leg: 0 for leg in legs}
    for no in range(n_steps):
        for drawn in legs:
            t, c = step(drawn, no)
            ms[drawn].append(t)
            fe[drawn] += c[1]
    dec.close()
    out = dict(code=name, batch=B, steps_each=n_steps, ebn0=ebn0, iters=ITERS, algo="MS",
               without_ms=round(statistics.median(ms[False]), 3), without_frame_errors=fe[False])
    if with_channel:
        out.update(with_ms=round(statistics.median(ms[True]), 3), with_frame_errors=fe[True],
                   ratio=round(statistics.median(ms[True]) / statistics.median(ms[False]), 4))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--without-channel", action="store_true",
                    help="only the step on a prepared buffer (runs on a build without the float channel)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "awgn_f32_rate.json"))
    a = ap.parse_args()
    import torch
    res = dict(tool="awgn_f32_rate", build=_lib.source_hash(), device=torch.cuda.get_device_name(0), batch=a.batch,
               launches=a.launches, peak_gb_per_s=PEAK_GBS)
    if a.without_channel:
        res["step"] = {name: steps(torch, name, a.batch, a.steps, 1.0, False) for name in CODES}
        print(json.dumps(res), flush=True)
        return 0
    res["kernels"] = {name: kernels(torch, name, a.batch, a.launches) for name in CODES}
    res["step"] = {name: steps(torch, name, a.batch, a.steps, 1.0, True) for name in CODES}
    ratio = res["step"]["dvbs2_r1_2"]["ratio"]
    res["gate"] = dict(what="step.dvbs2_r1_2.with_ms <= 1.05 * step.dvbs2_r1_2.without_ms", ratio=ratio, limit=1.05,
                       met=ratio <= 1.05)
    line = json.dumps(res)
    print(line, flush=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    return 0 if res["gate"]["met"] else 1


if __name__ == "__main__":
    sys.exit(main())
