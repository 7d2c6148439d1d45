#!/usr/bin/env python3
"""What the on-device bit source and encoder cost (csrc/encode.hip), as one
JSON line.  For DVB-S2 r1/2 and r9/10 at batch 4096: the info_bits, dvbs2_encode
and (for scale) awgn_i8 launches timed with device events, the host encoder's
time for the 64 codewords the pooled ldpc_sim mode encodes, and -- r1/2 only --
the ldpc_sim step (count reset, [bits, encode,] channel, 50-iteration decode,
count, counters read back) with the pooled codewords and with fresh ones,
alternated in one run.  The one gate: the fresh step takes at most 1.05 x the
pooled step.  GPU box:  python tools/encode_rate.py [--batch 4096] [--launches 50]
[--steps 20]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ldpcgputegra_amd import Code, Decoder, _lib, channel, default_params  # noqa: E402

PEAK_GBS = 8000.0   # MI355X HBM3E


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
    table = channel.i8_table(channel.sigma_from_ebn0(1.0, k / n))
    info = torch.empty((B, k), dtype=torch.uint8, device="cuda")
    cw = torch.empty((B, n), dtype=torch.uint8, device="cuda")
    llr = torch.empty((B, n), dtype=torch.int8, device="cuda")
    out = dict(
        info_bits=rate(timed(torch, lambda: dec.info_bits_device(info, 0, 1), launches), B * k),
        dvbs2_encode=rate(timed(torch, lambda: dec.encode_device(info, cw), launches), B * (k + n)),
        awgn_i8=rate(timed(torch, lambda: dec.awgn_i8_device(llr, 0, 1, table, codeword=cw), launches), 2 * B * n))
    # the host encoder on 64 codewords: what the pooled mode runs once per sweep
    pool = channel.info_bits_host(k, 64, 1)
    ts = []
    for _ in range(3):
        t = time.perf_counter()
        code.encode(pool)
        ts.append((time.perf_counter() - t) * 1e3)
    out["host_encode_64_ms"] = round(min(ts), 3)
    dec.close()
    return out


def steps(torch, name, B, n_steps, ebn0, early_term):
    code = Code(name)
    n, k = code.n, code.k_info
    dec = Decoder(code, max_batch=B)
    table = channel.i8_table(channel.sigma_from_ebn0(ebn0, k / n))
    p = default_params(algo=_lib.ALGO_OMS, offset=1, early_term=early_term)
    info = torch.empty((B, k), dtype=torch.uint8, device="cuda")
    fresh_cw = torch.empty((B, n), dtype=torch.uint8, device="cuda")
    pool = code.encode(channel.info_bits_host(k, 64, 1))
    pooled_cw = torch.from_numpy(pool[np.arange(B) % 64]).cuda()
    llr = torch.empty((B, n), dtype=torch.int8, device="cuda")
    hard = torch.empty((B, n), dtype=torch.uint8, device="cuda")
    cnt = torch.zeros(2, dtype=torch.int64, device="cuda")

    def step(fresh, no):
        t = time.perf_counter()
        cnt.zero_()
        cw = pooled_cw
        if fresh:
            cw = fresh_cw
            dec.info_bits_device(info, no * B, 1)
            dec.encode_device(info, cw)
        dec.awgn_i8_device(llr, no * B, 1, table, codeword=cw)
        dec.decode_i8_device(llr, hard, 50, p)
        dec.count_errors_device(hard, k, cnt, ref=cw)
        c = cnt.cpu().tolist()
        return (time.perf_counter() - t) * 1e3, c

    for no in range(3):
        step(False, no), step(True, no)
    ms = {False: [], True: []}
    fe = {False: 0, True: 0}
    for no in range(n_steps):
        for fresh in (False, True):
            t, c = step(fresh, no)
            ms[fresh].append(t)
            fe[fresh] += c[1]
    dec.close()
    pooled, fresh = statistics.median(ms[False]), statistics.median(ms[True])
    return dict(code=name, batch=B, steps_each=n_steps, ebn0=ebn0, iters=50, early_term=early_term,
                pooled_ms=round(pooled, 3), fresh_ms=round(fresh, 3), ratio=round(fresh / pooled, 4),
                pooled_frame_errors=fe[False], fresh_frame_errors=fe[True])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--steps", type=int, default=20)
    a = ap.parse_args()
    import torch
    res = dict(tool="encode_rate", build=_lib.source_hash(), device=torch.cuda.get_device_name(0), batch=a.batch,
               launches=a.launches, peak_gb_per_s=PEAK_GBS)
    res["kernels"] = {name: kernels(torch, name, a.batch, a.launches) for name in ("dvbs2_r1_2", "dvbs2_r9_10")}
    res["step"] = steps(torch, "dvbs2_r1_2", a.batch, a.steps, 1.0, 0)
    res["step_early_term"] = steps(torch, "dvbs2_r1_2", a.batch, a.steps, 1.3, 1)
    res["gate"] = dict(what="step.fresh_ms <= 1.05 * step.pooled_ms", ratio=res["step"]["ratio"], limit=1.05,
                       met=res["step"]["ratio"] <= 1.05)
    print(json.dumps(res), flush=True)
    return 0 if res["gate"]["met"] else 1


if __name__ == "__main__":
    sys.exit(main())
