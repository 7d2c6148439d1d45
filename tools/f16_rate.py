#!/usr/bin/env python3
"""What the binary16 decode costs on the packed staircase kernel
(csrc/stairh*), beside the float32 decode on stairf, as one JSON line, also
written to profiles/f16_rate.json.  Workload: dvbs2_r1_2, 20 iterations, plain
min-sum, no early termination, true LLRs at 2.0 dB; batches 1024, 4096, 16384
and, for f16 only (float32's V offsets end at 16384), 32768.  Legs per batch,
alternated step by step in one run on one device, each step one decode timed
with device events:

  f16_s<S>  decode_f16_device at each group width the code has (LDPC_STAIRF_S
            forces it)
  f32       decode_f32_device on stairf at its own width

No time is fixed in advance.  Two gates:
  1. at batch 16384, f16 at the width its rule picks beats f32 by more than the
     run's own spread: the larger (max - min) / median of the two legs;
  2. at every batch the rule's width is the fastest measured one, or within
     that spread of it.
README and DESIGN.md quote the times and f16_over_f32 from the file.

GPU box:  python tools/f16_rate.py [--steps 9]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ldpcgputegra_amd import ALGO_MS, Code, Decoder, _lib, channel, default_params  # noqa: E402

CODE, ITERS, EBN0 = "dvbs2_r1_2", 20, 2.0
BATCHES = (1024, 4096, 16384, 32768)
F32_MAX_BATCH = 16384


def widths_of(code):
    """stairf_upload's rule: S with M % S == 0 and min_hazard >= S * P(X, S)."""
    t = code.table()
    X, m, hazard = t.groups[0][0] - 2, t.m, code.plan_info()["min_hazard"]
    pr = 8 if X <= 5 else 6 if X <= 8 else 4 if X <= 12 else 2
    return tuple(S for S in (2, 4, 8, 16) if m % S == 0 and hazard >= S * min(pr, 48 // S))


def measure(torch, code, batch, steps):
    n, k = code.n, code.k_info
    widths = widths_of(code)
    stride = (batch + 63) // 64 * 64
    rule = _lib.lib().ldpc_f16_staircase_width_rule(stride, sum(widths))
    sigma = channel.sigma_from_ebn0(EBN0, k / n)
    dec = Decoder(code, max_batch=batch, kernel=11)
    with_f32 = batch <= F32_MAX_BATCH
    hard = torch.empty((batch, n), dtype=torch.uint8, device="cuda")
    h = torch.empty((batch, n), dtype=torch.float16, device="cuda")
    # the channel is drawn in chunks, so float32 samples of the whole batch exist only where the f32 leg runs
    y = torch.empty((batch if with_f32 else 4096, n), dtype=torch.float32, device="cuda")
    for b0 in range(0, batch, y.shape[0]):
        nb = min(y.shape[0], batch - b0)
        dec.awgn_f32_device(y[:nb], b0, 1, sigma, normalize=True)
        dec.convert_f16_device(y[:nb], h[b0:b0 + nb])
    torch.cuda.synchronize()
    ms = default_params(algo=ALGO_MS, beta=0.0)
    legs = [("f16_s%d" % S, S) for S in widths] + ([("f32", 0)] if with_f32 else [])

    def step(leg):
        name, S = leg
        if S:
            os.environ["LDPC_STAIRF_S"] = str(S)
        else:
            os.environ.pop("LDPC_STAIRF_S", None)
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        if S:
            dec.decode_f16_device(h, hard, ITERS, params=ms)
        else:
            dec.decode_f32_device(y, hard, ITERS, params=ms)
        t1.record()
        torch.cuda.synchronize()
        os.environ.pop("LDPC_STAIRF_S", None)
        assert dec.last_kernel == "stairf"
        return t0.elapsed_time(t1), int(hard[:, :k].any(dim=1).sum().item())

    for leg in legs:       # warm-up: sizes the scratch, one pass each
        step(leg)
    times = {leg[0]: [] for leg in legs}
    fe = {}
    for _ in range(steps):
        for leg in legs:
            t, fe[leg[0]] = step(leg)
            times[leg[0]].append(t)
    out = {}
    for name, v in times.items():
        med = statistics.median(v)
        out[name] = dict(step_ms=round(med, 3), min_ms=round(min(v), 3), max_ms=round(max(v), 3), steps=len(v),
                         spread=round((max(v) - min(v)) / med, 4), frame_errors=fe[name],
                         coded_mbps=round(batch * n / med / 1e3, 1))
    dec.close()
    del y, h, hard
    torch.cuda.empty_cache()
    assert len({d["frame_errors"] for n_, d in out.items() if n_.startswith("f16_")}) == 1, out   # one result at every width
    picked = "f16_s%d" % rule
    best = min((n_ for n_ in out if n_.startswith("f16_")), key=lambda n_: out[n_]["step_ms"])
    spread2 = max(out[picked]["spread"], out[best]["spread"])
    row = dict(batch=batch, widths=list(widths), rule_width=rule, fastest_width=int(best.rsplit("s", 1)[1]), legs=out,
               gates=dict(rule_is_fastest=out[picked]["step_ms"] <= out[best]["step_ms"] * (1.0 + spread2),
                          rule_spread=spread2))
    if with_f32:
        spread1 = max(out[picked]["spread"], out["f32"]["spread"])
        row["f16_over_f32"] = round(out[picked]["step_ms"] / out["f32"]["step_ms"], 3)
        row["gates"].update(f16_beats_f32=out[picked]["step_ms"] < out["f32"]["step_ms"] * (1.0 - spread1),
                            f32_spread=spread1)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=9)
    ap.add_argument("--batches", type=int, nargs="*", default=list(BATCHES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "f16_rate.json"))
    a = ap.parse_args()
    import torch
    code = Code(CODE)
    rows = [measure(torch, code, b, a.steps) for b in a.batches]
    g1 = all(r["gates"]["f16_beats_f32"] for r in rows if r["batch"] == 16384)
    g2 = all(r["gates"]["rule_is_fastest"] for r in rows)
    res = dict(tool="f16_rate", build=_lib.source_hash(), device=torch.cuda.get_device_name(0), code=CODE, iters=ITERS,
               ebn0=EBN0, algo="MS", steps_each=a.steps, batches=rows,
               gates=dict(what="at batch 16384 f16 at its rule's width beats f32 on stairf by more than the run's "
                               "spread; at every batch the rule's width is the fastest measured or within the spread "
                               "of it", f16_beats_f32_at_16384=g1, rule_is_fastest=g2, met=g1 and g2))
    line = json.dumps(res)
    print(line, flush=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    return 0 if g1 and g2 else 1


if __name__ == "__main__":
    sys.exit(main())
