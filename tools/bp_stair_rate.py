#!/usr/bin/env python3
"""What belief propagation costs on the staircase kernel (csrc/stairbp*), as
one JSON line, also written to profiles/bp_stair_rate.json.  Workload:
dvbs2_r1_2, 20 iterations, no early termination, true LLRs at 2.0 dB, batches
1024, 4096 and 16384.  Legs per batch, alternated step by step in one run on
one device, each step one decode_f32_device timed with device events:

  bp_stair_s<S>  LDPC_ALGO_BP on family 11 at each group width the code has
                 (LDPC_STAIRF_S forces it)
  bp_generic     LDPC_ALGO_BP on family 1 (any H), what BP ran on before; a few
                 steps only, each takes seconds
  ms_stair       plain min-sum on family 11 at its own width

No time is fixed in advance.  Two gates, at every batch:
  1. BP on family 11 at the width its rule picks is faster than BP on family 1;
  2. the rule's width is the fastest measured one, or within the run's own
     spread of it: the larger (max - min) / median of the two legs compared.
README and DESIGN.md quote the times and bp_over_ms from the file.

GPU box:  python tools/bp_stair_rate.py [--steps 9] [--generic-steps 3]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ldpcgputegra_amd import ALGO_BP, ALGO_MS, Code, Decoder, _lib, channel, default_params  # noqa: E402

CODE, ITERS, EBN0 = "dvbs2_r1_2", 20, 2.0
BATCHES = (1024, 4096, 16384)


def widths_of(code):
    """stairf_upload's rule: S with M % S == 0 and min_hazard >= S * P(X, S)."""
    t = code.table()
    X, m, hazard = t.groups[0][0] - 2, t.m, code.plan_info()["min_hazard"]
    pr = 8 if X <= 5 else 6 if X <= 8 else 4 if X <= 12 else 2
    return X, m, tuple(S for S in (2, 4, 8, 16) if m % S == 0 and hazard >= S * min(pr, 48 // S))


def measure(torch, code, batch, steps, gsteps):
    n, k = code.n, code.k_info
    X, m, widths = widths_of(code)
    stride = (batch + 63) // 64 * 64
    rule = _lib.lib().ldpc_bp_staircase_width_model(X, m, stride, sum(widths))
    sigma = channel.sigma_from_ebn0(EBN0, k / n)
    stair = Decoder(code, max_batch=batch, kernel=11, bp_staircase=True)
    generic = Decoder(code, max_batch=batch, kernel=1)
    llr = torch.empty((batch, n), dtype=torch.float32, device="cuda")
    stair.awgn_f32_device(llr, 0, 1, sigma, normalize=True)
    hard = torch.empty((batch, n), dtype=torch.uint8, device="cuda")
    bp, ms = default_params(algo=ALGO_BP), default_params(algo=ALGO_MS, beta=0.0)
    legs = [("bp_stair_s%d" % S, stair, bp, S) for S in widths] + [("ms_stair", stair, ms, 0),
                                                                  ("bp_generic", generic, bp, 0)]

    def step(leg):
        name, dec, params, S = leg
        if S:
            os.environ["LDPC_STAIRF_S"] = str(S)
        else:
            os.environ.pop("LDPC_STAIRF_S", None)
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        dec.decode_f32_device(llr, hard, ITERS, params=params)
        t1.record()
        torch.cuda.synchronize()
        os.environ.pop("LDPC_STAIRF_S", None)
        return t0.elapsed_time(t1), int(hard[:, :k].any(dim=1).sum().item())

    for leg in legs:       # warm-up: sizes the scratch, one pass each
        step(leg)
    times = {leg[0]: [] for leg in legs}
    fe = {}
    for i in range(steps):
        for leg in legs:
            if leg[0] == "bp_generic" and i >= gsteps:
                continue
            t, fe[leg[0]] = step(leg)
            times[leg[0]].append(t)
    out = {}
    for name, v in times.items():
        med = statistics.median(v)
        out[name] = dict(step_ms=round(med, 3), min_ms=round(min(v), 3), max_ms=round(max(v), 3), steps=len(v),
                         spread=round((max(v) - min(v)) / med, 4), frame_errors=fe[name],
                         coded_mbps=round(batch * n / med / 1e3, 1))
    stair.close()
    generic.close()
    del llr, hard
    torch.cuda.empty_cache()
    picked, best = "bp_stair_s%d" % rule, min((n_ for n_ in out if n_.startswith("bp_stair")),
                                              key=lambda n_: out[n_]["step_ms"])
    spread = max(out[picked]["spread"], out[best]["spread"])
    g1 = out[picked]["step_ms"] < out["bp_generic"]["step_ms"]
    g2 = out[picked]["step_ms"] <= out[best]["step_ms"] * (1.0 + spread)
    assert len({d["frame_errors"] for n_, d in out.items() if n_.startswith("bp_")}) == 1, out   # one algorithm, one result
    return dict(batch=batch, widths=list(widths), rule_width=rule, fastest_width=int(best.rsplit("s", 1)[1]),
                legs=out, bp_over_ms=round(out[picked]["step_ms"] / out["ms_stair"]["step_ms"], 2),
                generic_over_stair=round(out["bp_generic"]["step_ms"] / out[picked]["step_ms"], 2),
                gates=dict(faster_than_generic=g1, rule_is_fastest=g2, spread=spread))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=9)
    ap.add_argument("--generic-steps", type=int, default=3)
    ap.add_argument("--batches", type=int, nargs="*", default=list(BATCHES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bp_stair_rate.json"))
    a = ap.parse_args()
    import torch
    code = Code(CODE)
    rows = [measure(torch, code, b, a.steps, a.generic_steps) for b in a.batches]
    met = all(r["gates"]["faster_than_generic"] and r["gates"]["rule_is_fastest"] for r in rows)
    res = dict(tool="bp_stair_rate", build=_lib.source_hash(), device=torch.cuda.get_device_name(0), code=CODE,
               iters=ITERS, ebn0=EBN0, steps_each=a.steps, generic_steps=a.generic_steps, batches=rows,
               gates=dict(what="at every batch BP on stairf at the rule's width beats BP on generic, and the rule's "
                               "width is the fastest measured or within the run's spread of it", met=met))
    line = json.dumps(res)
    print(line, flush=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    return 0 if met else 1


if __name__ == "__main__":
    sys.exit(main())
