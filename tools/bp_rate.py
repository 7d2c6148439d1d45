#!/usr/bin/env python3
"""What belief propagation costs on the device (csrc/bp.hip), as one JSON line,
also written to profiles/bp_rate.json.  Workload: 648x324, batch 1024, 20
iterations, no early termination -- the shape of BASELINE.json configs[1] -- on
true LLRs at 2.0 dB.  Three legs, alternated step by step in one run on one
device, each step one decode_f32_device timed with device events:

  bp_lds       LDPC_ALGO_BP on family 7 (LDS-resident)
  bp_generic   LDPC_ALGO_BP on family 1 (any H)
  ms_lds       plain min-sum on family 7, the kernel the BP one is shaped after

No time is fixed in advance.  The one gate: the family the automatic choice
takes for BP on this code is the faster of the two BP legs.  README quotes
bp_over_ms (bp_lds / ms_lds) from the file.

GPU box:  python tools/bp_rate.py [--steps 30]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ldpcgputegra_amd import ALGO_BP, ALGO_MS, Code, Decoder, _lib, channel, default_params  # noqa: E402

CODE, BATCH, ITERS, EBN0 = "648x324", 1024, 20, 2.0
LEGS = (("bp_lds", ALGO_BP, 7), ("bp_generic", ALGO_BP, 1), ("ms_lds", ALGO_MS, 7))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bp_rate.json"))
    a = ap.parse_args()
    import torch
    code = Code(CODE)
    n, k = code.n, code.k_info
    sigma = channel.sigma_from_ebn0(EBN0, k / n)
    llr = torch.from_numpy(channel.awgn_f32_host(n, BATCH, seed=1, sigma=sigma, normalize=True)).cuda()
    hard = torch.empty((BATCH, n), dtype=torch.uint8, device="cuda")
    decs = {name: Decoder(code, max_batch=BATCH, kernel=kern) for name, _, kern in LEGS}
    params = {name: default_params(algo=algo, beta=0.0) for name, algo, _ in LEGS}

    def step(name):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        decs[name].decode_f32_device(llr, hard, ITERS, params=params[name])
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1), int(hard[:, :k].any(dim=1).sum().item())

    for _ in range(3):
        for name, _, _ in LEGS:
            step(name)
    ms = {name: [] for name, _, _ in LEGS}
    fe = {}
    for _ in range(a.steps):
        for name, _, _ in LEGS:
            t, fe[name] = step(name)
            ms[name].append(t)
    auto = Decoder(code, max_batch=BATCH)
    auto.decode_f32_device(llr, hard, ITERS, params=params["bp_lds"])
    torch.cuda.synchronize()
    picked = auto.last_kernel
    med = {name: statistics.median(v) for name, v in ms.items()}
    faster = "lds" if med["bp_lds"] <= med["bp_generic"] else "generic"
    res = dict(tool="bp_rate", build=_lib.source_hash(), device=torch.cuda.get_device_name(0), code=CODE, batch=BATCH,
               iters=ITERS, ebn0=EBN0, steps_each=a.steps,
               legs={name: dict(algo="BP" if algo == ALGO_BP else "MS", family=decs[name].last_kernel,
                                step_ms=round(med[name], 4), min_ms=round(min(ms[name]), 4),
                                max_ms=round(max(ms[name]), 4), frame_errors=fe[name],
                                coded_mbps=round(BATCH * n / med[name] / 1e3, 1)) for name, algo, _ in LEGS},
               bp_over_ms=round(med["bp_lds"] / med["ms_lds"], 2),
               gate=dict(what="the family auto selects for BP is the faster of bp_lds and bp_generic", auto=picked,
                         faster=faster, met=picked == faster))
    line = json.dumps(res)
    print(line, flush=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    return 0 if res["gate"]["met"] else 1


if __name__ == "__main__":
    sys.exit(main())
