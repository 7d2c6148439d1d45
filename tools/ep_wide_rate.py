#!/usr/bin/env python3
"""What the float min-sum decode of the longer QC codes costs on `ldsepw`
(csrc/ldsepw.hip: kernel family 9 with one codeword spread over W = 2 or 4
waves, behind the ep_wide switch) beside the kernel those codes run on with the
switch off, the LDS-resident family 7, in the same build and the same run.  One
JSON line, also written to profiles/ep_wide_rate.json.  The automatic rule
(`waves_auto` of ldpc_code_ep_wide_info, ldsepw_rule in csrc/ldsepw.hip) is
fitted to this file, and the file says whether the rule it was run with agrees
with it.

1944x972, 1248x624 and 2304x1152, 20 iterations, plain min-sum and NMS 0.8125,
no early termination, true LLRs at 2.0 dB, 1024 / 4096 / 16384 / 65536
codewords.  The method is tools/f16_ep_rate.py's: one warm-up pass of every leg,
then the legs alternated step by step, the median of the steps kept and the
spread (max - min) / median of the repeats recorded.  A step's time is the
decode kernel's own, from the context's profile (ldpc_ctx_profile: device events
around the launch).  Every (code, batch) runs in a fresh child process, each
under a time limit of its own; a child that fails ends the run.

  w2, w4   decode_f32_device forced to family 9, LDPC_EPW_WAVES = 2 / 4 (the W compiled for the code)
  auto     the switch on, the automatic choice (its family and W are recorded)
  off      the switch off: the parent's choice, family 7

Per point: `spread` is the largest spread of its legs; `best_w` the fastest
forced W; `rule_ok` whether the automatic leg's choice is as the issue of the
rule demands: within the spread of the fastest forced W where that W beats
`off`, and on the old family where even the fastest W is slower than `off` by
more than the spread.

GPU box:  python tools/ep_wide_rate.py [--steps 9]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ITERS, EBN0 = 20, 2.0
CODES, BATCHES = ("1944x972", "1248x624", "2304x1152"), (1024, 4096, 16384, 65536)
ALGOS = {"MS": 0.0, "NMS": 0.8125}
CHILD_TIMEOUT = 240     # seconds per (code, batch): two algorithms x at most four legs x (1 + steps) decodes of milliseconds


def child(name, batch, steps):
    import torch
    from ldpcgputegra_amd import ALGO_MS, ALGO_NMS, Code, Decoder, _lib, channel, default_params
    code = Code(name)
    n, k = code.n, code.k_info
    info = code.ep_wide_info(batch)
    assert info["waves"], name
    sigma = channel.sigma_from_ebn0(EBN0, k / n)
    forced = Decoder(code, max_batch=batch, kernel=9, ep_wide=True)
    decs = {"w%d" % w: forced for w in info["waves"]}
    decs["auto"] = Decoder(code, max_batch=batch, ep_wide=True)
    decs["off"] = Decoder(code, max_batch=batch)
    y = torch.empty((batch, n), dtype=torch.float32, device="cuda")
    hard = torch.empty((batch, n), dtype=torch.uint8, device="cuda")
    forced.awgn_f32_device(y, 0, 1, sigma, normalize=True)
    torch.cuda.synchronize()
    for d in set(decs.values()):
        d.profile(True)
    legs = list(decs)
    ran = {}

    def step(leg, p):
        dec = decs[leg]
        if leg.startswith("w"):
            os.environ["LDPC_EPW_WAVES"] = leg[1:]
        else:
            os.environ.pop("LDPC_EPW_WAVES", None)
        dec.decode_f32_device(y, hard, ITERS, params=p)
        torch.cuda.synchronize()
        ran[leg] = (dec.last_kernel, dec.last_ep_waves)
        if leg.startswith("w"):
            assert ran[leg] == ("ldsep", int(leg[1:])), (leg, ran[leg])
        if leg == "off":
            assert ran[leg] == ("lds", 0), ran[leg]
        ms, launches = dec.kernel_time(reset=True)
        assert launches == 1, (leg, launches)
        return ms, int(hard[:, :k].any(dim=1).sum().item())

    for algo in ALGOS:
        p = default_params(algo=ALGO_MS if algo == "MS" else ALGO_NMS, beta=ALGOS[algo])
        for leg in legs:       # warm-up, one pass each
            step(leg, p)
        times = {leg: [] for leg in legs}
        fe = {}
        for _ in range(steps):
            for leg in legs:
                t, fe[leg] = step(leg, p)
                times[leg].append(t)
        assert len(set(fe.values())) == 1, fe       # one contract (up to the sign of a zero): one result
        out = {}
        for leg, v in times.items():
            med = statistics.median(v)
            out[leg] = dict(kernel_ms=round(med, 4), min_ms=round(min(v), 4), max_ms=round(max(v), 4), steps=len(v),
                            spread=round((max(v) - min(v)) / med, 4), coded_mbps=round(batch * n / med / 1e3, 1))
        out["auto"]["kernel"], out["auto"]["waves"] = ran["auto"]
        spread = max(l["spread"] for l in out.values())
        best_w = min(info["waves"], key=lambda w: out["w%d" % w]["kernel_ms"])
        best, off = out["w%d" % best_w]["kernel_ms"], out["off"]["kernel_ms"]
        auto_w = ran["auto"][1]
        if best > off * (1.0 + spread):     # slower than the old family by more than the spread: left to it
            rule_ok = auto_w == 0
        else:
            rule_ok = auto_w != 0 and out["w%d" % auto_w]["kernel_ms"] <= best * (1.0 + spread)
        row = dict(code=name, algo=algo, batch=batch, n_layers=info["n_layers"], n_passes=info["n_passes"],
                   waves=info["waves"], waves_auto=info["waves_auto"], legs=out, frame_errors=fe["off"],
                   spread=round(spread, 4), best_w=best_w, best_over_off=round(best / off, 3), rule_ok=bool(rule_ok),
                   build=_lib.source_hash(), device=torch.cuda.get_device_name(0))
        assert info["waves_auto"] == auto_w, (info, ran)
        print("ROW " + json.dumps(row), flush=True)
    for d in set(decs.values()):
        d.close()
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=9)
    ap.add_argument("--batches", type=int, nargs="*", default=list(BATCHES))
    ap.add_argument("--codes", nargs="*", default=list(CODES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ep_wide_rate.json"))
    ap.add_argument("--child", nargs=2, metavar=("CODE", "BATCH"), help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a.child[0], int(a.child[1]), a.steps)
    rows = []
    for name in a.codes:
        for batch in a.batches:
            try:
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--steps", str(a.steps), "--child", name,
                                    str(batch)], stdout=subprocess.PIPE, text=True, timeout=CHILD_TIMEOUT)
                status = r.returncode
            except subprocess.TimeoutExpired:
                status = 124
            if status != 0:      # a failed configuration ends the run: nothing more is started
                print("configuration %s %d failed with status %d" % (name, batch, status), file=sys.stderr)
                return 1
            for line in (ln for ln in r.stdout.splitlines() if ln.startswith("ROW ")):
                rows.append(json.loads(line[4:]))
                print(line, flush=True)
    build, device = rows[0].pop("build"), rows[0].pop("device")
    for r in rows[1:]:
        assert (r.pop("build"), r.pop("device")) == (build, device)
    res = dict(tool="ep_wide_rate", build=build, device=device, iters=ITERS, ebn0=EBN0, steps_each=a.steps, rows=rows,
               rule_ok_everywhere=all(r["rule_ok"] for r in rows),
               wide_beats_off_at=[[r["code"], r["algo"], r["batch"]] for r in rows if r["best_over_off"] < 1.0])
    line = json.dumps(res)
    print(line, flush=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
