#!/usr/bin/env python3
"""What the int8 decode of the longer QC codes costs on `ldsepwi`
(csrc/ldsepwi.hip: kernel family 9 in int8 with one pair of codewords spread
over W = 2 or 4 waves, behind the i8_ep_wide switch) beside the kernel those
codes run on with the switch off, the LDS-resident family 7, and beside the
float32 `ldsepw`, in the same build and the same run.  One JSON line, also
written to profiles/i8_ep_wide_rate.json.  The automatic rule (`waves_auto` of
ldpc_code_i8_ep_wide_info, ldsepwi_rule in csrc/ldsepwi.hip) is fitted to this
file, and the file says whether the rule it was run with agrees with it.

1944x972, 1248x624 and 2304x1152, 20 iterations, OMS 1 and NMS 26, no early
termination, quantised LLRs at 2.0 dB (ldpc_awgn_i8: the default chain of
ldpc_sim), 1024 / 4096 / 16384 / 65536 codewords.  The method is
tools/ep_wide_rate.py's: one warm-up pass of every leg, then the legs alternated
step by step, the median of the steps kept and the spread (max - min) / median
of the repeats recorded.  A step's time is the decode kernel's own, from the
context's profile (ldpc_ctx_profile: device events around the launch).  Every
(code, batch) runs in a fresh child process, all its legs in that one process,
each child under a time limit of its own; a child that fails ends the run.

  w2, w4   decode_i8_device forced to family 9, LDPC_EPW_WAVES = 2 / 4 (the W compiled for the code in int8)
  auto     the switch on, the automatic choice (its family and W are recorded)
  off      the switch off: the parent's choice, family 7 in int8 -- the baseline of every ratio
  f32      decode_f32_device with ep_wide on, automatic (`ldsepw`), on the dequantised LLRs: for comparison only

Per point: `spread` is the largest spread of the int8 legs; `best_w` the fastest
forced W; `rule_ok` whether the automatic leg's choice is as the fitting of the
rule demands: the fastest forced W (or one within the spread of it) where that W
is ahead of `off` by more than the spread, and the old family elsewhere.

GPU box:  python tools/i8_ep_wide_rate.py [--steps 9]"""
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
ALGOS = {"OMS": 1, "NMS": 26}
F32_BETA = {"OMS": 1.0, "NMS": 26 / 32.0}
CHILD_TIMEOUT = 240     # seconds per (code, batch): two algorithms x at most five legs x (1 + steps) decodes of milliseconds


def child(name, batch, steps):
    import torch
    from ldpcgputegra_amd import ALGO_NMS, ALGO_OMS, Code, Decoder, _lib, channel, default_params
    code = Code(name)
    n, k = code.n, code.k_info
    info = code.i8_ep_wide_info(batch)
    assert info["waves"], name
    sigma = channel.sigma_from_ebn0(EBN0, k / n)
    forced = Decoder(code, max_batch=batch, kernel=9, i8_ep_wide=True)
    decs = {"w%d" % w: forced for w in info["waves"]}
    decs["auto"] = Decoder(code, max_batch=batch, i8_ep_wide=True)
    decs["off"] = Decoder(code, max_batch=batch)
    decs["f32"] = Decoder(code, max_batch=batch, ep_wide=True)
    q = torch.empty((batch, n), dtype=torch.int8, device="cuda")
    hard = torch.empty((batch, n), dtype=torch.uint8, device="cuda")
    forced.awgn_i8_device(q, 0, 1, channel.i8_table(sigma))
    torch.cuda.synchronize()
    y = q.to(torch.float32)
    for d in set(decs.values()):
        d.profile(True)
    legs = list(decs)
    i8_legs = [leg for leg in legs if leg != "f32"]
    ran = {}

    def step(leg, algo):
        dec = decs[leg]
        if leg.startswith("w"):
            os.environ["LDPC_EPW_WAVES"] = leg[1:]
        else:
            os.environ.pop("LDPC_EPW_WAVES", None)
        a = ALGO_OMS if algo == "OMS" else ALGO_NMS
        if leg == "f32":
            dec.decode_f32_device(y, hard, ITERS, params=default_params(algo=a, beta=F32_BETA[algo]))
        else:
            dec.decode_i8_device(q, hard, ITERS, params=default_params(algo=a, offset=ALGOS[algo], factor=ALGOS[algo]))
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
        for leg in legs:       # warm-up, one pass each
            step(leg, algo)
        times = {leg: [] for leg in legs}
        fe = {}
        for _ in range(steps):
            for leg in legs:
                t, fe[leg] = step(leg, algo)
                times[leg].append(t)
        assert len(set(fe[leg] for leg in i8_legs)) == 1, fe       # one contract, one result
        out = {}
        for leg, v in times.items():
            med = statistics.median(v)
            out[leg] = dict(kernel_ms=round(med, 4), min_ms=round(min(v), 4), max_ms=round(max(v), 4), steps=len(v),
                            spread=round((max(v) - min(v)) / med, 4), coded_mbps=round(batch * n / med / 1e3, 1))
        out["auto"]["kernel"], out["auto"]["waves"] = ran["auto"]
        out["f32"]["kernel"], out["f32"]["waves"] = ran["f32"]
        spread = max(out[leg]["spread"] for leg in i8_legs)
        best_w = min(info["waves"], key=lambda w: out["w%d" % w]["kernel_ms"])
        best, off = out["w%d" % best_w]["kernel_ms"], out["off"]["kernel_ms"]
        auto_w = ran["auto"][1]
        if best * (1.0 + spread) < off:     # ahead of the old family by more than the spread
            rule_ok = auto_w != 0 and out["w%d" % auto_w]["kernel_ms"] <= best * (1.0 + spread)
        else:
            rule_ok = auto_w == 0
        row = dict(code=name, algo=algo, batch=batch, n_layers=info["n_layers"], n_passes=info["n_passes"],
                   waves=info["waves"], waves_auto=info["waves_auto"], legs=out, frame_errors=fe["off"],
                   spread=round(spread, 4), best_w=best_w, best_over_off=round(best / off, 3),
                   best_over_f32=round(best / out["f32"]["kernel_ms"], 3), rule_ok=bool(rule_ok),
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "i8_ep_wide_rate.json"))
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
    res = dict(tool="i8_ep_wide_rate", build=build, device=device, iters=ITERS, ebn0=EBN0, steps_each=a.steps, rows=rows,
               rule_ok_everywhere=all(r["rule_ok"] for r in rows),
               wide_beats_off_at=[[r["code"], r["algo"], r["batch"]] for r in rows if r["best_over_off"] < 1.0])
    line = json.dumps(res)
    print(line, flush=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
