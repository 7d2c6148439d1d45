#!/usr/bin/env python3
"""What the int8 decode costs on the edge-parallel kernel (csrc/ldsepi.hip,
family 9 behind the i8_edge_parallel switch) beside the kernels it is measured
against, all of the same build and the same run: the int8 decode with the switch
off (family 7, `lds`: what these codes ran on before), the binary16 decode on
`ldseph` and the float32 decode on `ldsep`.  One JSON line, also written to
profiles/i8_ep_rate.json.

648x324 and 576x288, 20 iterations, OMS offset 1 (the default) and NMS 26, no
early termination, LLRs at 2.0 dB (int8: the quantised channel; the float legs:
true LLRs with the matching OMS 0.125 / NMS 0.8125), 1024 / 4096 / 16384 / 65536
codewords.  The method is tools/f16_ep_rate.py's: one warm-up pass of every leg,
then the legs alternated step by step, the median of the steps kept.  A step's
time is the decode kernel's own, from the context's profile (ldpc_ctx_profile:
device events around the launch).  Every configuration (code, algorithm, batch)
runs in a fresh child process.

  i8_ep      decode_i8_device on family 9 (ldsepi), the switch on
  i8_lds     decode_i8_device with the switch off: family 7
  f16_ep     decode_f16_device on family 9 (ldseph)
  f32_ldsep  decode_f32_device on family 9

The ratio that decides the automatic rule is ep_over_lds, of the same run.

GPU box:  python tools/i8_ep_rate.py [--steps 9]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ITERS, EBN0 = 20, 2.0
CODES, BATCHES = ("648x324", "576x288"), (1024, 4096, 16384, 65536)
ALGOS = {"OMS": (1, 0.125), "NMS": (26, 0.8125)}      # int8 parameter, float beta
LEGS = (("i8_ep", "i8", "ldsep"), ("i8_lds", "i8", "lds"), ("f16_ep", "f16", "ldsep"), ("f32_ldsep", "f32", "ldsep"))


def child(name, algo, batch, steps):
    import torch
    from ldpcgputegra_amd import ALGO_NMS, ALGO_OMS, Code, Decoder, _lib, channel, default_params
    code = Code(name)
    n, k = code.n, code.k_info
    sigma = channel.sigma_from_ebn0(EBN0, k / n)
    decs = dict(i8_ep=Decoder(code, max_batch=batch, i8_edge_parallel=True),
                i8_lds=Decoder(code, max_batch=batch),
                f16_ep=Decoder(code, max_batch=batch, f16_edge_parallel=True),
                f32_ldsep=Decoder(code, max_batch=batch, kernel=9))
    q = torch.empty((batch, n), dtype=torch.int8, device="cuda")
    y = torch.empty((batch, n), dtype=torch.float32, device="cuda")
    h = torch.empty((batch, n), dtype=torch.float16, device="cuda")
    hard = torch.empty((batch, n), dtype=torch.uint8, device="cuda")
    decs["i8_ep"].awgn_i8_device(q, 0, 1, channel.i8_table(sigma))
    decs["f32_ldsep"].awgn_f32_device(y, 0, 1, sigma, normalize=True)
    decs["f32_ldsep"].convert_f16_device(y, h)
    torch.cuda.synchronize()
    param, beta = ALGOS[algo]
    a = ALGO_OMS if algo == "OMS" else ALGO_NMS
    p8 = default_params(algo=a, offset=param, factor=param)
    pf = default_params(algo=a, beta=beta)
    for d in decs.values():
        d.profile(True)

    def step(leg):
        leg_name, kind, kernel = leg
        dec = decs[leg_name]
        if kind == "i8":
            dec.decode_i8_device(q, hard, ITERS, params=p8)
        elif kind == "f16":
            dec.decode_f16_device(h, hard, ITERS, params=pf)
        else:
            dec.decode_f32_device(y, hard, ITERS, params=pf)
        torch.cuda.synchronize()
        assert dec.last_kernel == kernel, (leg_name, dec.last_kernel)
        ms, launches = dec.kernel_time(reset=True)
        assert launches == 1, (leg_name, launches)
        return ms, int(hard[:, :k].any(dim=1).sum().item())

    for leg in LEGS:       # warm-up, one pass each
        step(leg)
    times = {leg[0]: [] for leg in LEGS}
    fe = {}
    for _ in range(steps):
        for leg in LEGS:
            t, fe[leg[0]] = step(leg)
            times[leg[0]].append(t)
    legs = {}
    for leg_name, v in times.items():
        med = statistics.median(v)
        legs[leg_name] = dict(kernel_ms=round(med, 4), min_ms=round(min(v), 4), max_ms=round(max(v), 4), steps=len(v),
                              spread=round((max(v) - min(v)) / med, 4), frame_errors=fe[leg_name],
                              coded_mbps=round(batch * n / med / 1e3, 1))
    lanes = decs["i8_lds"].last_lds_shape
    for d in decs.values():
        d.close()
    assert legs["i8_ep"]["frame_errors"] == legs["i8_lds"]["frame_errors"], legs   # one contract, one result
    row = dict(code=name, algo=algo, batch=batch, lds_lanes=lanes[0], legs=legs,
               ep_over_lds=round(legs["i8_ep"]["kernel_ms"] / legs["i8_lds"]["kernel_ms"], 3),
               ep_over_f16_ep=round(legs["i8_ep"]["kernel_ms"] / legs["f16_ep"]["kernel_ms"], 3),
               ep_over_f32_ldsep=round(legs["i8_ep"]["kernel_ms"] / legs["f32_ldsep"]["kernel_ms"], 3),
               build=_lib.source_hash(), device=torch.cuda.get_device_name(0))
    print("ROW " + json.dumps(row), flush=True)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=9)
    ap.add_argument("--batches", type=int, nargs="*", default=list(BATCHES))
    ap.add_argument("--codes", nargs="*", default=list(CODES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "i8_ep_rate.json"))
    ap.add_argument("--child", nargs=3, metavar=("CODE", "ALGO", "BATCH"), help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a.child[0], a.child[1], int(a.child[2]), a.steps)
    rows = []
    for name in a.codes:
        for algo in ALGOS:
            for batch in a.batches:
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--steps", str(a.steps), "--child", name,
                                    algo, str(batch)], stdout=subprocess.PIPE, text=True, timeout=120)
                if r.returncode != 0:      # a failed configuration ends the run: nothing more is started
                    print("configuration %s %s %d failed with status %d" % (name, algo, batch, r.returncode),
                          file=sys.stderr)
                    return 1
                (line,) = [ln for ln in r.stdout.splitlines() if ln.startswith("ROW ")]
                rows.append(json.loads(line[4:]))
                print(line, flush=True)
    build, device = rows[0].pop("build"), rows[0].pop("device")
    for r in rows[1:]:
        assert (r.pop("build"), r.pop("device")) == (build, device)
    res = dict(tool="i8_ep_rate", build=build, device=device, iters=ITERS, ebn0=EBN0, steps_each=a.steps, rows=rows,
               ep_beats_lds_everywhere=all(r["ep_over_lds"] < 1.0 for r in rows),
               ep_loses_to_lds_at=[[r["code"], r["algo"], r["batch"]] for r in rows if r["ep_over_lds"] >= 1.0])
    line = json.dumps(res)
    print(line, flush=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
