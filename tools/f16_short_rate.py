#!/usr/bin/env python3
"""What the binary16 decode costs on the packed LDS-resident kernel (csrc/ldsh*,
family 7) and the packed any-H kernel (csrc/generich.hip, family 1), beside the
float32 decode of the same build, as one JSON line, also written to
profiles/f16_short_rate.json.  20 iterations of plain min-sum, no early
termination, true LLRs at 2.0 dB.  Legs, alternated step by step in one run on
one device, each step one decode timed with device events, the median kept:

  648x324 and 200x100 (the two shipped tables ldsh can run at more than one
  shape) at 1024 / 4096 / 16384 / 65536 codewords
    f16_auto   decode_f16_device on family 7 at the shape its rule picks
    f16_l<L>   the same at each shape the code can run (LDPC_LDSH_LANES forces it)
    f32_k7     decode_f32_device forced to family 7
    f32_auto   decode_f32_device at its automatic choice (648x324: ldsep)
  4000x2000 at 4096 codewords
    f16_k1 / f32_k1   both decodes on family 1

Nothing here gates anything: the file reports, per batch, whether the shape rule
(launch_lds's, with pairs in place of the batch) picked the fastest measured
shape, and the ratios README and DESIGN.md quote.

GPU box:  python tools/f16_short_rate.py [--steps 9]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ldpcgputegra_amd import ALGO_MS, Code, Decoder, _lib, channel, default_params  # noqa: E402

ITERS, EBN0 = 20, 2.0
LDS_CODES, LDS_BATCHES = ("648x324", "200x100"), (1024, 4096, 16384, 65536)
GEN_CODE, GEN_BATCH = "4000x2000", 4096
LANES = (8, 16, 32, 64)


def legal_lanes(code):
    """the shapes ldsh can run: at least the lanes the widest layer needs, the pairs of a wave within 64 KB"""
    import ctypes as C
    nl, mw, i8, f32 = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    _lib.check(_lib.lib().ldpc_code_layer_info(code.handle, C.byref(nl), C.byref(mw), C.byref(i8), C.byref(f32)))
    need = 8 if mw.value <= 8 else 16 if mw.value <= 16 else 32 if mw.value <= 32 else 64
    e = len(code.table().edge_var)
    return [L for L in LANES if f32.value and L >= need and
            (2 * e + 15) // 16 * 16 + (64 // L) * (code.n + e) * 4 <= 64 * 1024]


def measure(torch, code, batch, steps, legs_of):
    """legs_of(decoders) -> [(name, decoder, "f16" | "f32", forced lanes or 0, expected last_kernel)]"""
    n, k = code.n, code.k_info
    sigma = channel.sigma_from_ebn0(EBN0, k / n)
    decs = dict(f16=Decoder(code, max_batch=batch, f16_all_codes=True), f32=Decoder(code, max_batch=batch),
                f32_forced=Decoder(code, max_batch=batch))
    legs = legs_of(decs)
    y = torch.empty((batch, n), dtype=torch.float32, device="cuda")
    h = torch.empty((batch, n), dtype=torch.float16, device="cuda")
    hard = torch.empty((batch, n), dtype=torch.uint8, device="cuda")
    decs["f32"].awgn_f32_device(y, 0, 1, sigma, normalize=True)
    decs["f32"].convert_f16_device(y, h)
    torch.cuda.synchronize()
    ms = default_params(algo=ALGO_MS, beta=0.0)
    shapes, kernels = {}, {}

    def step(leg):
        name, dec, kind, lanes, kernel = leg
        if lanes:
            os.environ["LDPC_LDSH_LANES"] = str(lanes)
        else:
            os.environ.pop("LDPC_LDSH_LANES", None)
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        if kind == "f16":
            dec.decode_f16_device(h, hard, ITERS, params=ms)
        else:
            dec.decode_f32_device(y, hard, ITERS, params=ms)
        t1.record()
        torch.cuda.synchronize()
        os.environ.pop("LDPC_LDSH_LANES", None)
        assert kernel is None or dec.last_kernel == kernel, (name, dec.last_kernel)
        kernels[name] = dec.last_kernel
        shapes[name] = dec.last_lds_shape
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
        out[name] = dict(step_ms=round(med, 4), min_ms=round(min(v), 4), max_ms=round(max(v), 4), steps=len(v),
                         spread=round((max(v) - min(v)) / med, 4), frame_errors=fe[name],
                         kernel=kernels[name], lanes=shapes[name][0], split=shapes[name][1], coded_mbps=round(batch * n / med / 1e3, 1))
    for d in decs.values():
        d.close()
    del y, h, hard
    torch.cuda.empty_cache()
    assert len({d["frame_errors"] for n_, d in out.items() if n_.startswith("f16_")}) == 1, out   # one result at every shape
    return out


def lds_row(torch, name, code, batch, steps):
    lanes = legal_lanes(code)

    def legs_of(d):
        d["f16"].set_kernel(7)
        d["f32_forced"].set_kernel(7)
        return [("f16_auto", d["f16"], "f16", 0, "lds")] + [("f16_l%d" % L, d["f16"], "f16", L, "lds") for L in lanes] + \
            [("f32_k7", d["f32_forced"], "f32", 0, "lds"), ("f32_auto", d["f32"], "f32", 0, None)]

    out = measure(torch, code, batch, steps, legs_of)
    forced = [n_ for n_ in out if n_.startswith("f16_l")]
    best = min(forced, key=lambda n_: out[n_]["step_ms"])
    picked = "f16_l%d" % out["f16_auto"]["lanes"]
    spread = max(out[picked]["spread"], out[best]["spread"])
    return dict(code=name, batch=batch, shapes=lanes,
                rule_lanes=out["f16_auto"]["lanes"], fastest_lanes=int(best.rsplit("l", 1)[1]), legs=out,
                rule_is_fastest=out[picked]["step_ms"] <= out[best]["step_ms"] * (1.0 + spread), rule_spread=spread,
                f16_over_f32_k7=round(out["f16_auto"]["step_ms"] / out["f32_k7"]["step_ms"], 3),
                f16_over_f32_auto=round(out["f16_auto"]["step_ms"] / out["f32_auto"]["step_ms"], 3),
                f16_best_over_f32_auto=round(out[best]["step_ms"] / out["f32_auto"]["step_ms"], 3))


def gen_row(torch, code, batch, steps):
    def legs_of(d):
        d["f16"].set_kernel(1)
        d["f32_forced"].set_kernel(1)
        return [("f16_k1", d["f16"], "f16", 0, "generic"), ("f32_k1", d["f32_forced"], "f32", 0, "generic")]

    out = measure(torch, code, batch, steps, legs_of)
    return dict(code=GEN_CODE, batch=batch, legs=out,
                f16_over_f32=round(out["f16_k1"]["step_ms"] / out["f32_k1"]["step_ms"], 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=9)
    ap.add_argument("--batches", type=int, nargs="*", default=list(LDS_BATCHES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "f16_short_rate.json"))
    a = ap.parse_args()
    import torch
    rows = [lds_row(torch, name, Code(name), b, a.steps) for name in LDS_CODES for b in a.batches]
    gen = gen_row(torch, Code(GEN_CODE), GEN_BATCH, a.steps)
    res = dict(tool="f16_short_rate", build=_lib.source_hash(), device=torch.cuda.get_device_name(0), iters=ITERS,
               ebn0=EBN0, algo="MS", steps_each=a.steps, lds=rows, generic=gen,
               rule_is_fastest=all(r["rule_is_fastest"] for r in rows))
    line = json.dumps(res)
    print(line, flush=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
