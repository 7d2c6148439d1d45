#!/usr/bin/env python3
"""What the general encoder costs (csrc/genc.hip, csrc/genc_host.cpp), as one
JSON line -- the sibling of tools/encode_rate.py for the codes that have no
Annex-B table.  For 648x324 and 1944x972 at batch 4096: the time to build the
encoder on the host, the info_bits, general-encode, awgn_i8 and 20-iteration
int8 decode launches timed with device events, and the ldpc_sim step (count
reset, [bits, encode,] channel, decode, count, counters read back) on the
all-zero codeword and on fresh random codewords, alternated in one run.  The
figure to read is step.ratio = fresh / all-zero; no threshold is set.
GPU box:  python tools/genc_rate.py [--batch 4096] [--launches 50] [--steps 30]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ldpcgputegra_amd import Code, Decoder, _lib, channel, default_params  # noqa: E402
from tools.encode_rate import PEAK_GBS, rate, timed  # noqa: E402

CODES = ("648x324", "1944x972")
ITERS = 20
EBN0 = 2.0


def measure(torch, name, B, launches, n_steps):
    code = Code(name)
    n, k = code.n, code.k_info
    t = time.perf_counter()
    enc = code.encoder()
    create_ms = (time.perf_counter() - t) * 1e3
    dec = Decoder(code, max_batch=B)
    dec.set_encoder(enc)
    table = channel.i8_table(channel.sigma_from_ebn0(EBN0, k / n))
    p = default_params(algo=_lib.ALGO_OMS, offset=1)
    info = torch.empty((B, k), dtype=torch.uint8, device="cuda")
    cw = torch.empty((B, n), dtype=torch.uint8, device="cuda")
    llr = torch.empty((B, n), dtype=torch.int8, device="cuda")
    hard = torch.empty((B, n), dtype=torch.uint8, device="cuda")
    cnt = torch.zeros(2, dtype=torch.int64, device="cuda")
    kw = (k + 63) // 64
    kernels = dict(
        info_bits=rate(timed(torch, lambda: dec.info_bits_device(info, 0, 1), launches), B * k),
        # bytes the encoder must move: info in, codeword out (P, rank x kw words, stays in cache)
        encode=rate(timed(torch, lambda: dec.encode_any_device(info, cw), launches), B * (k + n)),
        awgn_i8=rate(timed(torch, lambda: dec.awgn_i8_device(llr, 0, 1, table, codeword=cw), launches), 2 * B * n))
    dec.awgn_i8_device(llr, 0, 1, table, codeword=cw)
    kernels["decode_i8_ms"] = round(timed(torch, lambda: dec.decode_i8_device(llr, hard, ITERS, p), launches), 4)
    kernels["decode_kernel"] = dec.last_kernel
    kernels["encode_gf2_and_xor_per_s"] = round(B * enc.rank * kw / (kernels["encode"]["ms"] * 1e-3), 0)

    def step(fresh, no):
        t = time.perf_counter()
        cnt.zero_()
        ref = None
        if fresh:
            ref = cw
            dec.info_bits_device(info, no * B, 1)
            dec.encode_any_device(info, cw)
        dec.awgn_i8_device(llr, no * B, 1, table, codeword=ref)
        dec.decode_i8_device(llr, hard, ITERS, p)
        dec.count_errors_device(hard, k, cnt, ref=ref)
        c = cnt.cpu().tolist()
        return (time.perf_counter() - t) * 1e3, c

    for no in range(5):
        step(False, no), step(True, no)
    ms = {False: [], True: []}
    fe = {False: 0, True: 0}
    for no in range(n_steps):
        for fresh in (False, True):
            t, c = step(fresh, no)
            ms[fresh].append(t)
            fe[fresh] += c[1]
    dec.close()
    zero, fresh = statistics.median(ms[False]), statistics.median(ms[True])
    return dict(n=n, k=k, rank=enc.rank, systematic=enc.systematic, create_ms=round(create_ms, 3), kernels=kernels,
                step=dict(batch=B, steps_each=n_steps, ebn0=EBN0, iters=ITERS, all_zero_ms=round(zero, 3),
                          fresh_ms=round(fresh, 3), ratio=round(fresh / zero, 4),
                          all_zero_frame_errors=fe[False], fresh_frame_errors=fe[True]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--steps", type=int, default=30)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("genc_rate: no GPU (nothing is measured on the CPU)")
    res = dict(tool="genc_rate", build=_lib.source_hash(), device=torch.cuda.get_device_name(0), batch=a.batch,
               launches=a.launches, peak_gb_per_s=PEAK_GBS)
    res["codes"] = {name: measure(torch, name, a.batch, a.launches, a.steps) for name in CODES}
    print(json.dumps(res), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
