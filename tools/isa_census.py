#!/usr/bin/env python3
"""ISA census of a kernel: instruction classes per region between barriers.

usage: isa_census.py <lib.so | obj.o | file.s> [kernel-substring] [--min-valu N]
Prints, for every region between two s_barrier of the chosen kernel(s), its
ISA line span and the counts of VALU (v_*), packed-16 VALU (v_pk_*), SALU
(s_*), LDS (ds_*), VMEM (buffer/global) and s_nop instructions, plus a
per-mnemonic histogram of the largest straight-line region of each kind
(--hist).  Used for coop3's per-period VALU census.
"""
import argparse
import collections
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import check_vmcnt  # noqa: E402


def classify(mn):
    if mn.startswith("v_"):
        return "valu"
    if mn.startswith("ds_"):
        return "lds"
    if mn.startswith(("buffer_", "global_", "scratch_", "flat_")):
        return "vmem"
    if mn == "s_nop":
        return "nop"
    if mn.startswith("s_"):
        return "salu"
    return "other"


def regions(lines):
    cur, start = [], 0
    for i, l in enumerate(lines):
        mn = l.split()[0] if l.split() else ""
        if mn == "s_barrier":
            yield start, i, cur
            cur, start = [], i + 1
        else:
            cur.append(mn)
    yield start, len(lines), cur


_ADDR = re.compile(r"//\s*([0-9A-Fa-f]{8,16}):")


def _addr(line):
    m = _ADDR.search(line)
    return int(m.group(1), 16) if m else None


def pass_through_skips(L, mn, s, e):
    """The wave-uniform branches around the pre's pass-through block inside
    lines [s, e): {branch line: line of its target} for every conditional
    forward branch that jumps over at most 16 instructions, all VALU (or the
    exec save / restore around them), with the block's six selects among them
    (v_cndmask_b32, or v_mov_b32 under exec).  A slab wave outside the plan's
    pass-through mask takes the branch; the others fall through."""
    out = {}
    for j in range(s, e):
        if not mn[j].startswith("s_cbranch"):
            continue
        a = _addr(L[j])
        try:
            off = int(L[j].split()[1], 0)
        except (IndexError, ValueError):
            continue
        if a is None or off <= 0:
            continue
        target = a + 4 + 4 * off
        t = j + 1
        while t < e and _addr(L[t]) is not None and _addr(L[t]) < target:
            t += 1
        span = mn[j + 1:t]
        if t < e and _addr(L[t]) == target and len(span) <= 16 \
                and all(m.startswith("v_") or m in ("s_and_saveexec_b64", "s_or_b64") for m in span) \
                and sum(1 for m in span if m.startswith(("v_cndmask_b32", "v_mov_b32"))) >= 6:
            out[j] = t
    return out


def coop3_slab_paths(L, mn):
    """The unrolled steady periods of the slab waves (the barrier-delimited
    regions holding all the fast-period variants: > 700 VALU), each split at
    its branches.  The last four large blocks of a region are the post-first
    path (waves 0-2: post + the pre's reads, then the pre) and the pre-first
    path (waves 3-5: reads + pre, then the post); what precedes them is the
    shared prefix and the guarded tail-window variant.

    A branch around the pre's pass-through block (pass_through_skips) does not
    split a block: post_first / pre_first count the path of a wave that runs
    the block (every instruction of the path, as before there was a branch),
    post_first_skip / pre_first_skip the path of a wave that branches around
    it, and pt_valu the block's VALU instructions per path."""
    out = []
    start = 0
    keys = ("valu", "lds", "nop", "waitcnt")
    for i, m in enumerate(mn + ["s_barrier"]):
        if m != "s_barrier":
            continue
        s, e, start = start, i, i + 1
        if sum(1 for x in mn[s:e] if x.startswith("v_")) <= 700:
            continue
        skips = pass_through_skips(L, mn, s, e)
        marks = [s - 1] + [j for j in range(s, e)
                           if mn[j].startswith(("s_cbranch", "s_branch")) and j not in skips] + [e]
        blk = []
        for x, y in zip(marks, marks[1:]):
            c = collections.Counter(classify(m2) for m2 in mn[x + 1:y])
            d = dict(valu=c["valu"], lds=c["lds"], nop=c["nop"],
                     waitcnt=sum(1 for m2 in mn[x + 1:y] if m2 == "s_waitcnt"))
            # what a wave taking the block's pass-through branches does not run
            sk = [m2 for j, t in skips.items() if x < j < y for m2 in mn[j + 1:t]]
            c = collections.Counter(classify(m2) for m2 in sk)
            d["skipped"] = dict(valu=c["valu"], lds=c["lds"], nop=c["nop"],
                                waitcnt=sum(1 for m2 in sk if m2 == "s_waitcnt"))
            blk.append(d)
        big = [b for b in blk if b["valu"] >= 50]
        if len(big) < 4:
            continue
        path = lambda bs: {k: sum(b[k] for b in bs) for k in keys}  # noqa: E731
        skip = lambda bs: {k: sum(b[k] - b["skipped"][k] for b in bs) for k in keys}  # noqa: E731
        ptv = lambda bs: sum(b["skipped"]["valu"] for b in bs)  # noqa: E731
        out.append(dict(lines=[s, e], valu=sum(b["valu"] for b in blk), post_first=path(big[-4:-2]),
                        pre_first=path(big[-2:]), post_first_skip=skip(big[-4:-2]), pre_first_skip=skip(big[-2:]),
                        pt_valu=dict(post_first=ptv(big[-4:-2]), pre_first=ptv(big[-2:])),
                        pass_through_branches=len(skips)))
    return out


def _counts(mns):
    c = collections.Counter(classify(m) for m in mns)
    return dict(valu=c["valu"], salu=c["salu"] - sum(1 for m in mns if m == "s_waitcnt"), lds=c["lds"],
                vmem=c["vmem"], waitcnt=sum(1 for m in mns if m == "s_waitcnt"), nop=c["nop"], all=len(mns))


def coop3_memory_periods(L, mn):
    """The memory wave's steady periods: the straight-line regions between two
    period-closing vmcnt waits that hold its s_sleep (the prologue's gathers
    sit between two such waits too, but sleep nowhere)."""
    w = [i for i, l in enumerate(L) if "vmcnt(" in l and check_vmcnt.closes_period(L, i)]
    out = []
    for x, y in zip(w, w[1:]):
        body = mn[x + 1:y]
        if "s_sleep" not in body or any(m.startswith(("s_cbranch_scc", "s_cbranch_vcc", "s_branch")) for m in body):
            continue
        d = _counts(body)
        d.update(lines=[x, y], valu_lane_ops_per_check_cw=round(d["valu"] * 64 / (48 * 16), 2))
        out.append(d)
    return out


def coop3_chain_window(mn):
    """The chain wave's window (fixed-iteration kernels hold one: every
    v_pk_mad_i16 of the kernel is a chain step): from the branch that guards it
    to the end of its last step, and per block of 8 steps (from its first step
    to the next block's) the constant reads, how many of them directly follow
    a step's last instruction (LDPC_C3_CHAIN_RD1 puts every one there), the
    x-input writes, the waits and the s_nop."""
    mad = [i for i, m in enumerate(mn) if m == "v_pk_mad_i16"]
    if len(mad) < 16 or len(mad) % 8:
        return None
    b = mad[0]
    while not mn[b].startswith(("s_cbranch", "s_branch", "s_barrier")):
        b -= 1
    e = mad[-1]
    while mn[e] != "v_med3_i16" or mn[e + 1] == "v_med3_i16":
        e += 1   # the step's last v_med3_i16
    out = _counts(mn[b + 1:e + 1])
    out.update(lines=[b + 1, e + 1], steps=len(mad), blocks=[])
    for k in range(0, len(mad), 8):
        x, y = mad[k], mad[k + 8] if k + 8 < len(mad) else e + 1
        rd = [i for i in range(x, y) if mn[i].startswith("ds_read")]
        out["blocks"].append(dict(
            reads=len(rd), reads_after_a_step=sum(1 for i in rd if mn[i - 1] == "v_med3_i16" and mn[i - 2] == "v_med3_i16"),
            writes=sum(1 for i in range(x, y) if mn[i].startswith("ds_write")),
            valu=sum(1 for i in range(x, y) if mn[i].startswith("v_")),
            waitcnt=sum(1 for i in range(x, y) if mn[i] == "s_waitcnt"),
            nop=sum(1 for i in range(x, y) if mn[i] == "s_nop")))
    return out


def coop3_census(funcs, kernel="coop3_decodeILi7ELi6ELi2ELb0ELb0ELb0E"):
    """One steady period of coop3 (DVB-S2 r1/2, WS = 6): the slab waves' fast
    period split at its branches (the shared prefix, the post variants for
    slab wave 0 / the others, the pre), the memory wave's unrolled steady
    periods (coop3_memory_periods), a chain block of 8 steps and the chain
    window with its blocks (coop3_chain_window); VALU also as lane-ops per
    check x codeword (a slab lane = one check x 2 codewords; the memory and
    chain waves serve a window's 48 checks x 16 codewords); and the two slab
    paths of each unrolled steady period (coop3_slab_paths)."""
    name = next(k for k in funcs if kernel in k)
    L = funcs[name]
    mn = [l.split()[0] if l.split() else "" for l in L]
    out = {"kernel": name, "slab_paths_per_unrolled_period": coop3_slab_paths(L, mn)}
    st = [i for i, l in enumerate(L) if mn[i] == "s_setprio" and l.split()[1] == "1"]
    s0 = st[len(st) // 2]
    b = s0
    while not mn[b].startswith("s_cbranch"):
        b -= 1
    e = s0
    while mn[e] != "s_barrier":
        e += 1
    marks = [b] + [i for i in range(b + 1, e) if mn[i].startswith(("s_cbranch", "s_branch"))] + [e]
    parts = []
    for x, y in zip(marks, marks[1:]):
        c = collections.Counter(classify(m) for m in mn[x + 1:y])
        parts.append(dict(lines=[x, y], valu=c["valu"], salu=c["salu"], lds=c["lds"], nop=c["nop"]))
    out["slab_fast_period_blocks"] = parts
    out["memory_wave_periods"] = coop3_memory_periods(L, mn)
    mad = [i for i, m in enumerate(mn) if m == "v_pk_mad_i16"]
    if len(mad) >= 16:
        x, y = mad[8], mad[16]
        c = collections.Counter(classify(m) for m in mn[x:y])
        out["chain_8_steps"] = dict(valu=c["valu"], lds=c["lds"], salu=c["salu"])
    out["chain_window"] = coop3_chain_window(mn)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("path")
    ap.add_argument("kernel", nargs="?", default="coop3_decodeILi7ELi6ELi2ELb0ELb0ELb0E")
    ap.add_argument("--min-valu", type=int, default=100)
    ap.add_argument("--hist", action="store_true")
    ap.add_argument("--coop3", action="store_true", help="coop3 steady-period census as JSON")
    a = ap.parse_args()
    funcs = check_vmcnt.functions(check_vmcnt.disassemble(a.path))
    if a.coop3:
        import json
        print(json.dumps(coop3_census(funcs, a.kernel), indent=1))
        return
    for name, lines in funcs.items():
        if a.kernel not in name:
            continue
        print("==", name)
        for s, e, mns in regions(lines):
            c = collections.Counter(classify(m) for m in mns)
            if c["valu"] < a.min_valu:
                continue
            pk = sum(1 for m in mns if m.startswith("v_pk_"))
            br = sum(1 for m in mns if m.startswith("s_cbranch") or m == "s_branch")
            print("  lines %6d-%6d  valu %4d (pk %3d)  salu %3d  lds %3d  vmem %3d  nop %3d  branches %d"
                  % (s, e, c["valu"], pk, c["salu"], c["lds"], c["vmem"], c["nop"], br))
            if a.hist:
                h = collections.Counter(m for m in mns if m.startswith("v_"))
                print("    " + ", ".join("%s %d" % kv for kv in h.most_common()))


if __name__ == "__main__":
    main()
