"""The float layered min-sum restated in numpy float64: check-serial like the
oracle (oracle/ldpc_oracle.c oracle_decode_f32), vectorised over the batch, and
sharing no code with it.  On float_domain's dyadic grids plain and offset
min-sum with a dyadic offset never round, in float32 or in float64, so the two
must agree exactly (tests/test_float_short_cpu.py); normalised min-sum rounds
after a few layers and is not compared.

The comparisons are the oracle's: an edge is negative if c < 0 (false for
-0.0), a hard decision is v > 0.
"""
import numpy as np

OMS, NMS = 0, 1      # oracle.OMS / oracle.NMS; OMS with beta 0 is plain min-sum


def decode(table, llr, iters, algo=OMS, beta=0.0, early=False):
    """(hard uint8 [B, N], soft float32 [B, N], iters_used int32 [B]).  With
    `early` a codeword stops after the first iteration that leaves the syndrome
    of its hard decisions zero."""
    v = np.array(llr, dtype=np.float64)
    B = v.shape[0]
    ev = np.asarray(table.edge_var, dtype=np.int64)
    msg = np.zeros((B, len(ev)), dtype=np.float64)
    used = np.zeros(B, dtype=np.int32)
    running = np.arange(B)
    for _ in range(iters):
        if not len(running):
            break
        vr, mr = v[running], msg[running]
        pos = 0
        for d, cnt in zip(table.group_deg, table.group_cnt):
            d = int(d)
            for _ in range(int(cnt)):
                idx = ev[pos:pos + d]
                c = vr[:, idx] - mr[:, pos:pos + d]
                a = np.abs(c)
                neg = c < 0.0
                two = np.sort(a, axis=1)[:, :2]
                min1, min2 = two[:, :1], two[:, 1:]
                if algo == NMS:
                    cst1, cst2 = min2 * beta, min1 * beta
                else:
                    cst1, cst2 = np.maximum(min2 - beta, 0.0), np.maximum(min1 - beta, 0.0)
                r = np.where(a == min1, cst1, cst2)
                odd = ((neg.sum(axis=1, keepdims=True) + d) & 1).astype(bool)      # all the signs, and the degree flip
                m = np.where(odd ^ neg, -r, r)
                mr[:, pos:pos + d] = m
                vr[:, idx] = c + m
                pos += d
        v[running], msg[running] = vr, mr
        used[running] += 1
        if early:
            running = running[syndrome(table, v[running] > 0.0) != 0]
    return (v > 0.0).astype(np.uint8), v.astype(np.float32), used


def syndrome(table, hard):
    """Unsatisfied checks per codeword of hard [B, N]."""
    ev = np.asarray(table.edge_var, dtype=np.int64)
    hard = np.asarray(hard).astype(np.int64)
    bad = np.zeros(hard.shape[0], dtype=np.int64)
    pos = 0
    for d, cnt in zip(table.group_deg, table.group_cnt):
        d, cnt = int(d), int(cnt)
        idx = ev[pos:pos + d * cnt].reshape(cnt, d)
        bad += (hard[:, idx].sum(axis=2) & 1).sum(axis=1)
        pos += d * cnt
    return bad
