"""The half contract ("The half contract") restated in numpy
float16, and the inputs the f16 tests share.

numpy's float16 ``+ - *`` are IEEE binary16 operations rounded to nearest even
(numpy computes them in float32 and rounds once, which gives the same bits), and
its subnormals are kept.  ``decode`` is the serial layered decode, the codewords
of a batch side by side:

* load: V = min(max(llr, -1024), 1024), by comparisons (-0.0 passes);
* c_j = V[v_j] - m_j, a_j = |c_j| (sign bit cleared), min1 / min2 over a_j;
* the sign of a contribution is its sign bit; the check's sign starts at D & 1;
* cst(x) = min(x * beta16, 256) (NMS), min(max(x - beta16, +0), 256) (OMS; MS is
  OMS with beta16 = 0);
* r_j = cst(min2) where a_j == min1, else cst(min1); m'_j = r_j with the sign
  bit sign ^ signbit(c_j); V[v_j] = min(max(c_j + m'_j, -1024), 1024);
* hard = V > 0; with early termination a codeword stops after the first whole
  iteration whose hard decisions satisfy every check.

Everything is kept as uint16 bit patterns where a sign bit matters."""
import numpy as np

from bp_ref import check_rows

H = np.float16
VSAT, MSAT = H(1024.0), H(256.0)
SIGN, ABS = np.uint16(0x8000), np.uint16(0x7FFF)
ALGOS = ("MS", "OMS", "NMS")


def bits(x):
    return np.ascontiguousarray(x, dtype=H).view(np.uint16)


def vals(u):
    return np.ascontiguousarray(u, dtype=np.uint16).view(H)


def clamp_v(x):
    """min(max(x, -1024), 1024) by comparisons: zeros and subnormals pass unchanged."""
    x = np.asarray(x, dtype=H)
    return np.where(x < -VSAT, -VSAT, np.where(x > VSAT, VSAT, x)).astype(H)


def convert(y):
    """RNE16(min(max(y, -1024), 1024)) of float32 y, through float64 (exact) to float16 (one rounding)."""
    y = np.asarray(y, dtype=np.float32).astype(np.float64)
    y = np.where(y < -1024.0, -1024.0, np.where(y > 1024.0, 1024.0, y))
    return y.astype(H)


def cst(x, algo, beta16):
    """x: magnitudes (float16, >= +0)"""
    with np.errstate(over="ignore", invalid="ignore"):
        if algo == "NMS":
            r = (x * beta16).astype(H)
        else:
            r = (x - beta16).astype(H)
            r = np.where(r > H(0.0), r, H(0.0)).astype(H)
    return np.where(r > MSAT, MSAT, r).astype(H)


def syndrome_ok(table, rows, V):
    ev = np.asarray(table.edge_var, dtype=np.int64)
    hard = (V > H(0.0)).astype(np.uint8)
    bad = np.zeros(V.shape[0], dtype=np.uint8)
    for e0, d in rows:
        bad |= np.bitwise_xor.reduce(hard[:, ev[e0:e0 + d]], axis=1)
    return bad == 0


def decode(table, llr, iters, algo="MS", beta=0.0, early=False):
    """(hard uint8 [B, N], soft uint16 bit patterns [B, N], iters_used int32 [B])
    of the binary16 layered decode on llr (float16 or uint16 bit patterns)."""
    assert algo in ALGOS
    llr = np.asarray(llr)
    if llr.dtype == np.uint16:
        llr = llr.view(H)
    beta16 = H(0.0) if algo == "MS" else np.float32(beta).astype(H)
    kind = "NMS" if algo == "NMS" else "OMS"
    ev = np.asarray(table.edge_var, dtype=np.int64)
    rows = check_rows(table)
    V = clamp_v(llr)
    B = V.shape[0]
    msg = np.zeros((B, len(ev)), dtype=H)
    live = np.ones(B, dtype=bool)
    used = np.zeros(B, dtype=np.int32)
    inf = H(np.inf)
    for _ in range(iters):
        if not live.any():
            break
        Vl, ml = V[live], msg[live]
        for e0, d in rows:
            v = ev[e0:e0 + d]
            with np.errstate(over="ignore", invalid="ignore"):
                c = (Vl[:, v] - ml[:, e0:e0 + d]).astype(H)              # [b, d]
            cb = c.view(np.uint16)
            a = (cb & ABS).view(H)
            sign = np.full(c.shape[0], SIGN if d & 1 else 0, dtype=np.uint16)
            min1 = np.full(c.shape[0], inf, dtype=H)
            min2 = min1.copy()
            for j in range(d):
                sign ^= cb[:, j] & SIGN
                t = min1
                min1 = np.minimum(a[:, j], min1)
                min2 = np.minimum(min2, np.maximum(a[:, j], t))
            cst1, cst2 = cst(min2, kind, beta16), cst(min1, kind, beta16)
            r = np.where(a == min1[:, None], cst1[:, None], cst2[:, None]).astype(H)
            mb = (r.view(np.uint16) & ABS) | ((sign[:, None] ^ cb) & SIGN)
            m = mb.view(H)
            ml[:, e0:e0 + d] = m
            with np.errstate(over="ignore", invalid="ignore"):
                Vl[:, v] = clamp_v((c + m).astype(H))
        V[live], msg[live] = Vl, ml
        used[live] += 1
        if early:
            idx = np.flatnonzero(live)
            live[idx[syndrome_ok(table, rows, V[idx])]] = False
    return (V > H(0.0)).astype(np.uint8), V.view(np.uint16).copy(), used


# ---- inputs ----------------------------------------------------------------

F16_STREAM = 40
# values the contract names: zeros of both signs, the smallest and largest subnormal, the smallest normal, the
# clamp edges and what lies beyond them, the largest finite value, the infinities
SPECIAL = np.array([0x0000, 0x8000, 0x0001, 0x8001, 0x03FF, 0x83FF, 0x0400, 0x8400, 0x6400, 0xE400, 0x6401, 0xE401,
                    0x63FF, 0xE3FF, 0x7BFF, 0xFBFF, 0x7C00, 0xFC00, 0x5C00, 0xDC00], dtype=np.uint16)
_inputs = {}


def make_input(batch, n, stream=F16_STREAM):
    """uint16 bit patterns [batch, n], read-only, cached: per element one of
    (a) k / 4 for -32 <= k < 32: ties and zeros in most checks (half the draws);
    (b) a binary16 value spread over the whole exponent range, both signs,
        subnormals included, finite (three draws in eight);
    (c) one of SPECIAL (one draw in eight).  No NaN."""
    key = (batch, n, stream)
    if key not in _inputs:
        from param_domain import _draw32
        r = _draw32(batch, n, stream).astype(np.uint64)
        sel = (r >> np.uint64(29)).astype(np.int64)                  # 0 .. 7
        low = (r & np.uint64(0xFFFF)).astype(np.uint16)
        dyadic = bits(((((r >> np.uint64(8)) & np.uint64(63)).astype(np.float32) - 32.0) * 0.25).astype(H))
        spread = np.where((low & ABS) >= 0x7C00, low & np.uint16(0xFBFF), low).astype(np.uint16)   # inf / NaN -> finite
        special = SPECIAL[((r >> np.uint64(16)) % np.uint64(len(SPECIAL))).astype(np.int64)]
        x = np.where(sel < 4, dyadic, np.where(sel < 7, spread, special)).astype(np.uint16)
        x = np.ascontiguousarray(x)
        assert not np.isnan(x.view(H)).any()
        x.setflags(write=False)
        _inputs[key] = x
    return _inputs[key]
