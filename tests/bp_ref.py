"""Layered belief propagation restated in numpy (a helper, not a test): the
definition of DESIGN.md §3 "Belief propagation", vectorised over the codewords,
one Python loop over the checks.

It shares one thing with the product: the box-plus, taken from
``ldpc_boxplus_f32_host`` (test_bp_cpu.py holds that one against float64).
The schedule -- table order, t = V - m, the forward / backward recursion, the
message and V update, the hard decision and the early termination -- is
restated here, so a host decoder that walks the table differently from the
definition does not agree with it.  Every float32 operation outside the
box-plus is one numpy float32 subtraction or addition: correctly rounded, as
in the decoders.
"""
import numpy as np

from ldpcgputegra_amd import boxplus_host

INPUT_SEED = 77       # channel.awgn_f32_host seed of the unrounded inputs
SANITY = dict(code="648x324", ebn0=2.0, frames=2000, iters=20, seed=5)


def boxplus(a, b):
    return boxplus_host(np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32))


# ---- g and the box-plus: float32 restatement, float64 truth, inputs ---------

F = np.float32
G_CUT = F(18.0)
INV_LN2 = F(float.fromhex("0x1.715476p+0"))
LN2_HI = F(float.fromhex("0x1.62e4p-1"))
LN2_LO = F(float.fromhex("0x1.7f7d1cp-20"))
EXP_C = [F(float.fromhex(c)) for c in ("0x1p+0", "-0x1p+0", "0x1p-1", "-0x1.555556p-3", "0x1.555462p-5",
                                       "-0x1.1110a4p-7", "0x1.6da9a4p-10", "-0x1.a18p-13")]
LOG_C = [F(float.fromhex(c)) for c in ("0x1.fffffep-1", "-0x1.fffe8cp-2", "0x1.552d74p-2", "-0x1.fca104p-3",
                                       "0x1.86b1c8p-3", "-0x1.1692ecp-3", "0x1.3d816ep-4", "-0x1.dc5944p-6",
                                       "0x1.4ff184p-8")]


def g32(x):
    """csrc/bp_math.h bp_g restated in numpy float32, operation by operation
    (test_bp_cpu.py ties it to the product through the box-plus: box32 built
    on it equals ldpc_boxplus_f32_host bit for bit)."""
    x = np.asarray(x, dtype=F)
    xc = np.minimum(x, G_CUT)
    k = np.trunc(xc * INV_LN2 + F(0.5)).astype(np.int32)
    kf = k.astype(F)
    r = (xc - kf * LN2_HI) - kf * LN2_LO
    p = np.full_like(r, EXP_C[7])
    for c in EXP_C[6::-1]:
        p = p * r + c
    u = p * ((127 - k) << 23).astype(np.int32).view(F)
    q = np.full_like(r, LOG_C[8])
    for c in LOG_C[7::-1]:
        q = q * u + c
    return np.where(x < G_CUT, q * u, F(0.0)).astype(F)


def box32(a, b):
    """bp_boxplus restated in numpy float32."""
    a, b = np.asarray(a, dtype=F), np.asarray(b, dtype=F)
    x, y = np.abs(a), np.abs(b)
    d = (np.minimum(x, y) + g32(x + y)) - g32(np.abs(x - y))
    r = np.where(d > 0, d, F(0.0)).astype(F)
    return np.where((a < 0) == (b < 0), -r, r).astype(F)


def g64(x):
    """ln(1 + e^-x) in float64."""
    return np.log1p(np.exp(-np.asarray(x, dtype=np.float64)))


def box64(a, b):
    """The exact box-plus of this project's sign rule, in float64 through the
    identity the float32 one uses (= -2 atanh(tanh(a/2) tanh(b/2)) for a, b != 0)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    x, y = np.abs(a), np.abs(b)
    r = np.minimum(x, y) + g64(x + y) - g64(np.abs(x - y))
    return np.where((a < 0) == (b < 0), -r, r)


def g_boundaries():
    """float32 x >= 0 on both sides of every point where g changes its path:
    the range-reduction boundaries (k + 1/2) ln 2, k = 0 .. 25, and the cutoff,
    each with the 8 floats below and above it."""
    pts = [(k + 0.5) * np.log(2.0) for k in range(26)] + [float(G_CUT)]
    out = []
    for p in pts:
        c = np.array([p], dtype=F).view(np.uint32)[0]
        out.append((np.arange(-8, 9, dtype=np.int64) + int(c)).astype(np.uint32).view(F))
    return np.concatenate(out)


GRID = np.array([0.0, 2.0 ** -149, 2.0 ** -140, 2.0 ** -127] + [2.0 ** e for e in range(-20, 7)] + [1e30], dtype=F)
N_RANDOM = 2 * 1024 * 1024      # pairs per random range (two ranges: >= 4e6 in all)
_cache = {}


def pairs():
    """(a, b): the box-plus input set of test_bp_cpu.py and test_gpu_bp.py,
    float32, read-only, cached.  In order: N_RANDOM pairs uniform in +-40 and
    N_RANDOM in +-2 (splitmix64 streams 30 .. 33 of param_domain); the grid
    +-GRID x +-GRID (the zeros of both signs); equal magnitudes of every sign
    (the grid's and 4096 random ones); pairs whose |a| + |b| or ||a| - |b|| is a
    boundary value of g (g_boundaries), in every sign combination."""
    if "pairs" not in _cache:
        from param_domain import _draw32

        def uni(stream, lim):
            return ((_draw32(1, N_RANDOM, stream)[0].astype(np.float64) + 0.5) / 2.0 ** 32 * 2 * lim - lim).astype(F)
        A = [uni(30, 40.0), uni(32, 2.0)]
        Bv = [uni(31, 40.0), uni(33, 2.0)]
        sg = np.concatenate([GRID, -GRID])              # -GRID[0] is -0.0
        ga, gb = np.meshgrid(sg, sg, indexing="ij")
        A.append(ga.ravel())
        Bv.append(gb.ravel())
        mags = np.concatenate([GRID, np.abs(A[0][:4096])])
        bnd = g_boundaries()
        half = (bnd.astype(np.float64) / 2).astype(F)
        one = np.ones_like(bnd)
        for sa in (1, -1):
            for sb in (1, -1):
                A += [F(sa) * mags, F(sa) * half, F(sa) * (bnd + one)]
                Bv += [F(sb) * mags, F(sb) * (bnd - half), F(sb) * one]
        a, b = np.ascontiguousarray(np.concatenate(A)), np.ascontiguousarray(np.concatenate(Bv))
        a.setflags(write=False)
        b.setflags(write=False)
        _cache["pairs"] = (a, b)
    return _cache["pairs"]


def check_rows(table):
    """[(first edge, degree)] of the checks in table (= schedule) order."""
    rows, pos = [], 0
    for d, cnt in zip(table.group_deg, table.group_cnt):
        for _ in range(int(cnt)):
            rows.append((pos, int(d)))
            pos += int(d)
    return rows


def syndrome_ok(table, rows, V):
    """[B] bool: the hard decisions V > 0 satisfy every check."""
    ev = np.asarray(table.edge_var, dtype=np.int64)
    hard = (V > 0).astype(np.uint8)
    bad = np.zeros(V.shape[0], dtype=np.uint8)
    for e0, d in rows:
        bad |= np.bitwise_xor.reduce(hard[:, ev[e0:e0 + d]], axis=1)
    return bad == 0


def decode(table, llr, iters, early=False):
    """(hard uint8 [B, N], soft float32 [B, N], iters_used int32 [B]) of
    layered BP on llr (float32 [B, N]).  With `early`, a codeword stops after
    the first whole iteration whose hard decisions satisfy H; its state is
    frozen from then on."""
    ev = np.asarray(table.edge_var, dtype=np.int64)
    rows = check_rows(table)
    V = np.array(llr, dtype=np.float32)
    B = V.shape[0]
    msg = np.zeros((B, len(ev)), dtype=np.float32)
    live = np.ones(B, dtype=bool)
    used = np.zeros(B, dtype=np.int32)
    for _ in range(iters):
        if not live.any():
            break
        Vl, ml = V[live], msg[live]
        for e0, d in rows:
            v = ev[e0:e0 + d]
            t = Vl[:, v] - ml[:, e0:e0 + d]                       # [b, d]
            new = np.empty_like(t)
            if d == 2:
                new[:, 0], new[:, 1] = t[:, 1], t[:, 0]
            else:
                Fw = [t[:, 0]]                                    # F_0 .. F_{d-2}
                for j in range(1, d - 1):
                    Fw.append(boxplus(Fw[j - 1], t[:, j]))
                Bk = t[:, d - 1]                                  # B_{j+1}, j going down
                new[:, d - 1] = Fw[d - 2]
                for j in range(d - 2, 0, -1):
                    new[:, j] = boxplus(Fw[j - 1], Bk)
                    Bk = boxplus(t[:, j], Bk)
                new[:, 0] = Bk
            ml[:, e0:e0 + d] = new
            Vl[:, v] = t + new
        V[live], msg[live] = Vl, ml
        used[live] += 1
        if early:
            idx = np.flatnonzero(live)
            live[idx[syndrome_ok(table, rows, V[idx])]] = False
    return (V > 0).astype(np.uint8), V, used
