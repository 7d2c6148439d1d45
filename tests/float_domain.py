"""Shared inputs and oracle helper of the float-domain tests
(test_float_domain_cpu.py, test_gpu_float_domain.py): float LLRs on a dyadic
grid, so that the min1 / min2 reductions of the float kernels meet ties and
zeros, with -0.0, and scaled into the subnormal and the large range.  A plain
helper module, like param_domain.py, whose splitmix64 streams it draws from
(stream numbers 10 and up), so nothing depends on a numpy RNG stream.

Why a grid: every value is a small multiple of `step` (a power of two).  Plain
and offset min-sum with a dyadic beta then never round in float32 -- sub, add,
min, max and abs of multiples of 2^-1 far below 2^24 are exact -- so a kernel
that differs from the serial float decode (oracle/ldpc_oracle.c
oracle_decode_f32) on such an input differs in logic, not in rounding.  Scaling
by a power of two keeps that: x * 2^-130 makes every nonzero value of the fine
grid subnormal (a multiple of 2^-131), x * 2^100 makes them large.
"""
import math

import numpy as np

import oracle as O
from ldpcgputegra_amd import load_table
from param_domain import _draw32

COARSE = (1.0, 4)      # (step, clip): values k * step, |k| <= clip
FINE = (0.5, 16)
GRIDS = {"coarse": COARSE, "fine": FINE}
SCALES = {"sub": 2.0 ** -130, "big": 2.0 ** 100}

SHORT = ["648x324", "576x288", "200x100", "1944x972"]
DVBS2 = ["dvbs2_r1_2", "dvbs2_r2_3", "dvbs2shape_r3_4", "dvbs2shape_r5_6", "dvbs2_r8_9", "dvbs2_r9_10"]
# Eb/N0 per code: where 16 iterations of min-sum stop some codewords early, not all at the same iteration
# (r3/4 and r8/9, which have no early-termination case, sit between their neighbours)
EBN0 = {"648x324": 2.0, "576x288": 2.0, "200x100": 2.0, "1944x972": 2.0, "dvbs2_r1_2": 2.0, "dvbs2_r2_3": 2.6,
        "dvbs2shape_r3_4": 3.0, "dvbs2shape_r5_6": 3.5, "dvbs2_r8_9": 4.2, "dvbs2_r9_10": 4.4}
# the batch-edge tests (test_gpu_buffer_domain.py): 65 codewords of the fine grid, 16 iterations of min-sum.  r1/2
# at its EBN0 stops every codeword (codewords 0 .. 16 after 7 .. 9 iterations, codeword 64 after 8); r8/9 at 3.7 dB
# leaves 37 of the 65 running, codeword 64 among them (codewords 0 .. 16: 10 .. 16).  At 3.8 dB codeword 64 stops,
# at 3.6 dB none of the first 17 does.
EDGE_EBN0 = {"dvbs2_r1_2": 2.0, "dvbs2_r8_9": 3.7}
STREAM = 10            # grid_input draws from streams `stream` and `stream + 1`

_inputs = {}


def table_grid(t, batch, ebn0, step, clip, stream=STREAM):
    """float32 [batch, N] for the Table t, read-only, not cached: BPSK
    all-zero-codeword AWGN LLRs 2 y / sigma^2, y = -1 + sigma g, rounded to
    multiples of `step` and clipped to +-clip * step.  g by Box-Muller in
    float64 from the splitmix64 streams `stream` and `stream + 1`; sigma =
    sqrt(1 / (2 R 10^(ebn0 / 10))).  Zeros are +0.0.  The draws are indexed by
    position, so a smaller batch is a prefix of a larger one."""
    sigma = math.sqrt(1.0 / (2.0 * (t.k_info / t.n) * 10.0 ** (ebn0 / 10.0)))
    u1 = (_draw32(batch, t.n, stream).astype(np.float64) + 0.5) / 2.0 ** 32      # in (0, 1): log is finite
    u2 = _draw32(batch, t.n, stream + 1).astype(np.float64) / 2.0 ** 32
    g = np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * math.pi * u2)
    llr = 2.0 * (-1.0 + sigma * g) / (sigma * sigma)
    x = (np.clip(np.rint(llr / step), -clip, clip) * step + 0.0).astype(np.float32)   # + 0.0: rint's -0.0
    x = np.ascontiguousarray(x)
    x.setflags(write=False)
    return x


def grid_input(code, batch, ebn0, step, clip, stream=STREAM):
    """table_grid for the shipped table `code`, cached."""
    key = (code, batch, ebn0, step, clip, stream)
    if key not in _inputs:
        _inputs[key] = table_grid(load_table(code), batch, ebn0, step, clip, stream)
    return _inputs[key]


def grid(code, batch, name, stream=STREAM):
    """grid_input at the code's EBN0 on the named grid ("coarse" / "fine")."""
    return grid_input(code, batch, EBN0[code], *GRIDS[name], stream=stream)


def negzero(x):
    """x with every zero made -0.0, and every 7th column made -0.0 as well."""
    y = np.array(x, dtype=np.float32)
    y[y == 0.0] = -0.0
    y[:, ::7] = -0.0
    y.setflags(write=False)
    return y


def scaled(x, scale):
    """x * scale for a power of two `scale`: exact (checked), float32, read-only."""
    y = (x.astype(np.float64) * scale).astype(np.float32)
    assert np.array_equal(y.astype(np.float64), x.astype(np.float64) * scale)
    y.setflags(write=False)
    return y


def make(code, batch, kind):
    """The named input, cached: "coarse", "fine", "negzero" (of coarse), "sub"
    and "big" (fine times SCALES)."""
    key = ("made", code, batch, kind)
    if key not in _inputs:
        if kind in GRIDS:
            _inputs[key] = grid(code, batch, kind)
        elif kind == "negzero":
            _inputs[key] = negzero(grid(code, batch, "coarse"))
        else:
            _inputs[key] = scaled(grid(code, batch, "fine"), SCALES[kind])
    return _inputs[key]


def first_iteration_shares(table, x):
    """(share of checks whose two smallest |LLR| are equal, share of checks
    whose smallest |LLR| is 0), over all checks of all codewords of x: what
    the min1 / min2 reductions meet in the first iteration."""
    a = np.abs(np.asarray(x, dtype=np.float32))
    ev = np.asarray(table.edge_var, dtype=np.int64)
    ties = zeros = checks = 0
    pos = 0
    for d, cnt in zip(table.group_deg, table.group_cnt):
        d, cnt = int(d), int(cnt)
        idx = ev[pos:pos + d * cnt].reshape(cnt, d)
        pos += d * cnt
        two = np.partition(a[:, idx], 1, axis=-1)[..., :2]       # [batch, cnt, 2]: min1, min2
        ties += int((two[..., 0] == two[..., 1]).sum())
        zeros += int((two[..., 0] == 0.0).sum())
        checks += two.shape[0] * two.shape[1]
    return ties / checks, zeros / checks


# ---- oracle ---------------------------------------------------------------

_oracle = {}


def oracle_f32(code, key, llr, algo, beta, iters, early=False):
    """(hard, soft, iters_used) of oracle.decode_f32 on llr (float32 [B, N]),
    read-only and cached per (code, input, algo, beta, iters, early); `key`
    names the input; algo is O.OMS (beta 0: plain min-sum) or O.NMS.  The
    codewords are spread over oracle.host_threads() threads."""
    ck = (code, key, algo, float(beta), iters, bool(early))
    if ck not in _oracle:
        out = O.decode_f32(load_table(code), llr, iters, algo, beta, early_term=early, threads=O.host_threads())
        for a in out:
            a.setflags(write=False)
        _oracle[ck] = out
    return _oracle[ck]


def oracle_on(code, batch, kind, algo, beta, iters, early=False):
    """oracle_f32 on the named input of make().  For "sub" / "big" (O.OMS
    only), beta is the unscaled offset and the oracle gets beta * scale, like
    the input."""
    assert algo == O.OMS or kind not in SCALES
    s = SCALES.get(kind, 1.0)
    return oracle_f32(code, (kind, batch), make(code, batch, kind), algo, beta * s, iters, early)
