"""Shared inputs, references and literals of the float32 short-code tests
(test_float_short_cpu.py, test_gpu_float_short.py): the float min-sum kernels
of the short codes -- generic (1), lds (7), ldsep (9) -- on synthetic tables of
every check degree (short_domain.synthetic, ldsep_domain.synthetic) and in the
packed launch shapes of kernel 7.  A plain helper module, like float_domain.py,
whose grids, scalings and -0.0 variant it applies to a Table instead of a
shipped code's name.
"""
import numpy as np

import float_domain as FD
import ldsep_domain as ED
import oracle as O
import short_domain as SD
from ldpcgputegra_amd import ALGO_MS, ALGO_NMS, ALGO_OMS, load_table

EBN0 = 2.0
# name -> (product algo, oracle algo, beta).  OMS 4.0 clamps most messages to zero.
ALGOS = {"MS": (ALGO_MS, O.OMS, 0.0), "OMS0.5": (ALGO_OMS, O.OMS, 0.5), "OMS4": (ALGO_OMS, O.OMS, 4.0),
         "NMS0.75": (ALGO_NMS, O.NMS, 0.75)}
EXACT_ALGOS = ("MS", "OMS0.5", "OMS4")      # nothing rounds on a dyadic grid, in float32 or float64

# ---- the tables ------------------------------------------------------------

SWEEP_BATCH, SWEEP_ITERS = 5, 3
EP_BATCH, EP_ITERS = 7, 3
EP_BATCHES = (1, 2, 3, 4, 5, 7)           # every tail of ldsep's 4-codeword workgroup: 1, 2, 3, 0, 1, 3
SHORT_TABLES = [(d, Z) for Z in (SD.Z_SPLIT, SD.Z_LOOP) for d in SD.DEGREES]
# (d, Z) whose float state kernel 7 cannot hold (ldpc_code_layer_info's lds_f32 is 0): none.  The largest, d = 32,
# needs 46 976 (Z = 12, four codewords at 16 lanes) and 50 480 bytes (Z = 40) of the 65 536.
# test_float_short_cpu.test_float_state_fits_lds pins this; the GPU sweep leaves kernel 7 out for a pair listed here.
NO_LDS_F32 = ()
SCALED_DEGREES = (2, 3, 17, 32)           # the sub / big cases of the degree sweep
EP_SCALED_DEGREES = (2, 5, 8)             # ... and of ldsep, on each shape
EP_ET_DEGREES = (2, 8)


def short_table(d, Z):
    return SD.synthetic(d, Z), SD.synthetic_name(d, Z)


def ep_table(d, rows, Z):
    return ED.synthetic(d, rows, Z), ED.synthetic_name(d, rows, Z)


# ---- inputs ----------------------------------------------------------------

_inputs = {}


def synthetic_input(t, key, batch, grid="coarse", ebn0=EBN0):
    """float_domain.table_grid for a synthetic Table, cached under `key` (which
    names the table): the coarse grid at 2 dB unless told otherwise -- BPSK
    all-zero AWGN LLRs rounded to integers and clipped to +-4, from the
    splitmix64 streams 10 and 11."""
    k = (key, batch, grid, ebn0)
    if k not in _inputs:
        _inputs[k] = FD.table_grid(t, batch, ebn0, *FD.GRIDS[grid])
    return _inputs[k]


def make(t, name, batch, kind):
    """The named input for the Table t (`name` names it), cached: "coarse",
    "negzero" (float_domain.negzero of coarse), "sub" and "big" (the fine grid
    times float_domain.SCALES)."""
    k = ("made", name, batch, kind)
    if k not in _inputs:
        if kind == "coarse":
            _inputs[k] = synthetic_input(t, name, batch)
        elif kind == "negzero":
            _inputs[k] = FD.negzero(synthetic_input(t, name, batch))
        else:
            _inputs[k] = FD.scaled(synthetic_input(t, name, batch, "fine"), FD.SCALES[kind])
    return _inputs[k]


# ---- oracle ----------------------------------------------------------------

_oracle = {}


def beta_for(algo, kind):
    """The offset scaled like the input on "sub" / "big" (float_domain.oracle_on's rule); the NMS factor as it is."""
    _, oalgo, beta = ALGOS[algo]
    assert oalgo == O.OMS or kind not in FD.SCALES
    return beta if oalgo == O.NMS else beta * FD.SCALES.get(kind, 1.0)


def oracle_x(t, key, x, algo, beta, iters, early=False):
    """(hard, soft, iters_used) of oracle.decode_f32 on x, read-only and cached under `key` (which names t and x)."""
    k = (key, algo, float(beta), iters, bool(early))
    if k not in _oracle:
        out = O.decode_f32(t, x, iters, ALGOS[algo][1], beta, early_term=early, threads=O.host_threads())
        for a in out:
            a.setflags(write=False)
        _oracle[k] = out
    return _oracle[k]


def oracle(t, name, batch, kind, algo, iters, early=False, plus_zero=False):
    """The oracle on make(t, name, batch, kind); plus_zero: on that input + 0.0
    (every zero +0.0), ldsep's reference for the sign of a zero."""
    x = make(t, name, batch, kind)
    if plus_zero:
        x = x + np.float32(0.0)
    return oracle_x(t, (name, batch, kind, plus_zero), x, algo, beta_for(algo, kind), iters, early)


# ---- kernel 7's packed launch shapes in float ------------------------------

# Kernel 7 takes a float decode only if the table plus the codewords of one wave at the table's own lanes per
# codeword -- 64 / lanes codewords of (N + E) floats -- fit 64 KiB (lds_f32 of ldpc_code_layer_info).  Of the nine
# rows of short_domain.PACKED that leaves two, both without the split: 816x408, 1024x518 and 1200x600, which give
# int8 its split and 8-lane shapes, would need 8 codewords of float state (159 .. 197 KiB).  So:
# * PACKED_F32_SHIPPED: the rows of short_domain.PACKED that fit, and 200x100 at 4099, which is (32, split);
# * no shipped table reaches (16, split), (8, split) or (8, no split) in float.  Synthetic tables do: check degree
#   7 (the padding lane of the split form, 6 in the later group) at Z = 8 (one lane per check at 8 lanes) and Z = 4
#   (two lanes per check at 8 lanes), N = 256 and 128.
# Rows are (table name, batch, lanes per codeword, two lanes per check); packed_table() resolves the name.
# test_float_short_cpu.py pins lds_f32 of every row and of the rows left out, and the shapes against
# short_domain.predicted_shape.
PACKED_F32_SHIPPED = [("648x324", 4096 + 3, 32, False), ("200x100", 8192 + 3, 16, False),
                      ("200x100", 4096 + 3, 32, True)]
PACKED_NO_F32 = [r for r in SD.PACKED if r[0] in ("816x408", "1024x518", "1200x600")]
PACKED_SYN_D = 7
PACKED_F32_SYNTHETIC = [(SD.synthetic_name(PACKED_SYN_D, 8), 4096 + 3, 32, True),
                        (SD.synthetic_name(PACKED_SYN_D, 8), 8192 + 3, 16, True),
                        (SD.synthetic_name(PACKED_SYN_D, 8), 16384 + 3, 8, False),
                        (SD.synthetic_name(PACKED_SYN_D, 4), 16384 + 3, 8, True)]
PACKED_F32 = PACKED_F32_SHIPPED + PACKED_F32_SYNTHETIC
PACKED_ITERS = 3
PACKED_ALGOS = ("MS", "NMS0.75")


def packed_table(name):
    """The Table of a PACKED_F32 row's name: a shipped code or short_domain.synthetic(PACKED_SYN_D, Z)."""
    if name.startswith("synthetic_"):
        return SD.synthetic(PACKED_SYN_D, int(name.rsplit("_z", 1)[1]))
    return load_table(name)


def packed_input(name, batch, ebn0=EBN0):
    """The fine grid (step 0.5, clip 16) at `ebn0`: float_domain.make's "fine" for a shipped code."""
    if name.startswith("synthetic_"):
        return synthetic_input(packed_table(name), name, batch, "fine", ebn0)
    return FD.make(name, batch, "fine") if ebn0 == FD.EBN0[name] else FD.grid_input(name, batch, ebn0, *FD.FINE)


def packed_oracle(name, batch, algo, iters=PACKED_ITERS, early=False, ebn0=EBN0):
    return oracle_x(packed_table(name), (name, batch, "fine", ebn0), packed_input(name, batch, ebn0), algo,
                    ALGOS[algo][2], iters, early)


# early termination in a split packed shape: (row of PACKED_F32, Eb/N0 of the fine grid, iterations), plain min-sum.
# At 2 dB, 8 iterations, the 4099 codewords stop after 1 .. 8 iterations: 84, 765, 744, 452, 254, 150, 106 of them
# after 1 .. 7, and 1544 run to the end (short_domain.et_conditions holds: test_float_short_cpu.py).
PACKED_ET = (("200x100", 4096 + 3, 32, True), 2.0, 8)


# ---- ldsep: early termination ----------------------------------------------

# (d, rows, Z) -> (grid, Eb/N0, algorithm of the condition, row made to stall or None): 7 codewords, EP_ET_ITERS
# iterations; chosen on the CPU with the oracle alone so that, under that algorithm, one of ldsep's workgroups
# (codewords 0 .. 3 or 4 .. 6) holds a codeword that stops early, one that stops later and one that never stops
# (test_float_short_cpu.test_ldsep_early_termination_inputs).
# d = 8: plain min-sum on the grid input as it is.
# d = 2: every check joins a variable of column block 0 with one variable of another block, so the graph is a
# forest of stars and plain min-sum leaves all of a star equal after two iterations: on any input it stops at 1 or
# 2 and a codeword that never stops does not exist.  Offset min-sum can stall, so the condition is taken under
# OMS 0.5 and row 3 is replaced by stall_row(): 0 in column block 0, +0.5 elsewhere.  Every message is then
# max(0.5 - 0.5, 0) = 0 or max(0 - 0.5, 0) = 0, V stays the input, and its hard decisions (0 in block 0, 1 beside
# it) satisfy no check, in any iteration.  Under MS and NMS that row stops after one iteration; rows 0 .. 2 stop
# at 1 and 2.
EP_ET_ITERS = 16
EP_ET = {(8, 12, 8): ("fine", 2.0, "MS", None), (8, 12, 27): ("fine", 2.0, "MS", None),
         (8, 12, 32): ("coarse", 2.0, "MS", None), (8, 11, 41): ("fine", 2.0, "MS", None),
         (2, 12, 8): ("coarse", 2.0, "OMS0.5", 3), (2, 12, 27): ("coarse", 2.0, "OMS0.5", 3),
         (2, 12, 32): ("coarse", 2.0, "OMS0.5", 3), (2, 11, 41): ("coarse", 2.0, "OMS0.5", 3)}


def stall_row(Z, n):
    x = np.full(n, 0.5, dtype=np.float32)
    x[:Z] = 0.0
    return x


def ep_et_input(d, rows, Z):
    t, name = ep_table(d, rows, Z)
    grid, ebn0, _, stall = EP_ET[(d, rows, Z)]
    k = ("ep_et", d, rows, Z)
    if k not in _inputs:
        x = np.array(synthetic_input(t, name, EP_BATCH, grid, ebn0))
        if stall is not None:
            x[stall] = stall_row(Z, t.n)
        x.setflags(write=False)
        _inputs[k] = x
    return _inputs[k]


def ep_et_oracle(d, rows, Z, algo, plus_zero=False):
    t, name = ep_table(d, rows, Z)
    x = ep_et_input(d, rows, Z)
    return oracle_x(t, (name, "et", plus_zero), x + np.float32(0.0) if plus_zero else x, algo, ALGOS[algo][2],
                    EP_ET_ITERS, early=True)


def ep_et_condition(its, iters=EP_ET_ITERS, group=4):
    """Does some group of `group` consecutive codewords hold two that stop at different iterations before the last
    and one that never stops?"""
    its = np.asarray(its)
    for s in range(0, len(its), group):
        g = its[s:s + group]
        if len(set(g[g < iters].tolist())) >= 2 and (g == iters).any():
            return True
    return False
