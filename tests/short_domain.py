"""Shared tables, inputs and helpers of the short-code domain tests
(test_short_domain_cpu.py, test_gpu_short_domain.py): the sixteen plain .ldpc
tables on the generic kernel (1), the LDS-resident kernel (7) and the host
decoder, over the full int8 LLR range and the parameter grid of
param_domain.py, in every launch shape of kernel 7 and at every check degree
the kernels are instantiated for.  A plain helper module, like
param_domain.py, whose inputs, grid and oracle helper it reuses.
"""
import numpy as np

import param_domain as PD
from ldpcgputegra_amd import channel, load_table
from ldpcgputegra_amd.codes import Table

# ---- the shipped short tables ---------------------------------------------

LDS_CODES = ["200x100", "576x288", "648x324", "816x408", "1024x518", "1200x600", "1248x624", "1944x972",
             "2048x384", "2304x1152", "4000x2000", "4896x2448"]          # a codeword's int8 state fits kernel 7's LDS
GENERIC_ONLY = ["8000x4000", "9972x4986", "16200x7560", "20000x10000"]   # it does not
SHORT_CODES = LDS_CODES + GENERIC_ONLY
# kernel families per code (what test_gpu_parity.kernels_for gives, pinned so that none drops out unnoticed)
KERNELS = {c: [1, 7] for c in LDS_CODES}
KERNELS.update({c: [1] for c in GENERIC_ONLY})
# (layers, checks in the widest layer) of kernel 7's layer plan (ldpc_code_layer_info)
LAYER_PLAN = {
    "200x100": (25, 9), "576x288": (11, 48), "648x324": (12, 27), "816x408": (107, 9), "1024x518": (319, 6),
    "1200x600": (547, 3), "1248x624": (11, 104), "1944x972": (12, 81), "2048x384": (13, 64), "2304x1152": (11, 192),
    "4000x2000": (123, 43), "4896x2448": (132, 55),
    "8000x4000": (166, 65), "9972x4986": (221, 93), "16200x7560": (6841, 244), "20000x10000": (281, 83),
}
# the kernel the automatic choice (0) takes for int8: lds where it fits and m >= 8 * layers (lds_preferred)
AUTO = {"200x100": "generic", "576x288": "lds", "648x324": "lds", "816x408": "generic", "1024x518": "generic",
        "1200x600": "generic", "1248x624": "lds", "1944x972": "lds", "2048x384": "lds", "2304x1152": "lds",
        "4000x2000": "lds", "4896x2448": "lds", "8000x4000": "generic", "9972x4986": "generic",
        "16200x7560": "generic", "20000x10000": "generic"}

# ---- the launch shapes of kernel 7 ----------------------------------------

# (code, batch, lanes per codeword, two lanes per check): more than one codeword per wave.  The batches are the
# smallest at which the kernel takes these shapes (it widens a codeword's lane group while the launch has fewer
# than 2048 waves); the + 3 leaves the last wave partly empty.
PACKED = [
    ("648x324", 4096 + 3, 32, False),
    ("1024x518", 4096 + 3, 32, True),
    ("816x408", 4096 + 3, 32, True),
    ("200x100", 8192 + 3, 16, False),
    ("816x408", 8192 + 3, 16, False),
    ("1024x518", 8192 + 3, 16, True),
    ("1200x600", 8192 + 3, 16, True),
    ("1024x518", 16384 + 3, 8, False),
    ("1200x600", 16384 + 3, 8, True),
]
MIN_WAVES = 2048      # lds.hip launch_lds: 2 * kLdsSimds


def predicted_shape(max_width, batch):
    """(lanes per codeword, split) of launch_lds, restated: a guard on the
    literals of PACKED only; the GPU tests read the shape the launch took from
    Decoder.last_lds_shape."""
    lg = 3 if max_width <= 8 else 4 if max_width <= 16 else 5 if max_width <= 32 else 6
    while lg < 6 and (batch << lg) // 64 < MIN_WAVES:
        lg += 1
    return 1 << lg, (1 << lg) >= 2 * max_width


def packed_id(row):
    return "%s_b%d_l%d%s" % (row[0], row[1], row[2], "s" if row[3] else "")


# ---- synthetic tables: every check degree ---------------------------------

DEGREES = list(range(2, 33))
Z_SPLIT, Z_LOOP = 12, 40      # 64 >= 2 Z: two lanes per check; 40: one lane per check, lanes 40 .. 63 idle
COL_BLOCKS, BLOCK_ROWS = 32, 6
_tables = {}


def synthetic(d, Z):
    """Table of a quasi-cyclic code with N = 32 Z and two groups of three
    block rows each, the first of check degree d, the second of degree
    max(2, d - 1).  Check i of block row r uses the variables
    Z cb_j + (i + s_j) mod Z of deg distinct column blocks cb_j: column block
    0 (every block row covers it whole, so consecutive block rows never merge
    into one layer) and the first deg - 1 of the others in the order of their
    splitmix64 values, keyed like the shifts s_j by (d, Z, r).  A block row
    is one layer of Z checks sharing no variable."""
    if (d, Z) not in _tables:
        groups = [(d, 3 * Z), (max(2, d - 1), 3 * Z)]
        edges = []
        for r in range(BLOCK_ROWS):
            deg = groups[r // 3][0]
            key = np.uint64((d << 40) | (Z << 20) | (r << 8))
            draw = PD.splitmix64(key + np.arange(2 * COL_BLOCKS, dtype=np.uint64))
            first = 0
            others = [int(c) for c in np.argsort(draw[:COL_BLOCKS], kind="stable") if int(c) != first]
            cb = np.array([first] + others[:deg - 1], dtype=np.int64)
            s = (draw[COL_BLOCKS:COL_BLOCKS + deg] % np.uint64(Z)).astype(np.int64)
            i = np.arange(Z, dtype=np.int64)[:, None]
            edges.append((Z * cb[None, :] + (i + s[None, :]) % Z).ravel())
        _tables[(d, Z)] = Table(COL_BLOCKS * Z, BLOCK_ROWS * Z, groups, np.concatenate(edges).astype(np.uint32))
    return _tables[(d, Z)]


def synthetic_name(d, Z):
    return "synthetic_d%d_z%d" % (d, Z)


# the parameter sets of the synthetic sweeps: the default, the full message range, var_min -128, NMS at its bounds
SWEEP_PARAMS = [PD.CONTROL, PD.Params("OMS", 3, -127, 127), PD.Params("OMS", 1, -128, 31),
                PD.Params("NMS", 255, -127, 127)]
# `sat_flip` beside the two inputs of the packed tests: at the high degrees the two smallest of a check's |c| are
# seldom below -msg_max on uniform or tied inputs, so the later-group rule would go unseen there; with 96 % of the
# LLRs at -127 a quarter of the degree-32 checks hold nothing else
SWEEP_INPUTS = ("u128", "ties", "sat_flip")


def oracle_synthetic(d, Z, kind, batch, params, iters):
    t = synthetic(d, Z)
    return PD.oracle_decode(synthetic_name(d, Z), (kind, batch), PD.make_input(kind, batch, t.n), params, iters,
                            table=t)


# ---- early termination: saturated AWGN inputs that converge ----------------

# As param_domain.et_input: AWGN LLRs of channel.i8_table (|LLR| <= 31) at Eb/N0, times a scale, clipped to +-127.
# (Eb/N0 in dB under ET_PARAMS[0] and under ET_PARAMS[1], scale) per code, chosen on the CPU with the oracle alone
# at the batches of PACKED, 8 iterations, so that >= 10 % of the bytes are +-127 (22 .. 29 % here), under either
# parameter set some codewords stop early and some never do, and under the recipe's own parameter set some wave of
# kernel 7's packed shape holds codewords that stop at different iterations, some wave stops entirely early and
# some wave never stops (test_short_domain_cpu.py asserts all of that).  OMS 4 / msg_max 63 converges less often
# than the default (offset 4 of a variable range of 127 / 12 channel units), mostly at iteration 1 or never; with
# eight codewords per wave (1200x600 @ 16387) "a whole wave stops" and "a whole wave never stops" both need about
# half of the codewords to stop, which one Eb/N0 does not give under both parameter sets, hence the two values.
# Codewords that stop (at iterations), of the batch, under the default / under OMS 4 / msg_max 63:
#   200x100  @ 8195   3.5 dB   5297 (1-7) / 4857 (1-7)      648x324  @ 4099   5.0 dB   2673 (1-5) / 1243 (1-2)
#   816x408  @ 4099   3.5 dB   3309 (1-7) /  716 (1-7)      1024x518 @ 4099   5.0 dB   1944 (1-5) /  548 (1)
#   1200x600 @ 16387  5.0 dB   7871 (1-6); 6.0 dB under OMS 4 / msg_max 63: 9254 (1)
ET_SEED = 43
ET_ITERS = 8
ET_PARAMS = [PD.CONTROL, PD.Params("OMS", 4, -127, 63)]
ET_RECIPE = {"200x100": ((3.5, 3.5), 12), "648x324": ((5.0, 5.0), 12), "816x408": ((3.5, 3.5), 12),
             "1024x518": ((5.0, 5.0), 12), "1200x600": ((5.0, 6.0), 12)}
# the packed rows whose early termination runs on the GPU (int8), and the float ones (float_domain "fine" inputs)
ET_ROWS = [r for r in PACKED if (r[0], r[1]) in (("648x324", 4099), ("1024x518", 4099), ("200x100", 8195),
                                                 ("1200x600", 16387))]
ET_ROWS_F32 = [r for r in PACKED if (r[0], r[1]) in (("648x324", 4099), ("200x100", 8195))]
ET_ITERS_F32 = 8


def et_input(code, batch, params=PD.CONTROL):
    """int8 [batch, N], read-only and cached: the saturated AWGN input of
    ET_RECIPE for `params` (one of ET_PARAMS)."""
    ebn0s, scale = ET_RECIPE[code]
    ebn0 = ebn0s[ET_PARAMS.index(params)]
    key = ("short_et", code, batch, ebn0)
    if key not in PD._inputs:
        t = load_table(code)
        sigma = channel.sigma_from_ebn0(ebn0, t.k_info / t.n)
        raw = channel.awgn_i8_host(t.n, batch, seed=ET_SEED, table=channel.i8_table(sigma))
        x = np.clip(raw.astype(np.int32) * scale, -127, 127).astype(np.int8)
        x.setflags(write=False)
        PD._inputs[key] = x
    return PD._inputs[key]


def wave_groups(iters_used, lanes):
    """iters_used of the codewords of each full wave of kernel 7 at `lanes`
    lanes per codeword: [waves, 64 // lanes] (the ragged last wave left out)."""
    cpw = 64 // lanes
    full = len(iters_used) // cpw * cpw
    return np.asarray(iters_used[:full]).reshape(-1, cpw)


def et_conditions(iters_used, lanes, iters):
    """The conditions an early-termination input must meet for a packed shape,
    as a dict of booleans: some codewords stop early and some do not; a wave
    holds two different iters_used; a wave stops entirely before the last
    iteration; a wave never stops."""
    g = wave_groups(iters_used, lanes)
    return dict(some_stop=bool((iters_used < iters).any()), some_run_on=bool((iters_used == iters).any()),
                mixed_wave=bool((g.min(axis=1) != g.max(axis=1)).any()),
                wave_stops=bool((g.max(axis=1) < iters).any()),
                wave_never_stops=bool((g.min(axis=1) == iters).any()))
