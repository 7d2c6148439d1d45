"""Shared inputs, parameter grid and oracle helper of the parameter-domain
tests (test_param_domain_cpu.py, test_gpu_param_domain.py): full-range int8
LLRs and the decoder parameters the C-ABI accepts, inside and outside the
domain of the fast DVB-S2 kernels.  A plain helper module, like
windowed_model.py.

Inputs come from a numpy restatement of splitmix64 (the generator
golden/gen_golden.py restates), so nothing depends on a numpy RNG stream.
"""
from collections import namedtuple
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import oracle as O
from ldpcgputegra_amd import ALGO_MS, ALGO_NMS, ALGO_OMS, channel, default_params, load_table

M64 = np.uint64(0xFFFFFFFFFFFFFFFF)


def splitmix64(x):
    with np.errstate(over="ignore"):
        x = (x + np.uint64(0x9E3779B97F4A7C15)) & M64
        x = ((x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)) & M64
        x = ((x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)) & M64
        return x ^ (x >> np.uint64(31))


# ---- inputs ---------------------------------------------------------------

INPUTS = ("u128", "ext", "sat_flip", "ties")
EXT_VALUES = np.array([-128, -127, -1, 0, 1, 127], dtype=np.int8)
FLIP_RATE = 0.04
_inputs = {}


def _draw32(batch, n, stream):
    """[batch, n] uint64 values uniform over 0 .. 2^32 - 1: the high half of
    splitmix64(index ^ key), one key per stream."""
    idx = np.arange(batch * n, dtype=np.uint64).reshape(batch, n)
    key = np.uint64(((stream + 1) * 0xD1B54A32D192ED03) & 0xFFFFFFFFFFFFFFFF)
    return splitmix64(idx ^ key) >> np.uint64(32)


def make_input(kind, batch, n):
    """int8 [batch, n], read-only and cached:
    u128      uniform over -128 .. 127;
    ext       uniform over {-128, -127, -1, 0, 1, 127};
    sat_flip  all -127 with about 4 % of the positions +127: a saturated noisy
              all-zero codeword (hard decision = LLR > 0), which converges;
    ties      every value +-127 with a random sign: every |c| ties, on the
              two-lanes-per-check degrees with the sink entries too."""
    key = (kind, batch, n)
    if key not in _inputs:
        r = _draw32(batch, n, INPUTS.index(kind))
        if kind == "u128":
            x = (r >> np.uint64(24)).astype(np.uint8).view(np.int8)
        elif kind == "ext":
            x = EXT_VALUES[((r * np.uint64(6)) >> np.uint64(32)).astype(np.int64)]
        elif kind == "sat_flip":
            x = np.where(r < np.uint64(int(FLIP_RATE * 2 ** 32)), 127, -127).astype(np.int8)
        elif kind == "ties":
            x = np.where((r >> np.uint64(31)) != 0, 127, -127).astype(np.int8)
        else:
            raise KeyError(kind)
        x = np.ascontiguousarray(x)
        x.setflags(write=False)
        _inputs[key] = x
    return _inputs[key]


# A saturated input that converges, for early termination: AWGN LLRs of channel.i8_table (|LLR| <= 31) at the
# code's early-termination Eb/N0 (test_gpu_coop3_r23.EBN0[code][0]; r1/2: test_gpu_parity.ET_EBN0) plus a margin in
# dB, times a scale, clipped to +-127.  (margin, scale) chosen on the CPU with the oracle, 32 codewords, 16
# iterations, so that under each of OMS 4 / msg_max 63, MS / 63 and NMS 64 / 63 some codewords stop early, not all
# at the same iteration, and >= 10 % of the bytes are +-127.  Scale 8 saturates 1 .. 12 % (too few once the margin
# lets anything converge), scale 16 half of the bytes; with scale 12:
#   code      margin  +-127   codewords of 32 that stop (at iteration): OMS 4/63, MS /63, NMS 64/63
#   r1/2       7.0    17.3 %  15 (1)      20 (1)       1 (1)
#   r2/3       6.0    14.1 %  29 (1)      30 (1)      22 (1)
#   r3/4       5.0    14.2 %  28 (1, 9)   31 (1)      19 (1)
#   r5/6       3.3    14.8 %  24 (1, 9)   26 (1)       2 (1)
#   r8/9       3.0    12.3 %  32 (1, 2)   31 (1)      22 (1)
#   r9/10      3.0    11.9 %  32 (1, 2)   32 (1, 12)  24 (1)
# the others run all 16 iterations.  The margins are large and the spread is mostly "at once or never" because the
# variable range is only 127 / 12 channel units: a saturated wrong bit of a degree-2 parity node cannot be turned
# by two messages of 63, and NMS factor 64 doubles every message.  Lower margins stop nothing; scales 9 .. 11
# saturate less than 10 % wherever anything stops.
ET_SEED = 41
ET_RECIPE = {"dvbs2_r1_2": (7.0, 12), "dvbs2_r2_3": (6.0, 12), "dvbs2shape_r3_4": (5.0, 12),
             "dvbs2shape_r5_6": (3.3, 12), "dvbs2_r8_9": (3.0, 12), "dvbs2_r9_10": (3.0, 12)}


# The batch-edge recipe (test_buffer_domain_cpu.py, test_gpu_buffer_domain.py): 65 codewords, 16 iterations, the
# default parameters (OMS 1, msg_max 31).  Wanted: stopped and still-running codewords among the first 17 (one
# coop / coop3 group and a ragged one), and codeword 64 -- alone in its group at batch 65 -- stopping early for one
# code and not for the other.  r1/2's ET_RECIPE input gives that already (iterations used by codewords 0 .. 16: 1, 2
# and, for two of them, 16; codeword 64 stops after 1).  r8/9's stops every codeword at iteration 1 or 2, so its
# margin goes down to 1.0 dB, where 8 of the 65 never stop, and the seed is the first of 41 .. 89 whose codeword 64
# is one of those (65: codewords 0 .. 16 use 2 .. 4 iterations, codeword 2 all 16; 17.9 % of the bytes +-127).
ET_EDGE = {"dvbs2_r1_2": (ET_SEED, 7.0, 12), "dvbs2_r8_9": (65, 1.0, 12)}


def et_input(code, batch, recipe=None):
    """int8 [batch, N], read-only and cached: the saturated AWGN input of
    ET_RECIPE, or of `recipe` = (seed, margin, scale), e.g. ET_EDGE[code]."""
    key = ("et", code, batch) if recipe is None else ("et", code, batch, tuple(recipe))
    if key not in _inputs:
        from test_gpu_coop3_r23 import EBN0
        from test_gpu_parity import ET_EBN0
        t = load_table(code)
        seed, margin, scale = recipe if recipe is not None else (ET_SEED,) + tuple(ET_RECIPE[code])
        base = EBN0[code][0] if code in EBN0 else ET_EBN0[code]
        sigma = channel.sigma_from_ebn0(base + margin, t.k_info / t.n)
        raw = channel.awgn_i8_host(t.n, batch, seed=seed, table=channel.i8_table(sigma))
        x = np.clip(raw.astype(np.int32) * scale, -127, 127).astype(np.int8)
        x.setflags(write=False)
        _inputs[key] = x
    return _inputs[key]


# ---- parameter grid -------------------------------------------------------

class Params(namedtuple("Params", "algo param var_min msg_max")):
    """algo "OMS" / "MS" / "NMS"; param the OMS offset or the NMS factor."""

    @property
    def id(self):
        return "%s%s_vmin%d_mmax%d" % (self.algo, "" if self.algo == "MS" else self.param, self.var_min,
                                       self.msg_max)

    def product(self, **kw):
        """ldpc_params.  Plain MS leaves the offset field at its default, 1:
        LDPC_ALGO_MS is OMS with offset 0 whatever that field holds."""
        a = {"OMS": ALGO_OMS, "MS": ALGO_MS, "NMS": ALGO_NMS}[self.algo]
        f = {"OMS": {"offset": self.param}, "NMS": {"factor": self.param}, "MS": {}}[self.algo]
        return default_params(algo=a, var_min=self.var_min, msg_max=self.msg_max, msg_min=-self.msg_max, **f, **kw)

    @property
    def oracle(self):
        """(algo, param) of oracle.decode_i8 / oracle.ref_decode."""
        return (O.NMS, self.param) if self.algo == "NMS" else (O.OMS, 0 if self.algo == "MS" else self.param)


def _p(algo, param, msg_max, var_min=-127):
    return Params(algo, param, var_min, msg_max)


CONTROL = _p("OMS", 1, 31)
# inside the domain of coop3 (and, for OMS / MS, of coop and windowed2)
IN_DOMAIN = [
    _p("OMS", 0, 63), _p("OMS", 63, 63), _p("OMS", 31, 31), _p("OMS", 32, 31), _p("OMS", 5, 0), _p("OMS", 0, 1),
    CONTROL,
    _p("MS", 0, 31), _p("MS", 0, 63),
    _p("NMS", 0, 63), _p("NMS", 1, 63), _p("NMS", 32, 63), _p("NMS", 33, 63), _p("NMS", 64, 63), _p("NMS", 64, 31),
]
# outside it: the automatic choice falls back
OUT_OF_DOMAIN = [
    _p("OMS", 3, 127), _p("OMS", 1, 31, var_min=-128), _p("OMS", 64, 63), _p("OMS", 1, 31, var_min=-64),
    _p("NMS", 65, 63), _p("NMS", 255, 127),
]
GRID = IN_DOMAIN + OUT_OF_DOMAIN
# a subset for the slower host paths: the corners of the fast domain, NMS at
# its bound and one entry of each way out of it
SUBSET = [_p("OMS", 63, 63), _p("OMS", 5, 0), _p("MS", 0, 31), _p("NMS", 64, 63), _p("OMS", 3, 127),
          _p("OMS", 1, 31, var_min=-128), _p("NMS", 255, 127)]


# ---- oracle ---------------------------------------------------------------

_oracle = {}
_pool = None


def oracle_decode(code, key, llr, params, iters, early=False, table=None):
    """(hard, soft, iters_used) of oracle.decode_i8 on llr (int8 [B, N]),
    read-only and cached per (code, input, params, iters, early); `key` names
    the input.  `table`: the Table of a code that is no shipped one (`code`
    then only names it in the cache).  The batch is split into slices of at
    most 16 codewords (fewer where that keeps every thread busy) over
    oracle.host_threads() Python threads (the ctypes call releases the GIL):
    oracle_decode_i8_mt_ex runs for the default ranges only."""
    global _pool
    t = table if table is not None else load_table(code)
    ck = (code, key, params, iters, bool(early))
    if ck not in _oracle:
        if _pool is None:
            _pool = ThreadPoolExecutor(max_workers=O.host_threads())
        algo, param = params.oracle
        B = llr.shape[0]
        step = max(1, min(16, -(-B // O.host_threads())))

        def part(lo):
            return O.decode_i8(t, llr[lo:lo + step], iters, algo, param, var_min=params.var_min,
                               msg_max=params.msg_max, early_term=early, return_soft=True)

        parts = list(_pool.map(part, range(0, B, step)))
        out = tuple(np.concatenate([p[i] for p in parts]) for i in range(3))
        for a in out:
            a.setflags(write=False)
        _oracle[ck] = out
    return _oracle[ck]


def oracle_on(code, kind, batch, params, iters, early=False):
    """oracle_decode on the named make_input input."""
    return oracle_decode(code, (kind, batch), make_input(kind, batch, load_table(code).n), params, iters, early)


def ref_decode(code, llr, params, iters):
    """Hard decisions of the reference's own SSE decoder (oracle/_ref); the
    batch must be a multiple of 16."""
    algo, param = params.oracle
    return O.ref_decode(code, llr, iters, algo, param, vmin=params.var_min, vmax=127, mmin=-params.msg_max,
                        mmax=params.msg_max)
