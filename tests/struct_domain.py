"""Shared tables and helpers of the schedule-domain tests
(test_struct_domain_cpu.py, test_gpu_struct_domain.py): small synthetic
staircase tables whose static schedules are unlike any shipped DVB-S2 table's,
for the five staircase families -- windowed (2), windowed2 (3), coop (5),
coop3 (8), stairf (11) -- beside generic (1) and the automatic choice.  A plain
helper module, like param_domain.py and short_domain.py, whose inputs, Params
and oracle helper it reuses.

Every table is deterministic (keyed by splitmix64) and cached.  Three kinds:

* SWEEP, Annex-B style tables: M = 360 q checks, K = 360 rows, row g holding
  for each residue s < q the addresses q t + s of c[g] values t; every check
  then has X = sum(c) information edges.  Row 0's two t per residue are delta
  apart, so two checks q delta apart share one information variable; every
  other pair of touches of a variable is farther apart, so the table's
  min_hazard is q delta by construction (checked in numpy when the table is
  built, and against ldpc_code_plan_info on the CPU).  q delta sits just
  below, at and just above each schedule constant of each family;
* MIXED, the same with rows of unequal length and mixed variable degrees (the
  shapes of test_gpu_encoder.SMALL's q2 and q7, padded to X edges per check):
  a row of three addresses gives variables touched three times an iteration,
  delta and delta + 1 checks apart;
* HAND, staircase and near-staircase tables that no Annex-B table gives, through
  ldpc_code_create.

PINS records, per table, which family accepts it and what the host can see of
its schedules, written from the planners' own answers at the commit that added
this file: a family that drops out, or a schedule that changes shape, turns a
test red.
"""
from collections import namedtuple

import numpy as np

import oracle as O
import param_domain as PD
from ldpcgputegra_amd.codes import Table

# ---- the schedule constants the delta sweep brackets -----------------------
# each next to the literal it restates

WIN_S = 16                  # plan.cpp kPlanSlots; capi.hip windowed2_upload(h, 16, 2, ..)
WIN_LOOKAHEAD = 2           # plan.cpp kLookahead (windowed)
WIN2_P = 2                  # capi.hip windowed2_upload(h, 16, 2, ..)
COOP_S = 28                 # coop.hip 4 * kWS, kWS = 7
LC_GAP = 10                 # coop.h LC_GAP; linecache.cpp refuses nw < 4 * LC_GAP
COOP3_R = 2 + 2             # coop3.hip coop3_plan_host: coop_build_plan(h, S, r + 2, ..), r = 2
COOP3_WAVE0 = 8             # coop3.hip coop3_plan_host: at most 8 distance-2 checks per window (slab wave 0)
DEGREES = (7, 10, 14, 22, 27, 30)      # first-group degrees D0 = X + 2: windowed2_upload, g3_degree_ok, x_supported
XS = tuple(d - 2 for d in DEGREES)
WINDOWED_D0 = (7, 10)       # windowed.hip degree_ok
COOP_D0 = (7, 10, 14, 22)   # coop.hip coop_upload
STAIRF_S = (2, 4, 8, 16)    # stairf.hip stairf_upload: one table per group width
FAMILIES_I8 = (2, 3, 5, 8)  # the fast int8 families (Decoder.set_kernel numbers); 1 takes every table
STAIRF = 11


def coop_r(d0):
    """coop.hip coop_r: prefetch depth, windows."""
    return 2 if d0 > 16 else 3


def _g3_ws(d0):
    return 6 if d0 == 7 else 4 if (d0 <= 14 or d0 >= 22) else 2      # coop3_kernel.h G3::WS (HALF: D0 >= 22)


def g3_s(d0):
    """coop3_kernel.h G3::S = SPW * WS."""
    return (4 if d0 >= 22 else 8) * _g3_ws(d0)


def g3_dist(d0):
    """coop3_kernel.h G3::DIST."""
    return 2 if (_g3_ws(d0) == 2 or d0 >= 22) else 1


def p_of_s(X, S):
    """stairf.hip SF<X, S>::P: groups in flight."""
    pr = 8 if X <= 5 else 6 if X <= 8 else 4 if X <= 12 else 2
    return min(pr, 48 // S)


def stairf_widths(t, hazard):
    """The group widths stairf_upload builds a table for, restated (for a
    staircase table whose information variables are no parity variables,
    which every accepted table here is): two groups, the second one check of
    degree D0 - 1, X supported, M % 4 == 0, M >= 32, N <= 65536; then every
    S with M % S == 0 and min_hazard >= S * P."""
    if len(t.groups) != 2 or t.groups[1] != (t.groups[0][0] - 1, 1):
        return ()
    X = t.groups[0][0] - 2
    if X not in XS or t.m % 4 or t.m < 32 or t.n > 65536:
        return ()
    return tuple(S for S in STAIRF_S if t.m % S == 0 and hazard >= S * p_of_s(X, S))


def stairf_width_taken(widths, want):
    """stairf.hip stairf_width with LDPC_STAIRF_S = want."""
    for S in (want, 8, 4, 16, 2):
        if S in widths:
            return S
    return 0


def constants(X):
    """{name: sharing distance} of the schedule constants of first-group degree
    X + 2: the distances q delta the sweep puts a table just below, at and
    just above.  Windowed: a window, its lookahead of 2 windows, and the
    first distance past it; windowed2: P = 2 gives the same three.  coop: a
    window, two windows (where forwarding starts), R + 1 windows (where it
    ends).  coop3: a window, dist + 1 windows, three windows (dist 1: where
    the distance-2 pairs of slab wave 0 end), R + dist windows, and the limit
    of 8 distance-2 checks.  stairf: S * P per group width."""
    d0 = X + 2
    s3, d3 = g3_s(d0), g3_dist(d0)
    out = {"win": WIN_S, "win_look": WIN_S * WIN_LOOKAHEAD, "win_look1": WIN_S * (WIN_LOOKAHEAD + 1),
           "win2_p1": WIN_S * (WIN2_P + 1),
           "coop": COOP_S, "coop_2": 2 * COOP_S, "coop_fwd": COOP_S * (coop_r(d0) + 1),
           "coop3": s3, "coop3_dist": s3 * (d3 + 1), "coop3_3": s3 * 3, "coop3_fwd": s3 * (COOP3_R + d3),
           "coop3_wave0": COOP3_WAVE0}
    out.update({"stairf_%d" % S: S * p_of_s(X, S) for S in STAIRF_S})
    return out


# ---- Annex-B style tables --------------------------------------------------

Spec = namedtuple("Spec", "name q c delta")
_tables = {}


def _key(*parts):
    k = np.uint64(0x5EED)
    for p in parts:
        k = PD.splitmix64(k ^ np.uint64(p))
    return k


def annexb_rows(q, c, delta, salt=0):
    """Address rows of the table, as t values per residue: row g, residue s
    starts at (b_g + s * (360 // q) + j) % 360 -- the residues of one row about
    360 checks apart, b_g and j < 4 keyed, a different t per residue.  A row
    of c[g] > 1 addresses per residue continues delta, delta + 1, .. further
    for the first such row (so q delta is the table's least sharing distance)
    and delta + 1, delta + 2, .. further for the later ones."""
    rows, first = [], True
    for g, cg in enumerate(c):
        draw = PD.splitmix64(_key(q, len(c), delta, g, salt) + np.arange(1 + q, dtype=np.uint64))
        base = int(draw[0] % np.uint64(360))
        step = delta if first else delta + 1
        row = []
        for s in range(q):
            t0 = base + s * (360 // q) + int(draw[1 + s] % np.uint64(4))
            row.append([(t0 + i * step + i * (i - 1) // 2) % 360 for i in range(cg)])
        first = first and cg == 1
        rows.append(row)
    return rows


def table_from_rows(q, rows):
    """The layered H of an Annex-B address table (codes._dvbs2_from_text's
    rule, restated for rows given as t values per residue)."""
    k, m = 360 * len(rows), 360 * q
    info = [[] for _ in range(m)]
    for g, row in enumerate(rows):
        for s, ts in enumerate(row):
            for t in ts:
                for kk in range(360):
                    info[(q * t + s + kk * q) % m].append(360 * g + kk)
    edges, groups = [], []
    for idx in range(m):
        r = (idx + 1) % m
        lst = sorted(info[r]) + ([k + r - 1, k + r] if r > 0 else [k])
        edges.extend(lst)
        if groups and groups[-1][0] == len(lst):
            groups[-1][1] += 1
        else:
            groups.append([len(lst), 1])
    return Table(k + m, m, groups, np.array(edges, dtype=np.uint32))


def rows_text(q, rows):
    """The table as an Annex-B .txt (ldpc_code_load, the IRA encoder)."""
    lines = ["# N=%d K=%d" % (360 * (len(rows) + q), 360 * len(rows))]
    for row in rows:
        lines.append(" ".join(str(q * t + s) for s, ts in enumerate(row) for t in ts))
    return "\n".join(lines) + "\n"


def check_lists(t):
    return [v.tolist() for _, v in t.checks()]


def min_hazard(t):
    """plan.cpp's min_hazard in numpy: the least cyclic schedule distance
    between two touches of one variable, a staircase check's chain input
    (its entry deg - 2, shared with the previous check's last entry) left out;
    M when no variable is touched twice."""
    best = t.m
    last = {}
    chk = check_lists(t)
    for pas in range(2):
        for i, vs in enumerate(chk):
            prev = chk[i - 1]
            for j, v in enumerate(vs):
                if pas and v in last and last[v] != i:
                    if not (j == len(vs) - 2 and prev[-1] == v):
                        best = min(best, (i - last[v]) % t.m or t.m)
                last[v] = i
    return best


def annexb(spec):
    """(Table, rows) of an Annex-B Spec, cached: the first keyed draw whose
    min_hazard is q delta (the first one, for every Spec of this file)."""
    if spec.name not in _tables:
        for salt in range(16):
            rows = annexb_rows(spec.q, spec.c, spec.delta, salt)
            t = table_from_rows(spec.q, rows)
            if min_hazard(t) == spec.q * spec.delta:
                break
        else:
            raise AssertionError("no draw of %s has min_hazard %d" % (spec.name, spec.q * spec.delta))
        _tables[spec.name] = (t, rows)
    return _tables[spec.name]


# ---- the delta sweep -------------------------------------------------------

H_MAX = 170       # q delta beyond this: with q > 1 row 0's residues, 360 checks apart, come closer than q delta
# one q with M % 16 == 8 and one with M % 16 == 0 per degree, N <= 12000, M / g3_s(D0) >= 4 LC_GAP windows
LARGE_Q = {5: (7, 6), 8: (5, 4), 12: (5, 4), 20: (3, 4), 25: (3, 6), 28: (5, 6)}


def _c_of(X):
    return (2,) + (1,) * (X - 2)


def sweep_specs():
    """Per X: at q = 1 every distance just below, at and just above each
    constant of constants(X) (and 2, 3: the densest sharing); at the two
    larger q the multiples of q next to each constant (and q itself)."""
    out = []
    for X in XS:
        cs = sorted(set(constants(X).values()))
        for h in sorted({h + d for h in cs for d in (-1, 0, 1)} | {2, 3}):
            if 2 <= h <= H_MAX:
                out.append(Spec("x%d_q1_h%d" % (X, h), 1, _c_of(X), h))
        for q in LARGE_Q[X]:
            for d in sorted({d for h in cs for d in (h // q, -(-h // q)) if d >= 1 and q * d <= H_MAX} | {1}):
                out.append(Spec("x%d_q%d_h%d" % (X, q, q * d), q, _c_of(X), d))
    return out


SWEEP = sweep_specs()

# rows of unequal length, mixed variable degrees: q2's (1, 2, 1) and q7's (3, 1), padded with rows of one address
# to X edges per check, and one table with two rows of several addresses


def _mixed(X, q, head, delta):
    c = tuple(head) + (1,) * (X - sum(head))
    return Spec("m_x%d_q%d_h%d" % (X, q, q * delta), q, c, delta)


MIXED = [_mixed(5, 2, (1, 2, 1), 3), _mixed(5, 2, (1, 2, 1), 30), _mixed(5, 7, (3, 1), 2), _mixed(5, 7, (3, 1), 8),
         _mixed(8, 2, (1, 2, 1), 20), _mixed(8, 7, (3, 1), 1), _mixed(8, 3, (2, 3), 4), _mixed(12, 7, (3, 1), 5),
         _mixed(20, 2, (1, 2, 1), 2), _mixed(25, 7, (3, 1), 3), _mixed(28, 2, (1, 2, 1), 10)]
ANNEXB = {s.name: s for s in SWEEP + MIXED}
assert len(ANNEXB) == len(SWEEP) + len(MIXED)


# ---- hand-built tables -----------------------------------------------------

def _rebuild(t, chk):
    groups = []
    for vs in chk:
        if groups and groups[-1][0] == len(vs):
            groups[-1][1] += 1
        else:
            groups.append([len(vs), 1])
    return Table(t.n, t.m, groups, np.array([v for vs in chk for v in vs], dtype=np.uint32))


def permuted(t, key):
    """(a) the information edges of each check in a keyed random order instead
    of ascending; the parity edges keep their places."""
    chk = check_lists(t)
    X = t.groups[0][0] - 2
    for i, vs in enumerate(chk):
        order = np.argsort(PD.splitmix64(_key(key, i) + np.arange(X, dtype=np.uint64)), kind="stable")
        chk[i] = [vs[j] for j in order] + vs[X:]
    return _rebuild(t, chk)


def shortened(t, c, drop=1):
    """(b) the last c staircase checks (before the tail) each lose their
    first `drop` information edges -- variables of row 0, which keep their
    other edge.  drop = 1: a second degree group of c + 1 checks of degree
    D0 - 1; drop = 2: three groups."""
    chk = check_lists(t)
    for i in range(t.m - 1 - c, t.m - 1):
        assert all(v < 360 for v in chk[i][:drop])
        chk[i] = chk[i][drop:]
    return _rebuild(t, chk)


def double_share(t, i=11):
    """(c) check i's first information variable replaced by check i - 1's: two
    consecutive checks share an information variable besides the chain link."""
    chk = check_lists(t)
    assert chk[i - 1][0] not in chk[i]
    chk[i] = sorted([chk[i - 1][0]] + chk[i][1:-2]) + chk[i][-2:]
    return _rebuild(t, chk)


def short_staircase(X, m):
    """A staircase of m checks (no multiple of 360): variable j < m in checks
    j and j + m / 2, X - 2 variables of degree 1 per check, the parity chain
    as in an Annex-B table.  min_hazard m / 2; few windows: nw on both sides
    of coop's R + 4."""
    k = m * (X - 1)
    chk = []
    for i in range(m):
        info = sorted([i, (i - m // 2) % m]) + [m + i * (X - 2) + j for j in range(X - 2)]
        chk.append(info + ([k + i, k + i + 1] if i < m - 1 else [k]))
    groups = [(X + 2, m - 1), (X + 1, 1)]
    return Table(k + m, m, groups, np.array([v for vs in chk for v in vs], dtype=np.uint32))


def _base(name):
    return annexb(ANNEXB[name])[0]


HAND = {
    # (a)
    "perm_x5_q1_h57": lambda: permuted(_base("x5_q1_h57"), 1), "perm_x5_q1_h3": lambda: permuted(_base("x5_q1_h3"), 2),
    "perm_x8_q5_h110": lambda: permuted(_base("x8_q5_h110"), 3), "perm_x20_q4_h48": lambda: permuted(_base("x20_q4_h48"), 4),
    # (c)
    "deg8_q1_h57": lambda: annexb(Spec("deg8_q1_h57", 1, _c_of(6), 57))[0],
    "three_groups_x5": lambda: shortened(_base("x5_q1_h57"), 3, drop=2),
    "double_share_x5": lambda: double_share(_base("x5_q1_h57")),
    # few windows: coop's nw = 6, 7 (R + 4 = 7) at degree 7 and 5, 6 (R + 4 = 6) at degree 22
    "short_x5_m140": lambda: short_staircase(5, 140), "short_x5_m168": lambda: short_staircase(5, 168),
    "short_x20_m112": lambda: short_staircase(20, 112), "short_x20_m140": lambda: short_staircase(20, 140),
}
# (b) D0 = 7 and 10, c = 1, 15, 16, 17
SECOND_GROUP = [(X, c) for X in (5, 8) for c in (1, 15, 16, 17)]
for _X, _c in SECOND_GROUP:
    HAND["second_x%d_c%d" % (_X, _c)] = (lambda X=_X, c=_c: shortened(_base("x%d_q1_h57" % X), c))
REFUSED_BY_ALL = ("deg8_q1_h57", "three_groups_x5", "double_share_x5")

NAMES = [s.name for s in SWEEP + MIXED] + list(HAND)


def table(name):
    """The named Table, cached."""
    if name in ANNEXB:
        return annexb(ANNEXB[name])[0]
    if name not in _tables:
        _tables[name] = (HAND[name](), None)
    return _tables[name][0]


# ---- what the host sees of a table's schedules ------------------------------

View = namedtuple("View", "families staircase hazard windowed windowed2 coop coop3")


def windowed2_accepts(t, plan):
    """windowed2_upload's predicate, restated: a window plan, two groups of
    degrees D0 and D0 - 1, D0 one of DEGREES."""
    return bool(plan) and len(t.groups) == 2 and t.groups[0][0] in DEGREES and t.groups[1][0] == t.groups[0][0] - 1


def host_view(t):
    """View of a table through the C library on the host: the families whose
    schedule builders accept it (a string of the digits of FAMILIES_I8),
    staircase, min_hazard, windows of the windowed plan (0: none), of the
    windowed2 plan, (windows, empty windows, forwarded reads) of coop's plan
    and (line-cache slots, windows, empty windows, forwarded reads) of coop3's
    (None: no plan)."""
    from ldpcgputegra_amd import Code
    code = Code(t)
    pi = code.plan_info()
    d0 = t.groups[0][0]
    w2 = code.window_plan(WIN_S, WIN2_P)
    coop = coop3 = None
    if d0 in COOP_D0:
        p = code.coop_plan(COOP_S, coop_r(d0), 1)
        if p is not None:
            coop = (len(p["windows"]), sum(1 for _, n in p["windows"] if n == 0), p["n_fwd"])
    lc = code.coop3_line_cache()
    if lc is not None:
        p = code.coop_plan(g3_s(d0), COOP3_R, g3_dist(d0))
        coop3 = (lc["slots"], len(p["windows"]), sum(1 for _, n in p["windows"] if n == 0), p["n_fwd"])
    fam = "".join(str(k) for k, ok in zip(FAMILIES_I8, (pi["n_windows"] > 0, windowed2_accepts(t, w2), coop is not None,
                                                      coop3 is not None)) if ok)
    return View(fam, pi["staircase"], pi["min_hazard"], pi["n_windows"], len(w2) if windowed2_accepts(t, w2) else 0,
                coop, coop3)


# ---- inputs ----------------------------------------------------------------

INPUTS = ("u128", "ties", "sat_flip")
GRID_PARAMS = [PD.CONTROL, PD.Params("OMS", 63, -127, 63), PD.Params("MS", 0, -127, 63)]
NMS_PARAMS = PD.Params("NMS", 64, -127, 63)      # coop3 (and generic) only
WIDE_PARAMS = PD.Params("OMS", 3, -127, 127)     # generic and windowed only
BATCHES = (1, 17, 65)
ITERS = (1, 2, 5)
SWEEP_BATCH, SWEEP_ITERS = 17, 2


def params_for(k):
    """The parameter sets family k (0: the automatic choice) runs in the core grid."""
    return GRID_PARAMS + ([NMS_PARAMS] if k in (0, 1, 8) else []) + ([WIDE_PARAMS] if k in (0, 1, 2) else [])


def oracle_i8(name, kind, batch, params, iters, early=False, llr=None):
    t = table(name)
    x = llr if llr is not None else PD.make_input(kind, batch, t.n)
    return PD.oracle_decode("struct:" + name, (kind, batch), x, params, iters, early, table=t)


# Early termination.  The tables are weak codes: most information variables have one edge, so a wrong saturated LLR
# is never turned (param_domain.FLIP_RATE's `sat_flip` stops nothing here).  et_input: every LLR -127 but a share p
# of the positions of a codeword, p = (b % 8 + 1) * 0.3 / sqrt(M D0 (D0 - 1) / 2) for codeword b (0.09 .. 5.8
# checks with two such positions expected per codeword).  They hold +6, which the first iterations turn, in three
# codewords of four (these stop after 1 or 2 iterations), and +127, which nothing turns, in every fourth (these
# never stop).  test_struct_domain_cpu.py asserts both on the oracle alone.
ET_BATCH, ET_ITERS = 65, 4
ET_STREAM = 7


def et_input(name):
    key = ("struct_et", name)
    if key not in PD._inputs:
        t = table(name)
        d0 = t.groups[0][0]
        r = PD._draw32(ET_BATCH, t.n, ET_STREAM)
        p = (np.arange(ET_BATCH) % 8 + 1) * 0.3 / np.sqrt(t.m * d0 * (d0 - 1) / 2.0)
        thr = (p * 2.0 ** 32).astype(np.uint64)[:, None]
        flip = np.where(np.arange(ET_BATCH) % 4 == 3, 127, 6)[:, None]
        x = np.ascontiguousarray(np.where(r < thr, flip, -127).astype(np.int8))
        x.setflags(write=False)
        PD._inputs[key] = x
    return PD._inputs[key]


def et_oracle(name):
    return PD.oracle_decode("struct:" + name, ("struct_et", ET_BATCH), et_input(name), PD.CONTROL, ET_ITERS, True,
                            table=table(name))


# Float: values k / 2, -16 <= k < 16, uniform (ties and zeros in most checks; plain and offset min-sum with a dyadic
# offset never round on them, as float_domain.py explains), so the comparison with the oracle is bit for bit.
F32_STREAM = 8
F32_ALGOS = {"MS": (O.OMS, 0.0), "OMS0.5": (O.OMS, 0.5)}
_f32 = {}


def f32_input(batch, n):
    key = ("struct_f32", batch, n)
    if key not in PD._inputs:
        r = PD._draw32(batch, n, F32_STREAM)
        x = np.ascontiguousarray((((r >> np.uint64(27)).astype(np.float32) - 16.0) * 0.5 + 0.0).astype(np.float32))
        x.setflags(write=False)
        PD._inputs[key] = x
    return PD._inputs[key]


def f32_et_input(name):
    """The float early-termination input: et_input halved (-63.5 and 3.0), its
    +127 doubled (254.0: float messages are not clamped, so only an LLR
    larger than every other one is never turned)."""
    key = ("struct_f32_et", name)
    if key not in PD._inputs:
        x = et_input(name).astype(np.float32)
        x = np.ascontiguousarray(np.where(x == 127, np.float32(254.0), x * np.float32(0.5)).astype(np.float32))
        x.setflags(write=False)
        PD._inputs[key] = x
    return PD._inputs[key]


def oracle_f32(name, batch, algo, iters, early=False, et=False):
    """(hard, soft, iters_used) of oracle.decode_f32 on f32_input (et: on
    f32_et_input, batch ET_BATCH), cached."""
    key = (name, batch, algo, iters, early, et)
    if key not in _f32:
        t = table(name)
        oalgo, beta = F32_ALGOS[algo]
        x = f32_et_input(name) if et else f32_input(batch, t.n)
        out = O.decode_f32(t, x, iters, oalgo, beta, early_term=early, threads=O.host_threads())
        for a in out:
            a.setflags(write=False)
        _f32[key] = out
    return _f32[key]


# ---- the pins --------------------------------------------------------------

# name: (the fast int8 families that accept the table, min_hazard, windows of the windowed plan, windows of the
# windowed2 plan, coop's (windows, empty windows, forwarded reads), coop3's (line-cache slots, windows, empty windows,
# forwarded reads)); 0 / None: no plan.  host_view() of the table, as the planners answered when this file was
# written.  stairf follows from min_hazard by stairf_widths(); every table but NOT_STAIRCASE is a staircase.
NOT_STAIRCASE = ("double_share_x5",)
PINS = {
    "x5_q1_h2": ("58", 2, 0, 0, (361, 180, 360), (13, 361, 180, 360)),
    "x5_q1_h3": ("58", 3, 0, 0, (241, 120, 360), (12, 241, 120, 360)),
    "x5_q1_h7": ("58", 7, 0, 0, (105, 52, 356), (21, 105, 52, 360)),
    "x5_q1_h8": ("58", 8, 0, 0, (91, 45, 360), (20, 91, 45, 360)), "x5_q1_h9": ("5", 9, 0, 0, (81, 40, 360), None),
    "x5_q1_h15": ("5", 15, 0, 0, (49, 24, 360), None), "x5_q1_h16": ("5", 16, 0, 0, (47, 23, 352), None),
    "x5_q1_h17": ("5", 17, 0, 0, (45, 22, 346), None), "x5_q1_h27": ("5", 27, 0, 0, (29, 14, 342), None),
    "x5_q1_h28": ("5", 28, 0, 0, (27, 13, 356), None), "x5_q1_h29": ("5", 29, 0, 0, (26, 0, 360), None),
    "x5_q1_h31": ("5", 31, 0, 0, (24, 0, 360), None), "x5_q1_h32": ("5", 32, 0, 0, (24, 0, 360), None),
    "x5_q1_h33": ("35", 33, 0, 33, (23, 0, 360), None), "x5_q1_h47": ("35", 47, 0, 24, (17, 0, 360), None),
    "x5_q1_h48": ("235", 48, 24, 24, (16, 0, 360), None), "x5_q1_h49": ("235", 49, 24, 24, (16, 0, 360), None),
    "x5_q1_h55": ("235", 55, 24, 24, (15, 0, 360), None), "x5_q1_h56": ("235", 56, 24, 24, (14, 0, 360), None),
    "x5_q1_h57": ("235", 57, 24, 24, (14, 0, 360), None), "x5_q1_h95": ("235", 95, 24, 24, (14, 0, 305), None),
    "x5_q1_h96": ("235", 96, 24, 24, (14, 0, 301), None), "x5_q1_h97": ("235", 97, 24, 24, (14, 0, 297), None),
    "x5_q1_h111": ("235", 111, 24, 24, (14, 0, 249), None), "x5_q1_h112": ("235", 112, 24, 24, (14, 0, 248), None),
    "x5_q1_h113": ("235", 113, 24, 24, (14, 0, 238), None), "x5_q1_h143": ("235", 143, 24, 24, (14, 0, 0), None),
    "x5_q1_h144": ("235", 144, 24, 24, (14, 0, 0), None), "x5_q1_h145": ("235", 145, 24, 24, (14, 0, 0), None),
    "x5_q7_h7": ("58", 7, 0, 0, (721, 360, 2520), (51, 721, 360, 2520)),
    "x5_q7_h14": ("5", 14, 0, 0, (361, 180, 2520), None), "x5_q7_h21": ("5", 21, 0, 0, (241, 120, 2520), None),
    "x5_q7_h28": ("5", 28, 0, 0, (181, 90, 2520), None), "x5_q7_h35": ("35", 35, 0, 217, (145, 0, 2520), None),
    "x5_q7_h42": ("35", 42, 0, 181, (121, 0, 2520), None), "x5_q7_h49": ("235", 49, 159, 159, (104, 0, 2520), None),
    "x5_q7_h56": ("235", 56, 159, 159, (91, 0, 2520), None), "x5_q7_h91": ("235", 91, 159, 159, (91, 0, 2493), None),
    "x5_q7_h98": ("235", 98, 159, 159, (91, 0, 2465), None),
    "x5_q7_h112": ("235", 112, 159, 159, (91, 0, 2408), None),
    "x5_q7_h140": ("2358", 140, 159, 159, (91, 0, 0), (181, 54, 0, 4833)),
    "x5_q7_h147": ("2358", 147, 159, 159, (91, 0, 0), (181, 54, 0, 4816)),
    "x5_q6_h6": ("58", 6, 0, 0, (721, 360, 2160), (44, 721, 360, 2160)),
    "x5_q6_h12": ("5", 12, 0, 0, (361, 180, 2160), None), "x5_q6_h18": ("5", 18, 0, 0, (241, 120, 2160), None),
    "x5_q6_h24": ("5", 24, 0, 0, (181, 90, 2160), None), "x5_q6_h30": ("5", 30, 0, 0, (145, 0, 2160), None),
    "x5_q6_h36": ("35", 36, 0, 181, (121, 0, 2160), None), "x5_q6_h48": ("235", 48, 136, 136, (91, 0, 2160), None),
    "x5_q6_h54": ("235", 54, 136, 136, (81, 0, 2160), None), "x5_q6_h60": ("235", 60, 136, 136, (79, 0, 2160), None),
    "x5_q6_h96": ("235", 96, 136, 136, (79, 0, 2064), None),
    "x5_q6_h108": ("235", 108, 136, 136, (79, 0, 2052), None),
    "x5_q6_h114": ("235", 114, 136, 136, (79, 0, 1899), None),
    "x5_q6_h144": ("2358", 144, 136, 136, (79, 0, 0), (181, 46, 0, 4201)),
    "x8_q1_h2": ("58", 2, 0, 0, (361, 180, 360), (18, 361, 180, 360)),
    "x8_q1_h3": ("58", 3, 0, 0, (241, 120, 360), (20, 241, 120, 360)),
    "x8_q1_h7": ("58", 7, 0, 0, (105, 52, 356), (38, 105, 52, 360)),
    "x8_q1_h8": ("58", 8, 0, 0, (91, 45, 360), (34, 91, 45, 360)), "x8_q1_h9": ("5", 9, 0, 0, (81, 40, 360), None),
    "x8_q1_h11": ("5", 11, 0, 0, (67, 33, 357), None), "x8_q1_h12": ("5", 12, 0, 0, (61, 30, 360), None),
    "x8_q1_h13": ("5", 13, 0, 0, (57, 28, 356), None), "x8_q1_h15": ("5", 15, 0, 0, (49, 24, 360), None),
    "x8_q1_h16": ("5", 16, 0, 0, (47, 23, 352), None), "x8_q1_h17": ("5", 17, 0, 0, (45, 22, 346), None),
    "x8_q1_h23": ("5", 23, 0, 0, (33, 16, 352), None), "x8_q1_h24": ("5", 24, 0, 0, (31, 15, 360), None),
    "x8_q1_h25": ("5", 25, 0, 0, (31, 15, 345), None), "x8_q1_h27": ("5", 27, 0, 0, (29, 14, 342), None),
    "x8_q1_h28": ("5", 28, 0, 0, (27, 13, 356), None), "x8_q1_h29": ("5", 29, 0, 0, (26, 0, 360), None),
    "x8_q1_h31": ("5", 31, 0, 0, (24, 0, 360), None), "x8_q1_h32": ("5", 32, 0, 0, (24, 0, 360), None),
    "x8_q1_h33": ("35", 33, 0, 33, (23, 0, 360), None), "x8_q1_h47": ("35", 47, 0, 24, (17, 0, 360), None),
    "x8_q1_h48": ("235", 48, 24, 24, (16, 0, 360), None), "x8_q1_h49": ("235", 49, 24, 24, (16, 0, 360), None),
    "x8_q1_h55": ("235", 55, 24, 24, (15, 0, 360), None), "x8_q1_h56": ("235", 56, 24, 24, (14, 0, 360), None),
    "x8_q1_h57": ("235", 57, 24, 24, (14, 0, 360), None), "x8_q1_h63": ("235", 63, 24, 24, (14, 0, 360), None),
    "x8_q1_h64": ("235", 64, 24, 24, (14, 0, 360), None), "x8_q1_h65": ("235", 65, 24, 24, (14, 0, 360), None),
    "x8_q1_h95": ("235", 95, 24, 24, (14, 0, 305), None), "x8_q1_h96": ("235", 96, 24, 24, (14, 0, 301), None),
    "x8_q1_h97": ("235", 97, 24, 24, (14, 0, 297), None), "x8_q1_h111": ("235", 111, 24, 24, (14, 0, 249), None),
    "x8_q1_h112": ("235", 112, 24, 24, (14, 0, 248), None), "x8_q1_h113": ("235", 113, 24, 24, (14, 0, 238), None),
    "x8_q1_h159": ("235", 159, 24, 24, (14, 0, 0), None), "x8_q1_h160": ("235", 160, 24, 24, (14, 0, 0), None),
    "x8_q1_h161": ("235", 161, 24, 24, (14, 0, 0), None),
    "x8_q5_h5": ("58", 5, 0, 0, (721, 360, 1800), (64, 721, 360, 1800)),
    "x8_q5_h10": ("5", 10, 0, 0, (361, 180, 1800), None), "x8_q5_h15": ("5", 15, 0, 0, (241, 120, 1800), None),
    "x8_q5_h20": ("5", 20, 0, 0, (181, 90, 1800), None), "x8_q5_h25": ("5", 25, 0, 0, (145, 72, 1800), None),
    "x8_q5_h30": ("5", 30, 0, 0, (121, 0, 1800), None), "x8_q5_h35": ("35", 35, 0, 155, (104, 0, 1800), None),
    "x8_q5_h45": ("35", 45, 0, 121, (81, 0, 1800), None), "x8_q5_h50": ("235", 50, 114, 114, (73, 0, 1800), None),
    "x8_q5_h55": ("235", 55, 114, 114, (67, 0, 1800), None), "x8_q5_h60": ("235", 60, 114, 114, (66, 0, 1800), None),
    "x8_q5_h65": ("235", 65, 114, 114, (66, 0, 1797), None),
    "x8_q5_h95": ("2358", 95, 114, 114, (66, 0, 1705), (316, 58, 0, 1800)),
    "x8_q5_h100": ("2358", 100, 114, 114, (66, 0, 1700), (316, 58, 0, 1800)),
    "x8_q5_h110": ("2358", 110, 114, 114, (66, 0, 1690), (316, 58, 0, 1776)),
    "x8_q5_h115": ("2358", 115, 114, 114, (66, 0, 1504), (316, 58, 0, 1756)),
    "x8_q5_h160": ("2358", 160, 114, 114, (66, 0, 0), (316, 58, 0, 1711)),
    "x8_q4_h4": ("58", 4, 0, 0, (721, 360, 1440), (54, 721, 360, 1440)),
    "x8_q4_h8": ("58", 8, 0, 0, (361, 180, 1440), (61, 361, 180, 1440)),
    "x8_q4_h12": ("5", 12, 0, 0, (241, 120, 1440), None), "x8_q4_h16": ("5", 16, 0, 0, (181, 90, 1440), None),
    "x8_q4_h24": ("5", 24, 0, 0, (121, 60, 1440), None), "x8_q4_h28": ("5", 28, 0, 0, (105, 52, 1424), None),
    "x8_q4_h32": ("5", 32, 0, 0, (91, 0, 1440), None), "x8_q4_h48": ("235", 48, 91, 91, (61, 0, 1440), None),
    "x8_q4_h56": ("235", 56, 91, 91, (53, 0, 1440), None), "x8_q4_h64": ("235", 64, 91, 91, (53, 0, 1440), None),
    "x8_q4_h96": ("2358", 96, 91, 91, (53, 0, 1344), (316, 46, 0, 1440)),
    "x8_q4_h112": ("2358", 112, 91, 91, (53, 0, 1328), (316, 46, 0, 1440)),
    "x8_q4_h160": ("2358", 160, 91, 91, (53, 0, 0), (316, 46, 0, 1359)),
    "x12_q1_h2": ("58", 2, 0, 0, (361, 180, 360), (26, 361, 180, 360)),
    "x12_q1_h3": ("58", 3, 0, 0, (241, 120, 360), (31, 241, 120, 360)),
    "x12_q1_h7": ("58", 7, 0, 0, (105, 52, 356), (55, 105, 52, 360)),
    "x12_q1_h8": ("58", 8, 0, 0, (91, 45, 360), (57, 91, 45, 360)), "x12_q1_h9": ("5", 9, 0, 0, (81, 40, 360), None),
    "x12_q1_h15": ("5", 15, 0, 0, (49, 24, 360), None), "x12_q1_h16": ("5", 16, 0, 0, (47, 23, 352), None),
    "x12_q1_h17": ("5", 17, 0, 0, (45, 22, 346), None), "x12_q1_h27": ("5", 27, 0, 0, (29, 14, 342), None),
    "x12_q1_h28": ("5", 28, 0, 0, (27, 13, 356), None), "x12_q1_h29": ("5", 29, 0, 0, (26, 0, 360), None),
    "x12_q1_h31": ("5", 31, 0, 0, (24, 0, 360), None), "x12_q1_h32": ("5", 32, 0, 0, (24, 0, 360), None),
    "x12_q1_h33": ("35", 33, 0, 33, (23, 0, 360), None), "x12_q1_h47": ("35", 47, 0, 24, (17, 0, 360), None),
    "x12_q1_h48": ("35", 48, 0, 24, (16, 0, 360), None), "x12_q1_h49": ("35", 49, 0, 24, (16, 0, 360), None),
    "x12_q1_h55": ("35", 55, 0, 24, (15, 0, 360), None), "x12_q1_h56": ("35", 56, 0, 24, (14, 0, 360), None),
    "x12_q1_h57": ("35", 57, 0, 24, (14, 0, 360), None), "x12_q1_h63": ("35", 63, 0, 24, (14, 0, 360), None),
    "x12_q1_h64": ("35", 64, 0, 24, (14, 0, 360), None), "x12_q1_h65": ("35", 65, 0, 24, (14, 0, 360), None),
    "x12_q1_h95": ("35", 95, 0, 24, (14, 0, 305), None), "x12_q1_h96": ("35", 96, 0, 24, (14, 0, 301), None),
    "x12_q1_h97": ("35", 97, 0, 24, (14, 0, 297), None), "x12_q1_h111": ("35", 111, 0, 24, (14, 0, 249), None),
    "x12_q1_h112": ("35", 112, 0, 24, (14, 0, 248), None), "x12_q1_h113": ("35", 113, 0, 24, (14, 0, 238), None),
    "x12_q1_h159": ("35", 159, 0, 24, (14, 0, 0), None), "x12_q1_h160": ("35", 160, 0, 24, (14, 0, 0), None),
    "x12_q1_h161": ("35", 161, 0, 24, (14, 0, 0), None),
    "x12_q5_h5": ("58", 5, 0, 0, (721, 360, 1800), (102, 721, 360, 1800)),
    "x12_q5_h10": ("5", 10, 0, 0, (361, 180, 1800), None), "x12_q5_h15": ("5", 15, 0, 0, (241, 120, 1800), None),
    "x12_q5_h20": ("5", 20, 0, 0, (181, 90, 1800), None), "x12_q5_h25": ("5", 25, 0, 0, (145, 72, 1800), None),
    "x12_q5_h30": ("5", 30, 0, 0, (121, 0, 1800), None), "x12_q5_h35": ("35", 35, 0, 155, (104, 0, 1800), None),
    "x12_q5_h45": ("35", 45, 0, 121, (81, 0, 1800), None), "x12_q5_h50": ("35", 50, 0, 114, (73, 0, 1800), None),
    "x12_q5_h55": ("35", 55, 0, 114, (67, 0, 1800), None), "x12_q5_h60": ("35", 60, 0, 114, (66, 0, 1800), None),
    "x12_q5_h65": ("35", 65, 0, 114, (66, 0, 1797), None),
    "x12_q5_h95": ("358", 95, 0, 114, (66, 0, 1705), (496, 58, 0, 1800)),
    "x12_q5_h100": ("358", 100, 0, 114, (66, 0, 1700), (496, 58, 0, 1800)),
    "x12_q5_h110": ("358", 110, 0, 114, (66, 0, 1690), (496, 58, 0, 1776)),
    "x12_q5_h115": ("358", 115, 0, 114, (66, 0, 1504), (496, 58, 0, 1756)),
    "x12_q5_h160": ("358", 160, 0, 114, (66, 0, 0), (496, 58, 0, 1701)),
    "x12_q4_h4": ("58", 4, 0, 0, (721, 360, 1440), (82, 721, 360, 1440)),
    "x12_q4_h8": ("58", 8, 0, 0, (361, 180, 1440), (97, 361, 180, 1440)),
    "x12_q4_h16": ("5", 16, 0, 0, (181, 90, 1440), None), "x12_q4_h28": ("5", 28, 0, 0, (105, 52, 1424), None),
    "x12_q4_h32": ("5", 32, 0, 0, (91, 0, 1440), None), "x12_q4_h48": ("35", 48, 0, 91, (61, 0, 1440), None),
    "x12_q4_h56": ("35", 56, 0, 91, (53, 0, 1440), None), "x12_q4_h64": ("35", 64, 0, 91, (53, 0, 1440), None),
    "x12_q4_h96": ("358", 96, 0, 91, (53, 0, 1344), (496, 46, 0, 1440)),
    "x12_q4_h112": ("358", 112, 0, 91, (53, 0, 1328), (496, 46, 0, 1440)),
    "x12_q4_h160": ("358", 160, 0, 91, (53, 0, 0), (496, 46, 0, 1280)),
    "x20_q1_h2": ("58", 2, 0, 0, (361, 180, 360), (37, 541, 360, 360)),
    "x20_q1_h3": ("58", 3, 0, 0, (241, 120, 360), (40, 361, 240, 360)),
    "x20_q1_h4": ("58", 4, 0, 0, (181, 90, 360), (47, 271, 180, 360)),
    "x20_q1_h5": ("58", 5, 0, 0, (145, 72, 360), (49, 217, 144, 360)),
    "x20_q1_h7": ("58", 7, 0, 0, (105, 52, 356), (56, 157, 104, 356)),
    "x20_q1_h8": ("58", 8, 0, 0, (91, 45, 360), (68, 136, 90, 360)),
    "x20_q1_h9": ("58", 9, 0, 0, (81, 40, 360), (72, 121, 80, 360)),
    "x20_q1_h15": ("58", 15, 0, 0, (49, 24, 360), (101, 73, 48, 360)),
    "x20_q1_h16": ("58", 16, 0, 0, (47, 23, 352), (105, 70, 46, 352)),
    "x20_q1_h17": ("58", 17, 0, 0, (45, 22, 346), (108, 66, 22, 360)),
    "x20_q1_h27": ("58", 27, 0, 0, (29, 14, 342), (174, 42, 14, 360)),
    "x20_q1_h28": ("58", 28, 0, 0, (27, 13, 356), (185, 40, 13, 360)),
    "x20_q1_h29": ("5", 29, 0, 0, (26, 0, 344), None), "x20_q1_h31": ("5", 31, 0, 0, (24, 0, 351), None),
    "x20_q1_h32": ("5", 32, 0, 0, (24, 0, 340), None), "x20_q1_h33": ("35", 33, 0, 33, (23, 0, 354), None),
    "x20_q1_h47": ("35", 47, 0, 24, (17, 0, 328), None), "x20_q1_h48": ("35", 48, 0, 24, (16, 0, 356), None),
    "x20_q1_h49": ("35", 49, 0, 24, (16, 0, 345), None), "x20_q1_h55": ("35", 55, 0, 24, (15, 0, 310), None),
    "x20_q1_h56": ("35", 56, 0, 24, (14, 0, 352), None), "x20_q1_h57": ("35", 57, 0, 24, (14, 0, 350), None),
    "x20_q1_h83": ("35", 83, 0, 24, (14, 0, 277), None), "x20_q1_h84": ("35", 84, 0, 24, (14, 0, 276), None),
    "x20_q1_h85": ("35", 85, 0, 24, (14, 0, 265), None), "x20_q1_h95": ("35", 95, 0, 24, (14, 0, 165), None),
    "x20_q1_h96": ("35", 96, 0, 24, (14, 0, 155), None), "x20_q1_h97": ("35", 97, 0, 24, (14, 0, 145), None),
    "x20_q3_h3": ("58", 3, 0, 0, (721, 360, 1080), (93, 1081, 720, 1080)),
    "x20_q3_h6": ("58", 6, 0, 0, (361, 180, 1080), (106, 541, 360, 1080)),
    "x20_q3_h9": ("58", 9, 0, 0, (241, 120, 1080), (123, 361, 240, 1080)),
    "x20_q3_h15": ("58", 15, 0, 0, (145, 72, 1080), (154, 217, 144, 1080)),
    "x20_q3_h18": ("58", 18, 0, 0, (121, 60, 1080), (184, 181, 60, 1080)),
    "x20_q3_h27": ("58", 27, 0, 0, (81, 40, 1080), (218, 121, 40, 1080)),
    "x20_q3_h30": ("58", 30, 0, 0, (73, 0, 1080), (231, 109, 36, 1080)),
    "x20_q3_h33": ("358", 33, 0, 99, (66, 0, 1076), (268, 99, 0, 1080)),
    "x20_q3_h48": ("358", 48, 0, 69, (46, 0, 1076), (341, 69, 0, 1080)),
    "x20_q3_h54": ("358", 54, 0, 69, (41, 0, 1080), (344, 69, 0, 1080)),
    "x20_q3_h57": ("358", 57, 0, 69, (40, 0, 1054), (349, 69, 0, 1080)),
    "x20_q3_h84": ("358", 84, 0, 69, (40, 0, 996), (347, 69, 0, 1017)),
    "x20_q3_h96": ("358", 96, 0, 69, (40, 0, 563), (355, 69, 0, 984)),
    "x20_q4_h4": ("58", 4, 0, 0, (721, 360, 1440), (132, 1081, 720, 1440)),
    "x20_q4_h8": ("58", 8, 0, 0, (361, 180, 1440), (137, 541, 360, 1440)),
    "x20_q4_h16": ("58", 16, 0, 0, (181, 90, 1440), (203, 271, 180, 1440)),
    "x20_q4_h28": ("58", 28, 0, 0, (105, 52, 1424), (261, 156, 52, 1440)),
    "x20_q4_h32": ("58", 32, 0, 0, (91, 0, 1440), (301, 136, 45, 1440)),
    "x20_q4_h48": ("358", 48, 0, 91, (61, 0, 1440), (351, 91, 0, 1440)),
    "x20_q4_h56": ("358", 56, 0, 91, (53, 0, 1408), (345, 91, 0, 1440)),
    "x20_q4_h84": ("358", 84, 0, 91, (53, 0, 1356), (347, 91, 0, 1417)),
    "x20_q4_h96": ("358", 96, 0, 91, (53, 0, 768), (335, 91, 0, 1344)),
    "x25_q1_h2": ("8", 2, 0, 0, None, (47, 541, 360, 360)), "x25_q1_h3": ("8", 3, 0, 0, None, (52, 361, 240, 360)),
    "x25_q1_h4": ("8", 4, 0, 0, None, (58, 271, 180, 360)), "x25_q1_h5": ("8", 5, 0, 0, None, (66, 217, 144, 360)),
    "x25_q1_h7": ("8", 7, 0, 0, None, (72, 157, 104, 356)), "x25_q1_h8": ("8", 8, 0, 0, None, (86, 136, 90, 360)),
    "x25_q1_h9": ("8", 9, 0, 0, None, (92, 121, 80, 360)), "x25_q1_h15": ("8", 15, 0, 0, None, (127, 73, 48, 360)),
    "x25_q1_h16": ("8", 16, 0, 0, None, (132, 70, 46, 352)), "x25_q1_h17": ("8", 17, 0, 0, None, (136, 66, 22, 360)),
    "x25_q1_h27": ("8", 27, 0, 0, None, (198, 42, 14, 360)), "x25_q1_h28": ("8", 28, 0, 0, None, (228, 40, 13, 360)),
    "x25_q1_h29": ("", 29, 0, 0, None, None), "x25_q1_h31": ("", 31, 0, 0, None, None),
    "x25_q1_h32": ("", 32, 0, 0, None, None), "x25_q1_h33": ("3", 33, 0, 33, None, None),
    "x25_q1_h47": ("3", 47, 0, 24, None, None), "x25_q1_h48": ("3", 48, 0, 24, None, None),
    "x25_q1_h49": ("3", 49, 0, 24, None, None), "x25_q1_h55": ("3", 55, 0, 24, None, None),
    "x25_q1_h56": ("3", 56, 0, 24, None, None), "x25_q1_h57": ("3", 57, 0, 24, None, None),
    "x25_q1_h83": ("3", 83, 0, 24, None, None), "x25_q1_h84": ("3", 84, 0, 24, None, None),
    "x25_q1_h85": ("3", 85, 0, 24, None, None), "x25_q1_h95": ("3", 95, 0, 24, None, None),
    "x25_q1_h96": ("3", 96, 0, 24, None, None), "x25_q1_h97": ("3", 97, 0, 24, None, None),
    "x25_q3_h3": ("8", 3, 0, 0, None, (127, 1081, 720, 1080)),
    "x25_q3_h6": ("8", 6, 0, 0, None, (133, 541, 360, 1080)),
    "x25_q3_h9": ("8", 9, 0, 0, None, (159, 361, 240, 1080)),
    "x25_q3_h15": ("8", 15, 0, 0, None, (191, 217, 144, 1080)),
    "x25_q3_h18": ("8", 18, 0, 0, None, (221, 181, 60, 1080)),
    "x25_q3_h27": ("8", 27, 0, 0, None, (286, 121, 40, 1080)),
    "x25_q3_h30": ("8", 30, 0, 0, None, (303, 109, 36, 1080)),
    "x25_q3_h33": ("38", 33, 0, 99, None, (388, 99, 0, 1080)),
    "x25_q3_h48": ("38", 48, 0, 69, None, (427, 69, 0, 1080)),
    "x25_q3_h54": ("38", 54, 0, 69, None, (428, 69, 0, 1080)),
    "x25_q3_h57": ("38", 57, 0, 69, None, (432, 69, 0, 1080)),
    "x25_q3_h84": ("38", 84, 0, 69, None, (442, 69, 0, 1017)),
    "x25_q3_h96": ("38", 96, 0, 69, None, (457, 69, 0, 984)),
    "x25_q6_h6": ("8", 6, 0, 0, None, (254, 1081, 720, 2160)),
    "x25_q6_h12": ("8", 12, 0, 0, None, (263, 541, 360, 2160)),
    "x25_q6_h18": ("8", 18, 0, 0, None, (309, 361, 120, 2160)),
    "x25_q6_h24": ("8", 24, 0, 0, None, (348, 271, 90, 2160)),
    "x25_q6_h30": ("8", 30, 0, 0, None, (443, 217, 72, 2160)),
    "x25_q6_h36": ("38", 36, 0, 181, None, (488, 181, 0, 2160)),
    "x25_q6_h48": ("38", 48, 0, 136, None, (525, 136, 0, 2160)),
    "x25_q6_h54": ("38", 54, 0, 136, None, (515, 136, 0, 2160)),
    "x25_q6_h60": ("38", 60, 0, 136, None, (530, 136, 0, 2160)),
    "x25_q6_h84": ("38", 84, 0, 136, None, (529, 136, 0, 2137)),
    "x25_q6_h96": ("38", 96, 0, 136, None, (537, 136, 0, 2064)),
    "x28_q1_h2": ("8", 2, 0, 0, None, (50, 541, 360, 360)), "x28_q1_h3": ("8", 3, 0, 0, None, (58, 361, 240, 360)),
    "x28_q1_h4": ("8", 4, 0, 0, None, (73, 271, 180, 360)), "x28_q1_h5": ("8", 5, 0, 0, None, (72, 217, 144, 360)),
    "x28_q1_h7": ("8", 7, 0, 0, None, (79, 157, 104, 356)), "x28_q1_h8": ("8", 8, 0, 0, None, (97, 136, 90, 360)),
    "x28_q1_h9": ("8", 9, 0, 0, None, (107, 121, 80, 360)), "x28_q1_h15": ("8", 15, 0, 0, None, (143, 73, 48, 360)),
    "x28_q1_h16": ("8", 16, 0, 0, None, (145, 70, 46, 352)), "x28_q1_h17": ("8", 17, 0, 0, None, (156, 66, 22, 360)),
    "x28_q1_h27": ("8", 27, 0, 0, None, (247, 42, 14, 360)), "x28_q1_h28": ("8", 28, 0, 0, None, (267, 40, 13, 360)),
    "x28_q1_h29": ("", 29, 0, 0, None, None), "x28_q1_h31": ("", 31, 0, 0, None, None),
    "x28_q1_h32": ("", 32, 0, 0, None, None), "x28_q1_h33": ("3", 33, 0, 33, None, None),
    "x28_q1_h47": ("3", 47, 0, 24, None, None), "x28_q1_h48": ("3", 48, 0, 24, None, None),
    "x28_q1_h49": ("3", 49, 0, 24, None, None), "x28_q1_h55": ("3", 55, 0, 24, None, None),
    "x28_q1_h56": ("3", 56, 0, 24, None, None), "x28_q1_h57": ("3", 57, 0, 24, None, None),
    "x28_q1_h83": ("3", 83, 0, 24, None, None), "x28_q1_h84": ("3", 84, 0, 24, None, None),
    "x28_q1_h85": ("3", 85, 0, 24, None, None), "x28_q1_h95": ("3", 95, 0, 24, None, None),
    "x28_q1_h96": ("3", 96, 0, 24, None, None), "x28_q1_h97": ("3", 97, 0, 24, None, None),
    "x28_q5_h5": ("8", 5, 0, 0, None, (230, 1081, 720, 1800)),
    "x28_q5_h10": ("8", 10, 0, 0, None, (236, 541, 360, 1800)),
    "x28_q5_h15": ("8", 15, 0, 0, None, (292, 361, 240, 1800)),
    "x28_q5_h20": ("8", 20, 0, 0, None, (324, 271, 90, 1800)),
    "x28_q5_h25": ("8", 25, 0, 0, None, (390, 217, 72, 1800)),
    "x28_q5_h30": ("8", 30, 0, 0, None, (469, 181, 60, 1800)),
    "x28_q5_h35": ("38", 35, 0, 155, None, (445, 155, 0, 1800)),
    "x28_q5_h45": ("38", 45, 0, 121, None, (530, 121, 0, 1800)),
    "x28_q5_h50": ("38", 50, 0, 114, None, (583, 114, 0, 1800)),
    "x28_q5_h55": ("38", 55, 0, 114, None, (565, 114, 0, 1800)),
    "x28_q5_h60": ("38", 60, 0, 114, None, (596, 114, 0, 1800)),
    "x28_q5_h80": ("38", 80, 0, 114, None, (571, 114, 0, 1760)),
    "x28_q5_h85": ("38", 85, 0, 114, None, (605, 114, 0, 1731)),
    "x28_q5_h95": ("38", 95, 0, 114, None, (600, 114, 0, 1705)),
    "x28_q5_h100": ("38", 100, 0, 114, None, (583, 114, 0, 1275)),
    "x28_q6_h6": ("8", 6, 0, 0, None, (290, 1081, 720, 2160)),
    "x28_q6_h12": ("8", 12, 0, 0, None, (292, 541, 360, 2160)),
    "x28_q6_h18": ("8", 18, 0, 0, None, (358, 361, 120, 2160)),
    "x28_q6_h24": ("8", 24, 0, 0, None, (391, 271, 90, 2160)),
    "x28_q6_h30": ("8", 30, 0, 0, None, (474, 217, 72, 2160)),
    "x28_q6_h36": ("38", 36, 0, 181, None, (513, 181, 0, 2160)),
    "x28_q6_h48": ("38", 48, 0, 136, None, (591, 136, 0, 2160)),
    "x28_q6_h54": ("38", 54, 0, 136, None, (607, 136, 0, 2160)),
    "x28_q6_h60": ("38", 60, 0, 136, None, (601, 136, 0, 2160)),
    "x28_q6_h84": ("38", 84, 0, 136, None, (606, 136, 0, 2137)),
    "x28_q6_h96": ("38", 96, 0, 136, None, (612, 136, 0, 2064)),
    "m_x5_q2_h6": ("58", 6, 0, 0, (241, 120, 720), (23, 241, 120, 720)),
    "m_x5_q2_h60": ("235", 60, 46, 46, (27, 0, 720), None), "m_x5_q7_h14": ("5", 14, 0, 0, (361, 180, 5027), None),
    "m_x5_q7_h56": ("235", 56, 159, 159, (91, 0, 5040), None), "m_x8_q2_h40": ("35", 40, 0, 55, (37, 0, 720), None),
    "m_x8_q7_h7": ("58", 7, 0, 0, (721, 360, 5026), (78, 721, 360, 5040)),
    "m_x8_q3_h12": ("5", 12, 0, 0, (181, 90, 3224), None), "m_x12_q7_h35": ("35", 35, 0, 217, (145, 0, 5040), None),
    "m_x20_q2_h4": ("58", 4, 0, 0, (361, 180, 720), (71, 541, 360, 720)),
    "m_x25_q7_h21": ("8", 21, 0, 0, None, (353, 361, 120, 5036)),
    "m_x28_q2_h20": ("8", 20, 0, 0, None, (207, 109, 36, 720)),
    "perm_x5_q1_h57": ("235", 57, 24, 24, (14, 0, 360), None),
    "perm_x5_q1_h3": ("58", 3, 0, 0, (241, 120, 360), (12, 241, 120, 360)),
    "perm_x8_q5_h110": ("2358", 110, 114, 114, (66, 0, 1690), (316, 58, 0, 1776)),
    "perm_x20_q4_h48": ("358", 48, 0, 91, (61, 0, 1440), (351, 91, 0, 1440)),
    "deg8_q1_h57": ("", 57, 0, 0, None, None), "three_groups_x5": ("", 57, 0, 0, None, None),
    "double_share_x5": ("", 1, 0, 0, None, None), "short_x5_m140": ("23", 70, 10, 10, None, None),
    "short_x5_m168": ("235", 84, 12, 12, (7, 0, 336), None), "short_x20_m112": ("3", 56, 0, 8, None, None),
    "short_x20_m140": ("35", 70, 0, 10, (6, 0, 198), None), "second_x5_c1": ("23", 57, 24, 25, None, None),
    "second_x5_c15": ("23", 57, 23, 24, None, None), "second_x5_c16": ("23", 57, 24, 24, None, None),
    "second_x5_c17": ("23", 57, 24, 25, None, None), "second_x8_c1": ("23", 57, 24, 25, None, None),
    "second_x8_c15": ("23", 57, 23, 24, None, None), "second_x8_c16": ("23", 57, 24, 24, None, None),
    "second_x8_c17": ("23", 57, 24, 25, None, None),
}


def families(name):
    """The fast int8 families pinned as accepting the table, as numbers."""
    return [int(ch) for ch in PINS[name][0]]


def widths(name):
    """The stairf group widths the table gets by its pinned min_hazard (empty: stairf refuses)."""
    return () if name in NOT_STAIRCASE else stairf_widths(table(name), PINS[name][1])


# the core set, run over the whole grid of inputs, parameters, batches and iterations: each family's densest and
# plainest schedules, every first-group degree, a mixed-row table, a permuted one and a second group of 17 checks
CORE = ["x5_q1_h2", "x5_q1_h33", "x5_q1_h57", "x5_q6_h144", "x8_q1_h8", "x8_q5_h110", "x12_q4_h8", "x12_q5_h110",
        "x20_q3_h18", "x25_q3_h33", "x28_q6_h6", "m_x5_q7_h14", "m_x8_q7_h7", "perm_x20_q4_h48", "second_x5_c16"]
# early termination: one table per accepting family (2, 3, 5, 8; stairf on the first and the last)
ET_TABLES = {2: "x5_q1_h57", 3: "x12_q5_h45", 5: "m_x8_q3_h12", 8: "x20_q3_h18"}
ET_TABLES_F32 = ("x5_q1_h57", "x20_q3_h18")
COOP_PER_LAUNCH_ET = "x8_q1_h13"              # LDPC_COOP_ET_KERNEL=0
NODE_MAJOR = {5: "x12_q1_h17", 8: "x8_q4_h8"}   # decode_i8_nm_device with ld > batch
