"""The CPU side of the schedule-domain tests (struct_domain.py): the synthetic
staircase tables on the host.

* every table is what its name says: shape, degree groups, min_hazard = q delta
  in numpy and through ldpc_code_plan_info, the Annex-B ones equal to what
  ldpc_code_load reads from their .txt;
* the pins of struct_domain.PINS against what the schedule builders answer on
  the host (ldpc_plan_build, ldpc_plan_windows, coop_build_plan, coop3_plan_host
  + lc_build_plan): which family accepts the table, window / empty-window /
  forwarded-read counts, line-cache slots;
* the conditions that make the sweep worth running (every family accepts
  tables, coop3 at every degree, schedules with empty windows and with more
  forwarded reads than checks, every stairf width set);
* the schedule rules re-derived in numpy for every accepted plan, with the
  helpers of test_coop_plan.py and test_window_plan.py;
* the host decoder (device = -1) against the oracle on every table, bit for
  bit, so that a mismatch test_gpu_struct_domain.py finds is a kernel, planner
  or predicate bug, not a checker bug;
* the early-termination inputs stop some codewords and not others, on the
  oracle alone."""
import numpy as np
import pytest

import param_domain as PD
import struct_domain as ST
from ldpcgputegra_amd import Code, Decoder
from test_coop_plan import check_coop_plan, checks
from test_window_plan import check_window_plan

_views = {}


def view(name):
    if name not in _views:
        _views[name] = ST.host_view(ST.table(name))
    return _views[name]


def test_restated_constants():
    """The literals restated in struct_domain.py, as the kernels' headers give
    them per first-group degree, and the sweep brackets each of them."""
    assert {d: (ST.g3_s(d), ST.g3_dist(d)) for d in ST.DEGREES} == {7: (48, 1), 10: (32, 1), 14: (32, 1), 22: (16, 2),
                                                                  27: (16, 2), 30: (16, 2)}
    assert {d: ST.coop_r(d) for d in ST.COOP_D0} == {7: 3, 10: 3, 14: 3, 22: 2}
    assert {X: [S * ST.p_of_s(X, S) for S in ST.STAIRF_S] for X in ST.XS} == {
        5: [16, 32, 48, 48], 8: [12, 24, 48, 48], 12: [8, 16, 32, 48], 20: [4, 8, 16, 32], 25: [4, 8, 16, 32],
        28: [4, 8, 16, 32]}
    names = {s.name for s in ST.SWEEP}
    for X in ST.XS:
        for what, h in ST.constants(X).items():
            for d in (-1, 0, 1):
                if 2 <= h + d <= ST.H_MAX:
                    assert "x%d_q1_h%d" % (X, h + d) in names, (X, what)
        # M % 16 == 8 and M % 16 == 0, q in 3 .. 9
        assert sorted(360 * q % 16 for q in ST.LARGE_Q[X]) == [0, 8] and all(3 <= q <= 9 for q in ST.LARGE_Q[X])
    assert set(ST.PINS) == set(ST.NAMES) and len(ST.NAMES) == len(set(ST.NAMES))
    assert set(ST.CORE) <= set(ST.NAMES) and len(ST.CORE) <= 16


@pytest.mark.parametrize("name", ST.NAMES)
def test_table_and_pins(name, tmp_path):
    t = ST.table(name)
    assert t.n <= 12000 and ST.table(name) is t
    code = Code(t)
    back = code.table()
    assert back.groups == t.groups and np.array_equal(back.edge_var, t.edge_var)
    if name in ST.ANNEXB:
        spec = ST.ANNEXB[name]
        X = sum(spec.c)
        assert (t.n, t.m) == (360 * (len(spec.c) + spec.q), 360 * spec.q)
        assert t.groups == [(X + 2, t.m - 1), (X + 1, 1)]
        assert ST.min_hazard(t) == spec.q * spec.delta == ST.PINS[name][1]
        path = tmp_path / (name + ".txt")
        path.write_text(ST.rows_text(spec.q, ST.annexb(spec)[1]))
        loaded = Code(str(path)).table()
        assert loaded.groups == t.groups and np.array_equal(loaded.edge_var, t.edge_var)
    v = view(name)
    assert v.staircase == (name not in ST.NOT_STAIRCASE)
    assert v.hazard == ST.min_hazard(t)
    assert tuple(v)[:1] + tuple(v)[2:] == ST.PINS[name], "the planners' answer changed: %r" % (v,)


def test_hand_built_tables_are_what_they_say():
    for X, c in ST.SECOND_GROUP:
        t = ST.table("second_x%d_c%d" % (X, c))
        assert t.groups == [(X + 2, 359 - c), (X + 1, c + 1)]
        fam = ST.families("second_x%d_c%d" % (X, c))
        assert (2 in fam or 3 in fam) and 5 not in fam and 8 not in fam
        assert ST.widths("second_x%d_c%d" % (X, c)) == ()
    assert ST.table("deg8_q1_h57").groups == [(8, 359), (7, 1)]
    assert ST.table("three_groups_x5").groups == [(7, 356), (5, 3), (6, 1)]
    ch = checks(ST.table("double_share_x5"))
    assert len(set(ch[10]) & set(ch[11])) == 2 and ST.table("double_share_x5").groups == [(7, 359), (6, 1)]
    for name in ST.REFUSED_BY_ALL:
        assert ST.families(name) == [] and ST.widths(name) == (), name
    # permuted: the same H as the base table, the information edges of some check out of order
    for name, base in (("perm_x5_q1_h57", "x5_q1_h57"), ("perm_x20_q4_h48", "x20_q4_h48")):
        a, b = checks(ST.table(name)), checks(ST.table(base))
        X = ST.table(base).groups[0][0] - 2
        assert all(sorted(x[:X]) == y[:X] and x[X:] == y[X:] for x, y in zip(a, b))
        assert sum(x[:X] != y[:X] for x, y in zip(a, b)) > 0.9 * len(a)
        assert ST.PINS[name] == ST.PINS[base]       # the schedules do not depend on the order inside a check


def test_conditions_of_the_sweep():
    acc = {k: [n for n in ST.NAMES if k in ST.families(n)] for k in ST.FAMILIES_I8}
    ref = {k: [n for n in ST.NAMES if k not in ST.families(n)] for k in ST.FAMILIES_I8}
    sf = {n: ST.widths(n) for n in ST.NAMES}
    print({k: (len(acc[k]), len(ref[k])) for k in acc}, "stairf",
          (sum(1 for w in sf.values() if w), sum(1 for w in sf.values() if not w)))
    assert all(len(acc[k]) >= 4 and len(ref[k]) >= 4 for k in ST.FAMILIES_I8)
    assert sum(1 for w in sf.values() if w) >= 4
    assert {ST.table(n).groups[0][0] for n in acc[8]} == set(ST.DEGREES)
    assert {ST.table(n).groups[0][0] for n in acc[5]} == set(ST.COOP_D0)
    assert {ST.table(n).groups[0][0] for n in acc[2]} == set(ST.WINDOWED_D0)
    assert {ST.table(n).groups[0][0] for n in acc[3]} == set(ST.DEGREES)
    # schedules unlike a shipped table's: more than a third of the windows empty, more forwarded reads than checks
    for k, at in ((5, 4), (8, 5)):
        plans = {n: ST.PINS[n][at] for n in acc[k]}
        windows = lambda p: p[-3:]
        assert any(windows(p)[1] > windows(p)[0] / 3 for p in plans.values()), k
        assert any(windows(p)[2] > ST.table(n).m for n, p in plans.items()), k
    # coop3 at its least number of windows (fewer: test_coop3_refusals_have_their_reason), coop at and below R + 4
    assert min(ST.PINS[n][5][1] for n in acc[8]) == 4 * ST.LC_GAP
    assert ST.PINS["short_x5_m168"][4][0] == ST.coop_r(7) + 4 and 5 not in ST.families("short_x5_m140")
    assert ST.PINS["short_x20_m140"][4][0] == ST.coop_r(22) + 4 and 5 not in ST.families("short_x20_m112")
    # stairf: every width available, and only the narrowest; tables it refuses for their min_hazard alone
    assert {(2,), (2, 4), (2, 4, 8), (2, 4, 8, 16), ()} <= set(sf.values())
    for X in ST.XS:
        mine = {sf[s.name] for s in ST.SWEEP if sum(s.c) == X}
        assert {(2,), (2, 4, 8, 16), ()} <= mine, X
    # windowed and windowed2 windows in the second group that carry a chain input
    assert all(2 in ST.families(n) and 3 in ST.families(n) for n in ST.NAMES if n.startswith("second_"))


def _fixed_windows(t):
    """windowed's windows (plan.cpp ldpc_plan_build): runs of <= 16 checks of one group."""
    out, c = [], 0
    for _, cnt in t.groups:
        for first in range(c, c + cnt, ST.WIN_S):
            out.append((first, min(ST.WIN_S, c + cnt - first)))
        c += cnt
    return out


def _distance2_checks(t, plan):
    """Per window of a dist-1 coop3 plan: the checks that read a variable whose
    latest writer is two windows back, or are such a writer (coop3_plan_host
    moves them into slab wave 0, which holds 8)."""
    X, wins = t.groups[0][0] - 2, plan["windows"]
    nw, ch = len(wins), checks(t)
    last, special = {}, [set() for _ in wins]
    for pas in range(2):
        for u, (first, cnt) in enumerate(wins):
            for c in range(first, first + cnt):
                for v in ch[c][:X]:
                    if pas and v in last and (u - last[v][0]) % nw == 2:
                        special[u].add(c)
                        special[last[v][0]].add(last[v][1])
                    last[v] = (u, c)
    return [len(s) for s in special]


@pytest.mark.parametrize("name", [n for n in ST.NAMES if ST.PINS[n][0]])
def test_schedule_rules(name):
    """Tiling, no shared information variable inside a window or within `dist`
    windows cyclically, the forwarded-read count (check_coop_plan), at most 8
    distance-2 checks per coop3 window, and the windowed / windowed2 rules
    (check_window_plan), for every plan a family accepts."""
    t = ST.table(name)
    code, d0, fam = Code(t), t.groups[0][0], ST.families(name)
    if 5 in fam:
        plan = code.coop_plan(ST.COOP_S, ST.coop_r(d0), 1)
        check_coop_plan(t, plan, ST.COOP_S, ST.coop_r(d0), 1)
        assert len(plan["windows"]) >= ST.coop_r(d0) + 4
    if 8 in fam:
        S, dist = ST.g3_s(d0), ST.g3_dist(d0)
        plan = code.coop_plan(S, ST.COOP3_R, dist)
        check_coop_plan(t, plan, S, ST.COOP3_R, dist)
        assert len(plan["windows"]) >= 4 * ST.LC_GAP
        d2 = _distance2_checks(t, plan)
        assert max(d2) <= ST.COOP3_WAVE0 and (dist == 1 or max(d2) == 0)
        lc = code.coop3_line_cache()
        assert 2 <= lc["slots"] <= lc["max_slots"]
    if 3 in fam:
        check_window_plan(t, code.window_plan(ST.WIN_S, ST.WIN2_P), ST.WIN_S, ST.WIN2_P)
    if 2 in fam:
        fixed = _fixed_windows(t)
        assert len(fixed) == ST.PINS[name][2]
        check_window_plan(t, fixed, ST.WIN_S, ST.WIN_LOOKAHEAD, chain_break_ok=True)


def test_coop3_refusals_have_their_reason():
    """Where coop3 refuses a table of a degree it is built for although the
    window plan exists: too few windows for the line cache, or more distance-2
    checks in a window than slab wave 0 holds -- the two refusals this sweep
    is after (delta 9 at degree 7: nine such checks)."""
    seen = set()
    for s in ST.SWEEP:
        if 8 in ST.families(s.name):
            continue
        t = ST.table(s.name)
        d0 = t.groups[0][0]
        plan = Code(t).coop_plan(ST.g3_s(d0), ST.COOP3_R, ST.g3_dist(d0))
        if plan is None:
            seen.add("plan")
        elif len(plan["windows"]) < 4 * ST.LC_GAP:
            seen.add("windows")
        else:
            assert ST.g3_dist(d0) == 1 and max(_distance2_checks(t, plan)) > ST.COOP3_WAVE0, s.name
            seen.add("wave0")
    assert {"windows", "wave0"} <= seen
    assert max(_distance2_checks(ST.table("x5_q1_h9"), Code(ST.table("x5_q1_h9")).coop_plan(48, 4, 1))) == 9


# ---- the host decoder against the oracle -----------------------------------

def _host_vs_oracle(dec, name, kind, batch, params, iters, early=False, llr=None):
    t = ST.table(name)
    x = llr if llr is not None else PD.make_input(kind, batch, t.n)
    exp, _, eit = ST.oracle_i8(name, kind, batch, params, iters, early, llr=x)
    got = dec.decode_i8(x, iters, params.product(early_term=int(early)))
    assert dec.last_kernel == "host"
    diff = int((got != exp).sum())
    assert diff == 0, "%s %s %s batch %d: %d hard decisions differ from the oracle" % (name, kind, params.id, batch, diff)
    return eit


@pytest.mark.parametrize("name", ST.NAMES)
def test_host_decoder_equals_oracle(name):
    """Every table: the sweep's decode (`u128`, the default parameters, batch
    17, 2 iterations) and `sat_flip` under OMS 63 / 63; the core tables over
    the inputs and parameters of the grid at 5 iterations."""
    dec = Decoder(Code(ST.table(name)), device=-1, max_batch=ST.ET_BATCH)
    _host_vs_oracle(dec, name, "u128", ST.SWEEP_BATCH, PD.CONTROL, ST.SWEEP_ITERS)
    _host_vs_oracle(dec, name, "sat_flip", ST.SWEEP_BATCH, ST.GRID_PARAMS[1], ST.SWEEP_ITERS)
    if name in ST.CORE:
        for kind in ST.INPUTS:
            for params in ST.params_for(0):
                _host_vs_oracle(dec, name, kind, ST.SWEEP_BATCH, params, ST.ITERS[-1])
    dec.close()


@pytest.mark.parametrize("name", sorted(set(ST.ET_TABLES.values()) | {ST.COOP_PER_LAUNCH_ET}))
def test_early_termination_inputs_stop_some_codewords(name):
    """struct_domain.et_input, chosen by the oracle alone: of the 65 codewords
    some stop before the last of the 4 iterations and some never do, in the
    first 16-codeword group as well; the host decoder agrees."""
    llr = ST.et_input(name)
    assert llr.shape == (ST.ET_BATCH, ST.table(name).n) and set(np.unique(llr).tolist()) == {-127, 6, 127}
    _, _, eit = ST.et_oracle(name)
    print(name, "iterations used:", np.bincount(eit, minlength=ST.ET_ITERS + 1).tolist())
    assert eit.min() < ST.ET_ITERS and (eit == ST.ET_ITERS).sum() >= 4 and (eit < ST.ET_ITERS).sum() >= 4
    assert eit[:16].min() < ST.ET_ITERS == eit[:16].max()
    dec = Decoder(Code(ST.table(name)), device=-1, max_batch=ST.ET_BATCH)
    _host_vs_oracle(dec, name, "struct_et", ST.ET_BATCH, PD.CONTROL, ST.ET_ITERS, early=True, llr=llr)
    dec.close()


@pytest.mark.parametrize("name", ST.ET_TABLES_F32)
def test_float_early_termination_inputs_stop_some_codewords(name):
    _, _, eit = ST.oracle_f32(name, ST.ET_BATCH, "MS", ST.ET_ITERS, early=True, et=True)
    print(name, "iterations used:", np.bincount(eit, minlength=ST.ET_ITERS + 1).tolist())
    assert eit.min() < ST.ET_ITERS and (eit == ST.ET_ITERS).sum() >= 4 and (eit < ST.ET_ITERS).sum() >= 4


def test_float_inputs_are_dyadic_with_ties_and_zeros():
    x = ST.f32_input(ST.SWEEP_BATCH, 1800)
    assert x.dtype == np.float32 and np.array_equal(x * 2, np.rint(x * 2)) and np.abs(x).max() <= 8.0
    assert (x == 0).mean() > 0.02 and not np.signbit(x[x == 0]).any() and len(np.unique(x)) == 32
