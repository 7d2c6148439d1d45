"""The staircase kernels on synthetic tables (struct_domain.py): windowed (2),
windowed2 (3), coop (5), coop3 (8) and stairf (11), beside generic (1) and the
automatic choice (0), on small staircase tables whose schedules no shipped
DVB-S2 table gives -- empty windows, windows cut short by a conflict, the
padding windows at the iteration wrap, forwarding at every distance, coop3's
slab wave 0 full of distance-2 checks, line caches of a few dozen slots, few
windows, stairf's width tables dropping out one by one, second-group windows
that carry a chain input.

One invariant, for every table and every family k of {1, 2, 3, 5, 8} (int8)
and {1, 11} (float):

* the family refuses the table: Decoder.set_kernel(k) raises LDPC_EUNSUPPORTED;
* it accepts it: last_kernel == k, and hard, soft and iters_used equal the
  oracle's bit for bit (the float ones as test_gpu_float_domain.py compares
  them, the sign of a zero included), the rows behind each output untouched;
* the automatic choice equals the oracle too.

Which of the two holds is pinned per table in struct_domain.PINS (and, for
stairf, follows from the pinned min_hazard by the rule restated there), so a
family that drops out turns a test red.  test_struct_domain_cpu.py shows that
the pins are what the schedule builders answer on the host, that the plans
keep the rules the kernels rely on, and that the host decoder equals the
oracle on every table.

Shapes: the sweep runs one input, the default parameters, batch 17 (one
ragged 16-codeword group) and 2 iterations (the cyclic wrap of a schedule
shows from the second); the core tables run `u128`, `ties` and `sat_flip`
under the default parameters, OMS 63 / 63, MS / 63, NMS 64 / 63 (coop3) and
OMS 3 / 127 (generic, windowed), batches 1, 17 and 65, 1, 2 and 5 iterations."""
import numpy as np
import pytest

import param_domain as PD
import struct_domain as ST
from ldpcgputegra_amd import ALGO_MS, ALGO_OMS, Code, Decoder, LdpcError, _lib, default_params
from test_gpu_float_domain import assert_same
from test_gpu_short_domain import assert_equal, run

pytestmark = pytest.mark.gpu

NAME_OF = Decoder.KERNEL_NAMES
F32_PRODUCT = {"MS": (ALGO_MS, 0.0), "OMS0.5": (ALGO_OMS, 0.5)}
_device_inputs = {}


def _torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def device(x, key):
    if key not in _device_inputs:
        _device_inputs[key] = _torch().from_numpy(np.array(x)).cuda()
    return _device_inputs[key]


def device_input(kind, batch, n):
    return device(PD.make_input(kind, batch, n), (kind, batch, n))


def context(name, max_batch=ST.ET_BATCH):
    return Decoder(Code(ST.table(name)), max_batch=max_batch)


def take(dec, name, k):
    """set_kernel(k): True when the family accepts the table, as pinned; a
    refusal must be LDPC_EUNSUPPORTED and pinned too."""
    wanted = k in (0, 1) or (bool(ST.widths(name)) if k == ST.STAIRF else k in ST.families(name))
    try:
        dec.set_kernel(k)
    except LdpcError as e:
        assert e.status == _lib.LDPC_EUNSUPPORTED, (name, k, str(e))
        assert not wanted, "%s: family %d (%s) refuses a table pinned as accepted" % (name, k, NAME_OF[k])
        return False
    assert wanted, "%s: family %d (%s) accepts a table pinned as refused" % (name, k, NAME_OF[k])
    return True


def auto_i8(name):
    """The automatic choice's family (dispatch.hip pick_kernel), where the
    pins decide it: coop3, coop, windowed2 in that order."""
    fam = ST.families(name)
    return next((NAME_OF[k] for k in (8, 5, 3) if k in fam), None)


def check_i8(dec, name, k, kind, batch, params, iters, d_llr=None, early=False, node_major=False, llr=None):
    exp = ST.oracle_i8(name, kind, batch, params, iters, early, llr=llr)
    d = d_llr if d_llr is not None else device_input(kind, batch, ST.table(name).n)
    got = run(dec, d, iters, params.product(early_term=int(early)), batch=batch, extra=2, node_major=node_major)
    where = "%s %s %s batch %d, %d iterations, kernel %d (%s)" % (name, kind, params.id, batch, iters, k, dec.last_kernel)
    if k:
        assert dec.last_kernel == NAME_OF[k], where
    else:
        auto = auto_i8(name)
        assert dec.last_kernel == auto if auto else dec.last_kernel in ("lds", "windowed", "generic"), where
    assert_equal(got, exp, where)
    return exp


def run_f32(dec, d_llr, iters, params, extra=2):
    torch = _torch()
    B, n = d_llr.shape
    d_hard = torch.full((B + extra, n), 9, dtype=torch.uint8, device="cuda")
    d_soft = torch.full((B + extra, n), 99.0, dtype=torch.float32, device="cuda")
    d_its = torch.full((B + extra,), -7, dtype=torch.int32, device="cuda")
    dec.decode_f32_device(d_llr, d_hard, iters, params=params, soft=d_soft, iters_used=d_its)
    torch.cuda.synchronize()
    hard, soft, its = d_hard.cpu().numpy(), d_soft.cpu().numpy(), d_its.cpu().numpy()
    assert (hard[B:] == 9).all() and (soft[B:] == 99.0).all() and (its[B:] == -7).all(), "rows beyond the batch written"
    return hard[:B], soft[:B], its[:B]


def check_f32(dec, name, k, batch, algo, iters, monkeypatch, early=False, et=False):
    """Family k (0, 1 or 11) in float; stairf at each group width the table
    has, forced through LDPC_STAIRF_S."""
    t = ST.table(name)
    exp = ST.oracle_f32(name, batch, algo, iters, early, et)
    x = ST.f32_et_input(name) if et else ST.f32_input(batch, t.n)
    d = device(x, ("f32", name if et else None, batch, t.n))
    palgo, beta = F32_PRODUCT[algo]
    params = default_params(algo=palgo, beta=beta, early_term=int(early))
    widths = ST.widths(name)
    for S in (widths if k == ST.STAIRF else (None,)):
        if S:
            assert ST.stairf_width_taken(widths, S) == S
            monkeypatch.setenv("LDPC_STAIRF_S", str(S))
        else:
            monkeypatch.delenv("LDPC_STAIRF_S", raising=False)
        got = run_f32(dec, d, iters, params)
        where = "%s float %s batch %d, %d iterations, kernel %d (%s) width %s" % (name, algo, batch, iters, k,
                                                                                 dec.last_kernel, S)
        if k:
            assert dec.last_kernel == NAME_OF[k], where
        else:
            assert dec.last_kernel == "stairf" if widths else dec.last_kernel in ("ldsep", "lds", "generic"), where
        assert_same(got, exp, where, bitwise=dec.last_kernel != "ldsep")
    monkeypatch.delenv("LDPC_STAIRF_S", raising=False)
    return exp


@pytest.mark.parametrize("name", ST.NAMES)
def test_sweep(name, monkeypatch):
    """Every table, every family: refused as pinned, or equal to the oracle on
    `u128` under the default parameters (int8) and on the dyadic float input
    under plain min-sum, batch 17, 2 iterations."""
    dec = context(name, max_batch=ST.SWEEP_BATCH)
    for k in (1,) + ST.FAMILIES_I8 + (0,):
        if take(dec, name, k):
            check_i8(dec, name, k, "u128", ST.SWEEP_BATCH, PD.CONTROL, ST.SWEEP_ITERS)
    for k in (1, ST.STAIRF, 0):
        if take(dec, name, k):
            check_f32(dec, name, k, ST.SWEEP_BATCH, "MS", ST.SWEEP_ITERS, monkeypatch)
    dec.close()


@pytest.mark.parametrize("iters", ST.ITERS)
@pytest.mark.parametrize("batch", ST.BATCHES)
@pytest.mark.parametrize("name", ST.CORE)
def test_core_grid(name, batch, iters, monkeypatch):
    """The core tables over inputs x parameters, at one batch and iteration
    count: every accepting family and the automatic choice; float under plain
    and offset min-sum."""
    dec = context(name)
    for k in (1,) + tuple(ST.families(name)) + (0,):
        dec.set_kernel(k)
        for params in ST.params_for(k):
            for kind in ST.INPUTS:
                if k == 0 and params in (ST.NMS_PARAMS, ST.WIDE_PARAMS):   # the fallback: test_dispatch_boundary
                    exp = ST.oracle_i8(name, kind, batch, params, iters)
                    got = run(dec, device_input(kind, batch, ST.table(name).n), iters, params.product(), extra=2)
                    assert_equal(got, exp, "%s %s %s automatic (%s)" % (name, kind, params.id, dec.last_kernel))
                    continue
                check_i8(dec, name, k, kind, batch, params, iters)
    for k in (1, ST.STAIRF, 0):
        if take(dec, name, k):
            for algo in sorted(ST.F32_ALGOS):
                check_f32(dec, name, k, batch, algo, iters, monkeypatch)
    dec.close()


@pytest.mark.parametrize("k", sorted(ST.ET_TABLES))
def test_early_termination(k):
    """One table per accepting family, on struct_domain.et_input (chosen by
    the oracle: some of the 65 codewords stop before the last iteration, some
    never): iterations used, soft and hard output equal the oracle's, for the
    family, generic and the automatic choice."""
    name = ST.ET_TABLES[k]
    llr = ST.et_input(name)
    dec = context(name)
    for kk in (k, 1, 0):
        assert take(dec, name, kk)
        exp = check_i8(dec, name, kk, "struct_et", ST.ET_BATCH, PD.CONTROL, ST.ET_ITERS, early=True, llr=llr,
                       d_llr=device(llr, ("et", name)))
        assert exp[2].min() < ST.ET_ITERS == exp[2].max()
    dec.close()


def test_coop_per_launch_early_termination(monkeypatch):
    """coop's per-launch variant (one launch per iteration and a syndrome
    pass) on a table with empty windows."""
    monkeypatch.setenv("LDPC_COOP_ET_KERNEL", "0")
    name = ST.COOP_PER_LAUNCH_ET
    llr = ST.et_input(name)
    dec = context(name)
    assert take(dec, name, 5)
    exp = check_i8(dec, name, 5, "struct_et", ST.ET_BATCH, PD.CONTROL, ST.ET_ITERS, early=True, llr=llr,
                   d_llr=device(llr, ("et", name)))
    assert exp[2].min() < ST.ET_ITERS == exp[2].max()
    dec.close()


@pytest.mark.parametrize("name", ST.ET_TABLES_F32)
def test_float_early_termination(name, monkeypatch):
    """stairf at every width the table has, generic and the automatic choice
    on the float early-termination input."""
    dec = context(name)
    for k in (ST.STAIRF, 1, 0):
        assert take(dec, name, k)
        exp = check_f32(dec, name, k, ST.ET_BATCH, "MS", ST.ET_ITERS, monkeypatch, early=True, et=True)
        assert exp[2].min() < ST.ET_ITERS == exp[2].max()
    dec.close()


@pytest.mark.parametrize("k", sorted(ST.NODE_MAJOR))
def test_node_major_entry(k):
    """decode_i8_nm_device, node-major [N][ld] with ld > batch (the columns
    beyond the batch hold junk), on a coop and a coop3 table."""
    name, batch, ld = ST.NODE_MAJOR[k], ST.SWEEP_BATCH, 50
    n = ST.table(name).n
    nm = np.full((n, ld), 77, dtype=np.int8)
    nm[:, :batch] = PD.make_input("u128", batch, n).T
    dec = context(name)
    assert take(dec, name, k)
    for params in (PD.CONTROL, ST.GRID_PARAMS[1]):
        check_i8(dec, name, k, "u128", batch, params, ST.SWEEP_ITERS, d_llr=_torch().from_numpy(nm).cuda(),
                 node_major=True)
    dec.close()


@pytest.mark.parametrize("params", PD.OUT_OF_DOMAIN, ids=lambda p: p.id)
def test_dispatch_boundary(params):
    """As test_gpu_param_domain.test_dispatch_boundary, on a synthetic table
    that coop3 accepts: outside the fast kernels' domain the automatic choice
    falls back, says which kernel it skipped and equals the oracle; coop3
    forced raises; default parameters afterwards run coop3 again."""
    name, batch = "x8_q5_h110", ST.SWEEP_BATCH
    d_llr = device_input("u128", batch, ST.table(name).n)
    dec = context(name)
    exp = ST.oracle_i8(name, "u128", batch, params, ST.SWEEP_ITERS)
    got = run(dec, d_llr, ST.SWEEP_ITERS, params.product(), extra=2)
    assert dec.last_kernel in ("windowed", "generic") and dec.last_skipped == "coop3"
    assert_equal(got, exp, "%s %s automatic (%s)" % (name, params.id, dec.last_kernel))
    dec.set_kernel(8)
    with pytest.raises(LdpcError) as e:
        run(dec, d_llr, ST.SWEEP_ITERS, params.product(), extra=2)
    assert e.value.status == _lib.LDPC_EUNSUPPORTED
    dec.set_kernel(0)
    run(dec, d_llr, ST.SWEEP_ITERS, PD.CONTROL.product(), extra=2)
    assert dec.last_kernel == "coop3" and dec.last_skipped is None
    dec.close()
