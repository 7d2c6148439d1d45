"""Layered belief propagation (LDPC_ALGO_BP) on the GPU: the box-plus kernel
and both decode kernels of csrc/bp.hip -- the LDS-resident one (family 7) and
the any-H one (family 1) -- against the host decoder (device = -1), bit for
bit on hard decisions, soft output and iterations used.  test_bp_cpu.py holds
the host decoder to the definition and the box-plus to float64.

Shapes: batch 37 leaves the last wave of family 1 (64 codewords) partly empty
and, where family 7 packs codewords into a wave (648x324: two, 200x100: four),
codeword groups of the last wave empty; batch 5 is less than one wave of family 1.  Batch 37
decodes unrounded channel LLRs, batch 5 float_domain's grid with its zeros and
-0.0.  The synthetic tables cover the degree dispatch and the register arrays
(2, 3, 17 and 32, with 2, 2, 16 and 31 in their second group), the DVB-S2
tables the staircase and degrees 7 / 6 and 30 / 29 at N = 64800."""
import numpy as np
import pytest

import bp_ref as R
import float_domain as FD
import short_domain as SD
from ldpcgputegra_amd import ALGO_BP, ALGO_MS, Code, Decoder, LdpcError, _lib, boxplus_host, default_params, load_table
from test_bp_cpu import ET_ITERS, awgn_llr, grid_llr, host, table_of, u32

pytestmark = pytest.mark.gpu

# families per code, pinned (test_families_match_the_codes), and what the automatic choice takes for BP
FAMILIES = {"648x324": [1, 7, 0], "576x288": [1, 7, 0], "1944x972": [1, 7, 0], "200x100": [1, 7, 0]}
AUTO = {"648x324": "lds", "576x288": "lds", "1944x972": "lds", "200x100": "generic"}
SYNTH = [2, 3, 17, 32]
DVBS2 = ["dvbs2_r1_2", "dvbs2_r9_10"]
NAMES = {1: "generic", 7: "lds"}
_decoders = {}
_refs = {}


def _torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def decoder(name, kernel):
    key = (name, kernel)
    if key not in _decoders:
        _decoders[key] = Decoder(Code(table_of(name) if isinstance(name, int) else name), max_batch=64, kernel=kernel)
    return _decoders[key]


def bp(early=False):
    return default_params(algo=ALGO_BP, early_term=int(early))


def reference(name, kind, batch, iters, early=False):
    """(llr, (hard, soft, iters_used)) of the host decoder, cached."""
    key = (name, kind, batch, iters, early)
    if key not in _refs:
        llr = grid_llr(name, batch) if kind == "grid" else awgn_llr(name, batch, None if name in FD.EBN0 else 2.0)
        _refs[key] = (llr, host(name).decode_f32_soft(llr, iters, bp(early)))
    return _refs[key]


def run(dec, llr, iters, params, rows=None):
    """(hard, soft, iters_used) of one device decode; `rows`: rows of the output buffers (default: the batch)."""
    torch = _torch()
    B, n = llr.shape
    rows = rows or B
    d_llr = torch.from_numpy(np.array(llr)).cuda()
    d_hard = torch.full((rows, n), 9, dtype=torch.uint8, device="cuda")
    d_soft = torch.full((rows, n), 99.0, dtype=torch.float32, device="cuda")
    d_its = torch.full((rows,), -7, dtype=torch.int32, device="cuda")
    dec.decode_f32_device(d_llr, d_hard, iters, params=params, soft=d_soft, iters_used=d_its)
    torch.cuda.synchronize()
    return d_hard.cpu().numpy(), d_soft.cpu().numpy(), d_its.cpu().numpy()


def assert_same(got, exp, where):
    (hard, soft, its), (eh, es, eit) = got, exp
    diff = u32(soft) != u32(es)
    assert not diff.any(), "%s: %d soft values differ from the host decoder, the first at %s: %r, expected %r" % (
        where, int(diff.sum()), tuple(np.argwhere(diff)[0]), soft[diff][0], es[diff][0])
    assert np.array_equal(hard, eh), "%s: %d hard decisions differ" % (where, int((hard != eh).sum()))
    assert np.array_equal(its, eit), "%s: iterations used %s, expected %s" % (where, its.tolist(), eit.tolist())


def check_family(dec, kernel, name):
    if kernel:
        assert dec.last_kernel == NAMES[kernel]
    else:
        assert dec.last_kernel == AUTO[name]
    if dec.last_kernel == "lds":   # one lane per check, never two: the lane group of the widest layer
        w = SD.LAYER_PLAN[name][1]
        assert dec.last_lds_shape == (8 if w <= 8 else 16 if w <= 16 else 32 if w <= 32 else 64, False)
    else:
        assert dec.last_lds_shape == (0, False)


def test_families_match_the_codes():
    """Family 7 fits every short code of the table (ldpc_code_layer_info's
    lds_f32), and the automatic choice for BP is min-sum's for int8
    (short_domain.AUTO: lds where it fits and is preferred, else generic)."""
    for name in FAMILIES:
        info = Code(name).layer_info()
        assert info["lds_f32"] and (info["n_layers"], info["max_width"]) == SD.LAYER_PLAN[name]
        assert AUTO[name] == SD.AUTO[name]


def test_boxplus_device_is_the_hosts():
    torch = _torch()
    a, b = R.pairs()
    d_a, d_b = torch.from_numpy(np.array(a)).cuda(), torch.from_numpy(np.array(b)).cuda()
    d_out = torch.full((a.size,), 99.0, dtype=torch.float32, device="cuda")
    dec = decoder("200x100", 0)
    dec.boxplus_device(d_a, d_b, d_out)               # the whole input set in one launch
    torch.cuda.synchronize()
    got, exp = d_out.cpu().numpy(), boxplus_host(a, b)
    diff = u32(got) != u32(exp)
    assert not diff.any(), "%d of %d differ, the first at %d: (%r, %r) -> %r, host %r" % (
        int(diff.sum()), a.size, int(np.argmax(diff)), a[diff][0], b[diff][0], got[diff][0], exp[diff][0])
    # count 0 touches nothing
    dec.boxplus_device(d_a[:0], d_b[:0], d_out[:0])
    L = _lib.lib()
    assert L.ldpc_boxplus_f32_async(dec._ctx, None, None, d_b.data_ptr(), d_out.data_ptr(), 4) == _lib.LDPC_EINVAL


@pytest.mark.parametrize("iters", [1, 3])
@pytest.mark.parametrize("batch", [37, 5])
@pytest.mark.parametrize("name,kernel", [(c, k) for c in FAMILIES for k in FAMILIES[c]])
def test_decode_is_the_host_decoders(name, kernel, batch, iters):
    llr, exp = reference(name, "awgn" if batch == 37 else "grid", batch, iters)
    dec = decoder(name, kernel)
    assert_same(run(dec, llr, iters, bp()), exp, "%s kernel %d batch %d" % (name, kernel, batch))
    check_family(dec, kernel, name)


@pytest.mark.parametrize("name,kernel", [(c, k) for c in FAMILIES for k in FAMILIES[c]])
def test_early_termination(name, kernel):
    """16 iterations at float_domain.EBN0; iters_used of the 5 codewords, from the host decoder:
    648x324 [5 7 4 4 4]   576x288 [5 16 6 4 4]   200x100 [5 3 3 16 6]   1944x972: two values below 16 (asserted)."""
    llr, exp = reference(name, "awgn", 5, ET_ITERS, early=True)
    assert len(set(int(u) for u in exp[2] if u < ET_ITERS)) >= 2, exp[2]
    dec = decoder(name, kernel)
    assert_same(run(dec, llr, ET_ITERS, bp(early=True)), exp, "%s kernel %d early" % (name, kernel))
    check_family(dec, kernel, name)


@pytest.mark.parametrize("kernel", [1, 7])
@pytest.mark.parametrize("d", SYNTH)
def test_synthetic_degrees(d, kernel):
    llr, exp = reference(d, "awgn", 5, 2)
    dec = decoder(d, kernel)
    assert_same(run(dec, llr, 2, bp()), exp, "synthetic d = %d kernel %d" % (d, kernel))
    assert dec.last_kernel == NAMES[kernel]


@pytest.mark.parametrize("name", DVBS2)
def test_dvbs2_on_the_any_h_kernel(name):
    llr, exp = reference(name, "awgn", 5, 2)
    dec = decoder(name, 1)
    assert_same(run(dec, llr, 2, bp()), exp, name)
    assert dec.last_kernel == "generic"


# ---- selection -------------------------------------------------------------

@pytest.mark.parametrize("name,kernel,family", [("648x324", 9, "ldsep"), ("dvbs2_r1_2", 11, "stairf")])
def test_fast_float_families_refuse_bp(name, kernel, family):
    """A forced family without BP is LDPC_EUNSUPPORTED and stays selected: the
    next min-sum decode runs on it.  The automatic choice passes it over and
    says so (last_skipped)."""
    torch = _torch()
    t = load_table(name)
    llr, exp = reference(name, "awgn", 5, 1)
    dec = Decoder(Code(name), max_batch=64, kernel=kernel)
    d_llr = torch.from_numpy(np.array(llr)).cuda()
    d_hard = torch.full((5, t.n), 9, dtype=torch.uint8, device="cuda")
    with pytest.raises(LdpcError) as e:
        dec.decode_f32_device(d_llr, d_hard, 1, params=bp())
    assert e.value.status == _lib.LDPC_EUNSUPPORTED
    torch.cuda.synchronize()
    assert (d_hard.cpu().numpy() == 9).all() and dec.kernel == kernel
    dec.decode_f32_device(d_llr, d_hard, 1, params=default_params(algo=ALGO_MS))
    torch.cuda.synchronize()
    assert dec.last_kernel == family and dec.last_skipped is None
    assert np.array_equal(d_hard.cpu().numpy(), host(name).decode_f32(llr, 1, default_params(algo=ALGO_MS)))
    dec.set_kernel(0)
    assert_same(run(dec, llr, 1, bp()), exp, "%s auto" % name)
    assert dec.last_skipped == family and dec.last_kernel == ("lds" if name == "648x324" else "generic")
    dec.close()


@pytest.mark.parametrize("kernel", [2, 3, 5, 8])
def test_int8_families_refuse_bp(kernel):
    dec = Decoder(Code("dvbs2_r1_2"), max_batch=64, kernel=kernel)
    llr, _ = reference("dvbs2_r1_2", "awgn", 5, 1)
    with pytest.raises(LdpcError) as e:
        run(dec, llr, 1, bp())
    assert e.value.status == _lib.LDPC_EUNSUPPORTED and dec.kernel == kernel
    dec.close()


def test_int8_bp_is_unsupported_on_the_device():
    torch = _torch()
    dec = decoder("200x100", 0)
    d_llr = torch.zeros((2, 200), dtype=torch.int8, device="cuda")
    d_hard = torch.zeros((2, 200), dtype=torch.uint8, device="cuda")
    with pytest.raises(LdpcError) as e:
        dec.decode_i8_device(d_llr, d_hard, 1, params=bp())
    assert e.value.status == _lib.LDPC_EUNSUPPORTED


# ---- buffers, count, host buffers ------------------------------------------

@pytest.mark.parametrize("kernel", [1, 7])
def test_rows_beyond_the_batch_are_untouched(kernel):
    llr, exp = reference("648x324", "grid", 5, 3)
    hard, soft, its = run(decoder("648x324", kernel), llr, 3, bp(), rows=7)
    assert_same((hard[:5], soft[:5], its[:5]), exp, "kernel %d" % kernel)
    assert (hard[5:] == 9).all() and (soft[5:] == 99.0).all() and (its[5:] == -7).all()


@pytest.mark.parametrize("kernel", [1, 7])
def test_counting_decode(kernel):
    """ldpc_decode_f32_count_async with BP counts what a decode followed by
    ldpc_count_errors_async counts (1 iteration at 2.0 dB leaves errors)."""
    torch = _torch()
    llr, exp = reference("648x324", "awgn", 37, 1)
    dec = decoder("648x324", kernel)
    k = dec.code.k_info
    d_llr = torch.from_numpy(np.array(llr)).cuda()
    d_hard = torch.zeros((37, 648), dtype=torch.uint8, device="cuda")
    d_cnt = torch.zeros(4, dtype=torch.int64, device="cuda")
    dec.decode_count_device(d_llr, d_hard, 1, k, d_cnt[:2], params=bp())
    d_hard2 = torch.zeros_like(d_hard)
    dec.decode_f32_device(d_llr, d_hard2, 1, params=bp())
    dec.count_errors_device(d_hard2, k, d_cnt[2:])
    torch.cuda.synchronize()
    cnt = d_cnt.cpu().numpy()
    assert np.array_equal(d_hard.cpu().numpy(), exp[0]) and np.array_equal(d_hard2.cpu().numpy(), exp[0])
    assert cnt[0] == cnt[2] == int(exp[0][:, :k].sum()) and cnt[1] == cnt[3] == int(exp[0][:, :k].any(axis=1).sum())
    assert cnt[1] > 0


def test_host_buffer_entry_point():
    llr, exp = reference("648x324", "awgn", 37, 3)
    dec = decoder("648x324", 0)
    assert np.array_equal(dec.decode_f32(llr, 3, bp()), exp[0])
    assert dec.last_kernel == "lds"
