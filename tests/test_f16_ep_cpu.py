"""The edge-parallel binary16 kernel (`ldseph`, family 9 of the f16 decode),
host side: what tests/test_gpu_f16_ep.py rests on.

* ldsep_domain's synthetic tables have the layer plan the kernel's two compiled
  shapes need: 12 or 11 layers of Z checks;
* the host decoder (``ldpc_decode_f16_soft``), the yardstick of the GPU file,
  equals the numpy restatement f16_ref.decode bit for bit on a sample of them;
* the early-termination input of the GPU file holds what its test needs: a pair
  (stops, never), a pair (never, stops), pairs whose halves stop at different
  iterations, a lone last half that stops -- asserted on the restatement alone;
* the f16_edge_parallel switch on a host context is LDPC_EUNSUPPORTED and stays
  off."""
import ctypes as C

import numpy as np
import pytest

import f16_ref as R
import ldsep_domain as ED
import test_f16_short_cpu as SC
from ldpcgputegra_amd import ALGO_MS, ALGO_NMS, ALGO_OMS, Code, Decoder, LdpcError, _lib, default_params, load_table

ALGO = {"MS": (ALGO_MS, 0.0), "OMS": (ALGO_OMS, 0.375), "NMS": (ALGO_NMS, 0.8125)}
BATCH, ITERS = 5, 3
ET_CODE, ET_BATCH, ET_ITERS = "648x324", SC.ET_BATCH, SC.ET_ITERS
ET_REPLACED = (1, 4)          # codewords that never converge: rows of f16_ref.make_input
ET_ITERS_USED = [7, 16, 3, 6, 16, 10, 9, 5, 6, 8, 4, 7, 3, 8, 12, 5, 6]
_et = []


def et_input():
    """uint16 bit patterns [17, 648], read-only: test_f16_short_cpu.et_input("648x324") with codewords 1 and 4
    replaced by rows 1 and 4 of f16_ref.make_input(17, 648), which never satisfy the checks"""
    if not _et:
        x = np.array(SC.et_input(ET_CODE))
        noise = R.make_input(ET_BATCH, x.shape[1])
        for b in ET_REPLACED:
            x[b] = noise[b]
        x.setflags(write=False)
        _et.append(x)
    return _et[0]


@pytest.mark.parametrize("d,rows,Z", ED.ALL, ids=[ED.synthetic_name(*k) for k in ED.ALL])
def test_layer_plan(d, rows, Z):
    t = ED.synthetic(d, rows, Z)
    assert t.n == 24 * Z and t.m == rows * Z
    code = Code(t)
    nl, mw, i8, f32 = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    _lib.check(_lib.lib().ldpc_code_layer_info(code.handle,C.byref(nl), C.byref(mw), C.byref(i8), C.byref(f32)))
    assert (nl.value, mw.value) == (rows, Z)


@pytest.mark.parametrize("rows,Z", ED.SHAPES, ids=["r%d_z%d" % s for s in ED.SHAPES])
@pytest.mark.parametrize("d", (2, 3, 7, 8))
def test_host_equals_restatement(d, rows, Z):
    t = ED.synthetic(d, rows, Z)
    x = R.make_input(BATCH, t.n)
    dec = Decoder(Code(t), device=-1, max_batch=BATCH)
    for algo in sorted(ALGO):
        a, beta = ALGO[algo]
        hard, soft, its = dec.decode_f16_soft(x, ITERS, default_params(algo=a, beta=beta))
        exp = R.decode(t, x, ITERS, algo, beta)
        assert np.array_equal(hard, exp[0]), (d, rows, Z, algo)
        assert np.array_equal(np.asarray(soft).view(np.uint16), exp[1]), (d, rows, Z, algo)
        assert np.array_equal(its, exp[2]), (d, rows, Z, algo)
    dec.close()


def test_early_termination_input():
    its = R.decode(load_table(ET_CODE), et_input(), ET_ITERS, "MS", 0.0, True)[2]
    assert its.tolist() == ET_ITERS_USED
    pairs = [(int(its[2 * p]), int(its[2 * p + 1])) for p in range(ET_BATCH // 2)]
    assert pairs[0][0] < ET_ITERS and pairs[0][1] == ET_ITERS, "pair 0: (stops, never)"
    assert pairs[2][0] == ET_ITERS and pairs[2][1] < ET_ITERS, "pair 2: (never, stops)"
    assert all(a != b for a, b in pairs), "every pair's halves stop at different iterations"
    assert its[ET_BATCH - 1] == 6, "the lone last half stops"


def test_switch_on_a_host_context():
    dec = Decoder(Code("648x324"), device=-1, max_batch=4)
    assert dec.f16_edge_parallel is False
    for flag in (True, False):
        with pytest.raises(LdpcError) as e:
            dec.set_f16_edge_parallel(flag)
        assert e.value.status == _lib.LDPC_EUNSUPPORTED
        assert dec.f16_edge_parallel is False
    dec.close()
    with pytest.raises(LdpcError) as e:
        Decoder(Code("648x324"), device=-1, max_batch=4, f16_edge_parallel=True)
    assert e.value.status == _lib.LDPC_EUNSUPPORTED
    L = _lib.lib()
    on = C.c_int(5)
    assert L.ldpc_ctx_set_f16_edge_parallel(None, 1) == _lib.LDPC_EINVAL
    assert L.ldpc_ctx_get_f16_edge_parallel(None, C.byref(on)) == _lib.LDPC_EINVAL and on.value == 5
