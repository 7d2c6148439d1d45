"""`ldsepw`, the edge-parallel float kernel of family 9 spread over several
waves (csrc/ldsepw.hip, behind the ep_wide switch), host side: the plan and the
automatic rule that ``ldpc_code_ep_wide_info`` reports without a GPU, and the
inputs tests/test_gpu_ep_wide.py decodes.

* of the shipped tables exactly 1248x624, 1944x972 and 2304x1152 qualify, with
  (layers, passes of 8 checks) = (11, 13), (12, 11), (11, 24) and the W their
  shapes are compiled for; 648x324 and 576x288 stay with the one-wave kernel;
* synthetic quasi-cyclic tables (ldsep_domain.synthetic, any Z) at the edges of
  the compiled shapes: the smallest Z the one-wave kernel does not take, full
  and ragged last passes, a last pass of one check, the largest Z, and one past it;
* the automatic rule, restated here, at the measured batches and between them;
* the early-termination inputs: at the Eb/N0 chosen per code the oracle alone
  stops the 9 codewords at two or more different iterations and leaves at least
  one running to the end -- the GPU test reuses them;
* the switch on a host context is LDPC_EUNSUPPORTED and stays off."""
import ctypes as C

import pytest

import float_domain as FD
import ldsep_domain as ED
import oracle as O
from ldpcgputegra_amd import Code, Decoder, LdpcError, _lib
from ldpcgputegra_amd.codes import available

# shipped tables that qualify: name -> (layers, passes, compiled W)
SHIPPED = {"1248x624": (11, 13, [2, 4]), "1944x972": (12, 11, [2, 4]), "2304x1152": (11, 24, [4])}
# synthetic tables: (block rows, Z) -> (passes, compiled W).  By the qualifying rule (some compiled shape of the
# layer count has W * NPW >= passes) Z = 105 runs on W = 2 as well: 11 x 7 on two waves holds its 14 passes.
SYNTHETIC = {(12, 33): (5, [2, 4]), (12, 88): (11, [2, 4]), (11, 49): (7, [2, 4]), (11, 100): (13, [2, 4]),
             (11, 105): (14, [2, 4]), (11, 192): (24, [4])}
DEGREES = (2, 5, 8)
# (layers, passes per wave, waves) compiled (csrc/ldsepw.hip kEpwShapes)
COMPILED = ((12, 6, 2), (12, 3, 4), (11, 7, 2), (11, 4, 4), (11, 6, 4))
MEASURED_BATCHES = (1024, 4096, 16384, 65536)
# early termination: Eb/N0 per code of the fine-grid input (float_domain.grid_input), 9 codewords, 16 iterations
ET_BATCH, ET_ITERS = 9, 16
ET_EBN0 = {"1944x972": 1.6, "1248x624": 1.6, "2304x1152": 1.6}


def info(code, batch=4096):
    return (code if isinstance(code, Code) else Code(code)).ep_wide_info(batch)


def mask_of(nl, np_):
    """the qualifying rule's third clause, restated: bit W set where a compiled (nl, NPW, W) has W * NPW >= passes"""
    m = 0
    for l, npw, w in COMPILED:
        if l == nl and w * npw >= np_:
            m |= 1 << w
    return m


def rule(nl, np_, mask, batch):
    """csrc/ldsepw.hip ldsepw_rule restated: (W launched at `batch`, whether the rule found it faster than family 7).
    Fitted to profiles/ep_wide_rate.json."""
    if not mask:
        return 0, False
    if not mask & 4:
        return 4, True
    return (4 if nl == 12 and batch > 2048 and mask & 16 else 2), True


def et_input(code):
    """float32 [9, N], read-only: the fine grid at ET_EBN0[code]"""
    return FD.grid_input(code, ET_BATCH, ET_EBN0[code], *FD.FINE)


def et_oracle(code, algo=O.OMS, beta=0.0):
    return FD.oracle_f32(code, ("ep_wide_et", ET_EBN0[code]), et_input(code), algo, beta, ET_ITERS, early=True)


def test_shipped_tables():
    names = available()
    assert len([n for n in names if not n.startswith("dvbs2")]) == 16
    assert any(n.startswith("dvbs2") for n in names)
    qualifying = {}
    for name in names:
        i = info(name)
        assert (i["waves_mask"] != 0) == bool(i["waves"])
        if i["waves"]:
            qualifying[name] = (i["n_layers"], i["n_passes"], i["waves"])
            assert i["waves_mask"] == mask_of(i["n_layers"], i["n_passes"]), name
        else:
            assert (i["n_layers"], i["n_passes"], i["waves_auto"]) == (0, 0, 0), name
    assert qualifying == SHIPPED
    for name in ("648x324", "576x288"):      # the one-wave kernel serves them: it stays
        assert info(name)["waves"] == [], name


@pytest.mark.parametrize("rows,Z", sorted(SYNTHETIC))
def test_synthetic_tables(rows, Z):
    np_, waves = SYNTHETIC[(rows, Z)]
    assert np_ == -(-Z // 8)
    for d in DEGREES:
        t = ED.synthetic(d, rows, Z)
        code = Code(t)
        assert (code.layer_info()["n_layers"], code.layer_info()["max_width"]) == (rows, Z)
        i = info(code)
        assert (i["n_layers"], i["n_passes"], i["waves"]) == (rows, np_, waves), (d, rows, Z, i)
        assert i["waves_mask"] == mask_of(rows, np_)


def test_tables_that_do_not_qualify():
    assert info(Code(ED.synthetic(5, 11, 193)))["waves"] == []          # 25 passes: past 4 x 6
    assert info(Code(ED.synthetic(5, 12, 97)))["waves"] == []           # 12 layers hold 12 passes
    assert info(Code(ED.synthetic(5, 12, 32)))["waves"] == []           # the one-wave kernel's 12 x 4
    assert info(Code(ED.synthetic(5, 11, 48)))["waves"] == []           # ... and its 11 x 6
    assert info(Code(ED.synthetic(5, 12, 33)))["waves"] == [2, 4]       # the smallest Z it does not take
    assert info(Code(ED.synthetic(5, 10, 88)))["waves"] == []           # 10 layers: no compiled shape
    L = _lib.lib()
    assert L.ldpc_code_ep_wide_info(None, 1, None, None, None, None) == _lib.LDPC_EINVAL
    assert L.ldpc_code_ep_wide_info(Code("1944x972").handle, -1, None, None, None, None) == _lib.LDPC_EINVAL
    assert L.ldpc_code_ep_wide_info(Code("1944x972").handle, 1, None, None, None, None) == _lib.LDPC_OK


def test_rule_is_the_restated_one():
    batches = sorted(set(MEASURED_BATCHES) | {1, 2, 512, 1023, 1025, 2048, 2049, 3000, 4095, 4097, 8192, 10000, 16383,
                                              16385, 32768, 50000, 65535, 65537, 1 << 20})
    codes = [Code(n) for n in SHIPPED] + [Code(ED.synthetic(5, r, z)) for r, z in sorted(SYNTHETIC)]
    for code in codes:
        for b in batches:
            i = info(code, b)
            w, beats = rule(i["n_layers"], i["n_passes"], i["waves_mask"], b)
            assert w in i["waves"]
            assert i["waves_auto"] == (w if beats else 0), (code.name, code.n, b, i)
    for name in ("648x324", "200x100", "dvbs2_r1_2"):
        assert all(info(name, b)["waves_auto"] == 0 for b in batches)


@pytest.mark.parametrize("code", sorted(ET_EBN0))
def test_early_termination_inputs(code):
    its = et_oracle(code)[2]
    print("%s at %.2f dB: iterations used %s" % (code, ET_EBN0[code], its.tolist()))
    assert its.shape == (ET_BATCH,)
    assert len(set(its.tolist())) >= 2, "at least two distinct iterations used"
    assert (its == ET_ITERS).any(), "at least one codeword never stops"
    assert (its < ET_ITERS).any()


def test_switch_on_a_host_context():
    dec = Decoder(Code("1944x972"), device=-1, max_batch=4)
    assert dec.ep_wide is False and dec.last_ep_waves == 0
    for flag in (True, False):
        with pytest.raises(LdpcError) as e:
            dec.set_ep_wide(flag)
        assert e.value.status == _lib.LDPC_EUNSUPPORTED
        assert dec.ep_wide is False
    dec.close()
    with pytest.raises(LdpcError) as e:
        Decoder(Code("1944x972"), device=-1, max_batch=4, ep_wide=True)
    assert e.value.status == _lib.LDPC_EUNSUPPORTED
    L = _lib.lib()
    on = C.c_int(5)
    assert L.ldpc_ctx_set_ep_wide(None, 1) == _lib.LDPC_EINVAL
    assert L.ldpc_ctx_get_ep_wide(None, C.byref(on)) == _lib.LDPC_EINVAL and on.value == 5
    assert L.ldpc_ctx_last_ep_waves(None, C.byref(on)) == _lib.LDPC_EINVAL and on.value == 5
