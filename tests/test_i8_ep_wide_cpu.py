"""`ldsepwi`, the edge-parallel int8 kernel of family 9 spread over several waves
(csrc/ldsepwi.hip, behind the i8_ep_wide switch), host side: what
tests/test_gpu_i8_ep_wide.py rests on.

* the three exports, and the switch on a host context: LDPC_EUNSUPPORTED, stays off;
* ``ldpc_code_i8_ep_wide_info`` on every shipped table: exactly 1248x624,
  1944x972 and 2304x1152 qualify, and the mask is the int8 shape list's,
  restated here; on the synthetic tables of test_ep_wide_cpu and on those that
  do not qualify;
* the automatic rule, restated here, over test_ep_wide_cpu's batch list;
* the host int8 decoder equals the oracle on the synthetic tables at check
  degrees 2, 5 and 8 over the parameter sets the GPU file uses (hard decisions:
  all the host int8 entry point returns), so a GPU mismatch is a kernel bug;
* the early-termination inputs: per shipped code 9 codewords at an Eb/N0 and a
  seed at which the oracle alone, at 16 iterations and under each of the three
  algorithms, shows a pair (stops, runs to the end), a pair (runs to the end,
  stops), a pair whose halves stop at different iterations, neighbouring pairs
  that stop at different iterations, and a lone ninth codeword that stops."""
import ctypes as C
import os

import numpy as np
import pytest

import ldsep_domain as ED
import param_domain as PD
import test_ep_wide_cpu as EW
from ldpcgputegra_amd import Code, Decoder, LdpcError, _lib, channel, load_table
from ldpcgputegra_amd.codes import available

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))

# (layers, passes per wave, waves) compiled in int8 (csrc/ldsepwi.hip kEpwiShapes): every entry of the float list
# fits the 256-register budget without scratch, so none was dropped
COMPILED = ((12, 6, 2), (12, 3, 4), (11, 7, 2), (11, 4, 4), (11, 6, 4))
# shipped tables that qualify: name -> (layers, passes, compiled W)
SHIPPED = {"1248x624": (11, 13, [2, 4]), "1944x972": (12, 11, [2, 4]), "2304x1152": (11, 24, [4])}
SYNTHETIC = dict(EW.SYNTHETIC)      # (block rows, Z) -> (passes, compiled W): the float plan's tables, the int8 mask
DEGREES = (2, 5, 8)

BASIC = [PD.Params("OMS", 1, -127, 31), PD.Params("MS", 0, -127, 31), PD.Params("NMS", 26, -127, 31)]
# the parameter corners of tests/test_gpu_i8_ep.py: var_min -64 and 0, msg_max 0 and 127, offset 255, a large factor
CORNERS = [PD.Params("OMS", 63, -127, 63), PD.Params("OMS", 5, -127, 0), PD.Params("OMS", 3, -127, 127),
           PD.Params("OMS", 255, -127, 127), PD.Params("NMS", 64, -127, 63), PD.Params("NMS", 255, -127, 127),
           PD.Params("OMS", 1, -64, 31), PD.Params("OMS", 1, 0, 31)]
CORNER_TABLES = ((12, 88), (11, 105))
SYN_BATCH, SYN_ITERS = 5, 3

# early termination: 9 codewords of channel.awgn_i8_host at (Eb/N0, seed), 16 iterations; found by a search over
# seeds with the oracle, kept because all of test_early_termination_inputs' conditions hold under OMS 1, MS and NMS 26
ET_BATCH, ET_ITERS = 9, 16
ET_POINT = {"1944x972": (1.5, 35), "1248x624": (1.6, 89), "2304x1152": (1.6, 111)}
ET_PARAMS = {"OMS": BASIC[0], "MS": BASIC[1], "NMS": BASIC[2]}
ET_ITERS_USED = {
    "1944x972": {"OMS": [10, 16, 10, 8, 16, 15, 6, 7, 6], "MS": [14, 16, 16, 11, 16, 16, 8, 13, 7],
                 "NMS": [14, 16, 16, 8, 16, 16, 7, 9, 8]},
    "1248x624": {"OMS": [16, 6, 14, 8, 7, 16, 6, 7, 6], "MS": [16, 7, 16, 14, 10, 16, 8, 7, 6],
                 "NMS": [16, 6, 15, 10, 7, 16, 6, 7, 6]},
    "2304x1152": {"OMS": [7, 16, 7, 7, 8, 9, 16, 6, 7], "MS": [9, 16, 12, 10, 16, 16, 16, 8, 13],
                  "NMS": [8, 16, 10, 8, 11, 10, 16, 7, 9]},
}
_et = {}


def info(code, batch=4096):
    return (code if isinstance(code, Code) else Code(code)).i8_ep_wide_info(batch)


def mask_of(nl, np_):
    """bit W set where a compiled int8 (nl, NPW, W) has W * NPW >= passes"""
    m = 0
    for l, npw, w in COMPILED:
        if l == nl and w * npw >= np_:
            m |= 1 << w
    return m


def rule(nl, np_, mask, batch):
    """csrc/ldsepwi.hip ldsepwi_rule restated: (W launched at `batch`, whether the rule found it ahead of family 7).
    Fitted to profiles/i8_ep_wide_rate.json."""
    if not mask:
        return 0, False
    if not mask & 4:
        return 4, True
    if not mask & 16:
        return 2, True
    return (4 if nl == 12 or batch <= 8192 else 2), True


def et_input(code):
    """int8 [9, N], read-only: AWGN LLRs of `code` at ET_POINT[code]"""
    if code not in _et:
        t = load_table(code)
        ebn0, seed = ET_POINT[code]
        x = channel.awgn_i8_host(t.n, ET_BATCH, seed=seed, table=channel.i8_table(channel.sigma_from_ebn0(ebn0, t.k_info / t.n)))
        x.setflags(write=False)
        _et[code] = x
    return _et[code]


def et_oracle(code, algo):
    return PD.oracle_decode(code, ("i8epw_et",) + ET_POINT[code], et_input(code), ET_PARAMS[algo], ET_ITERS, early=True)


# ---- exports and the switch ---------------------------------------------------------

def test_exports():
    L = _lib.lib()
    for name in ("ldpc_ctx_set_i8_ep_wide", "ldpc_ctx_get_i8_ep_wide", "ldpc_code_i8_ep_wide_info"):
        assert name in _lib.SIGNATURES and hasattr(L, name), name
    with open(os.path.join(ROOT, "include", "ldpc_mi355x.h")) as f:
        header = f.read()
    assert "int ldpc_ctx_set_i8_ep_wide(ldpc_ctx *ctx, int enable);" in header
    assert "int ldpc_ctx_get_i8_ep_wide(ldpc_ctx *ctx, int *enable);" in header
    assert "int ldpc_code_i8_ep_wide_info(const ldpc_code *h, int batch, int *n_layers, int *n_passes, int *waves_mask," \
        in header
    with open(os.path.join(ROOT, "include", "ldpc_mi355x.hpp")) as f:
        hpp = f.read()
    assert "setI8EpWide" in hpp and "i8EpWide" in hpp


def test_switch_on_a_host_context():
    dec = Decoder(Code("1944x972"), device=-1, max_batch=4)
    assert dec.i8_ep_wide is False and dec.last_ep_waves == 0
    for flag in (True, False):
        with pytest.raises(LdpcError) as e:
            dec.set_i8_ep_wide(flag)
        assert e.value.status == _lib.LDPC_EUNSUPPORTED
        assert dec.i8_ep_wide is False
    dec.close()
    with pytest.raises(LdpcError) as e:
        Decoder(Code("1944x972"), device=-1, max_batch=4, i8_ep_wide=True)
    assert e.value.status == _lib.LDPC_EUNSUPPORTED
    L = _lib.lib()
    on = C.c_int(5)
    assert L.ldpc_ctx_set_i8_ep_wide(None, 1) == _lib.LDPC_EINVAL
    assert L.ldpc_ctx_get_i8_ep_wide(None, C.byref(on)) == _lib.LDPC_EINVAL and on.value == 5


# ---- the plan -----------------------------------------------------------------------

def test_shipped_tables():
    qualifying = {}
    for name in available():
        i = info(name)
        assert (i["waves_mask"] != 0) == bool(i["waves"])
        if i["waves"]:
            qualifying[name] = (i["n_layers"], i["n_passes"], i["waves"])
            assert i["waves_mask"] == mask_of(i["n_layers"], i["n_passes"]), name
            f = Code(name).ep_wide_info(4096)      # the float plan: the same layers and passes
            assert (f["n_layers"], f["n_passes"]) == (i["n_layers"], i["n_passes"]), name
        else:
            assert (i["n_layers"], i["n_passes"], i["waves_auto"]) == (0, 0, 0), name
    assert qualifying == SHIPPED
    for name in ("648x324", "576x288", "200x100", "dvbs2_r1_2"):
        assert info(name)["waves"] == [], name


@pytest.mark.parametrize("rows,Z", sorted(SYNTHETIC))
def test_synthetic_tables(rows, Z):
    np_ = SYNTHETIC[(rows, Z)][0]
    for d in DEGREES:
        i = info(Code(ED.synthetic(d, rows, Z)))
        assert (i["n_layers"], i["n_passes"]) == (rows, np_), (d, rows, Z, i)
        assert i["waves_mask"] == mask_of(rows, np_) and i["waves"] == SYNTHETIC[(rows, Z)][1]


def test_tables_that_do_not_qualify():
    assert info(Code(ED.synthetic(5, 11, 193)))["waves"] == []          # 25 passes: past 4 x 6
    assert info(Code(ED.synthetic(5, 12, 97)))["waves"] == []           # 12 layers hold 12 passes
    assert info(Code(ED.synthetic(5, 12, 32)))["waves"] == []           # the one-wave kernel's 12 x 4
    assert info(Code(ED.synthetic(5, 11, 48)))["waves"] == []           # ... and its 11 x 6
    assert info(Code(ED.synthetic(5, 12, 33)))["waves"] == [2, 4]       # the smallest Z it does not take
    assert info(Code(ED.synthetic(5, 10, 88)))["waves"] == []           # 10 layers: no compiled shape
    L = _lib.lib()
    assert L.ldpc_code_i8_ep_wide_info(None, 1, None, None, None, None) == _lib.LDPC_EINVAL
    assert L.ldpc_code_i8_ep_wide_info(Code("1944x972").handle, -1, None, None, None, None) == _lib.LDPC_EINVAL
    assert L.ldpc_code_i8_ep_wide_info(Code("1944x972").handle, 1, None, None, None, None) == _lib.LDPC_OK


def test_rule_is_the_restated_one():
    batches = sorted(set(EW.MEASURED_BATCHES) | {1, 2, 512, 1023, 1025, 2048, 2049, 3000, 4095, 4097, 8192, 10000,
                                                 16383, 16385, 32768, 50000, 65535, 65537, 1 << 20})
    codes = [Code(n) for n in SHIPPED] + [Code(ED.synthetic(5, r, z)) for r, z in sorted(SYNTHETIC)]
    for code in codes:
        for b in batches:
            i = info(code, b)
            w, beats = rule(i["n_layers"], i["n_passes"], i["waves_mask"], b)
            assert w in i["waves"]
            assert i["waves_auto"] == (w if beats else 0), (code.name, code.n, b, i)
    for name in ("648x324", "200x100", "dvbs2_r1_2"):
        assert all(info(name, b)["waves_auto"] == 0 for b in batches)


# ---- host decoder and oracle on the GPU file's tables and parameters ----------------

@pytest.mark.parametrize("rows,Z", sorted(SYNTHETIC))
def test_host_equals_oracle(rows, Z):
    for d in DEGREES:
        t = ED.synthetic(d, rows, Z)
        name = ED.synthetic_name(d, rows, Z)
        dec = Decoder(Code(t), device=-1, max_batch=SYN_BATCH)
        cases = [("u128", p) for p in BASIC]
        if (rows, Z) in CORNER_TABLES:
            cases += [(kind, p) for kind in ("ext", "ties") for p in CORNERS]
        for kind, p in cases:
            x = PD.make_input(kind, SYN_BATCH, t.n)
            exp = PD.oracle_decode(name, (kind, SYN_BATCH), x, p, SYN_ITERS, table=t)
            got = dec.decode_i8(x, SYN_ITERS, p.product())
            assert np.array_equal(got, exp[0]), (name, kind, p.id)
        dec.close()


# ---- the early-termination inputs ---------------------------------------------------

@pytest.mark.parametrize("algo", sorted(ET_PARAMS))
@pytest.mark.parametrize("code", sorted(ET_POINT))
def test_early_termination_inputs(code, algo):
    its = et_oracle(code, algo)[2]
    print("%s %s at %.2f dB, seed %d: iterations used %s" % ((code, algo) + ET_POINT[code] + (its.tolist(),)))
    assert its.tolist() == ET_ITERS_USED[code][algo]
    pr = [(int(its[2 * k]), int(its[2 * k + 1])) for k in range(ET_BATCH // 2)]
    assert any(a < ET_ITERS and b == ET_ITERS for a, b in pr), "a pair (stops, runs to the end)"
    assert any(a == ET_ITERS and b < ET_ITERS for a, b in pr), "a pair (runs to the end, stops)"
    assert any(a < ET_ITERS and b < ET_ITERS and a != b for a, b in pr), "a pair whose halves stop apart"
    # the iteration at which a pair's last stopping half stops (None: neither stops)
    last = [max([v for v in p if v < ET_ITERS], default=None) for p in pr]
    assert any(a is not None and b is not None and a != b for a, b in zip(last, last[1:])), \
        "neighbouring pairs that stop at different iterations"
    assert its[ET_BATCH - 1] < ET_ITERS, "the lone ninth codeword stops"
