"""The binary16 decode of the codes without a staircase, host side: what
tests/test_gpu_f16_short.py rests on.

* the host decoder (``ldpc_decode_f16_soft``), the yardstick of the GPU file,
  equals the numpy restatement f16_ref.decode bit for bit on the tables that
  file uses and test_f16_cpu.py does not cover: 200x100, 1024x518 (two degree
  groups), 2048x384 (its pairs do not fit LDS), and the synthetic tables of
  short_domain at check degrees 2, 3, 7, 17, 31, 32 (Z = 12 and 40);
* the early-termination inputs of the GPU file hold what its tests need: pairs
  of codewords (2p, 2p + 1) whose halves stop apart, pairs where one half never
  stops, pairs that never stop, a lone last codeword -- asserted on the
  restatement alone;
* the f16_all_codes switch: get / set / get on a host context, off by default."""
import ctypes as C

import numpy as np
import pytest

import f16_ref as R
import float_domain as FD
import short_domain as SD
from ldpcgputegra_amd import ALGO_MS, ALGO_NMS, ALGO_OMS, Code, Decoder, _lib, default_params, load_table

ALGO = {"MS": (ALGO_MS, 0.0), "OMS": (ALGO_OMS, 0.375), "NMS": (ALGO_NMS, 0.8125)}
SHIPPED = ("200x100", "1024x518", "2048x384")
SYNTH = [(d, Z) for d in (2, 3, 7, 17, 31, 32) for Z in (SD.Z_SPLIT, SD.Z_LOOP)]
BATCH, ITERS = 5, 3
ET_BATCH, ET_ITERS = 17, 16
ET_ITERS_USED = {
    "200x100": [2, 16, 16, 2, 16, 6, 3, 1, 16, 16, 2, 7, 16, 3, 2, 16, 16],
    "648x324": [7, 4, 3, 6, 4, 10, 9, 5, 6, 8, 4, 7, 3, 8, 12, 5, 6],
}


def et_input(code):
    """uint16 bit patterns [17, N]: the fine float grid (multiples of 0.5 up to +-8) at 2.0 dB, exact in binary16"""
    y = FD.grid_input(code, ET_BATCH, 2.0, 0.5, 16)
    x = y.astype(np.float16)
    assert np.array_equal(x.astype(np.float32), y)
    return R.bits(x)


def _tables():
    out = [(name, load_table(name)) for name in SHIPPED]
    return out + [(SD.synthetic_name(d, Z), SD.synthetic(d, Z)) for d, Z in SYNTH]


@pytest.mark.parametrize("name,t", _tables(), ids=[n for n, _ in _tables()])
def test_host_equals_restatement(name, t):
    x = R.make_input(BATCH, t.n)
    dec = Decoder(Code(t), device=-1, max_batch=BATCH)
    for algo in sorted(ALGO):
        a, beta = ALGO[algo]
        hard, soft, its = dec.decode_f16_soft(x, ITERS, default_params(algo=a, beta=beta))
        exp = R.decode(t, x, ITERS, algo, beta)
        assert np.array_equal(hard, exp[0]), (name, algo)
        assert np.array_equal(np.asarray(soft).view(np.uint16), exp[1]), (name, algo)
        assert np.array_equal(its, exp[2]), (name, algo)
    dec.close()


def test_two_degree_groups_and_lds_fit():
    """What the table list is chosen for.  (1024x518: its widest layer has 6 checks, so the float plan packs 8
    codewords -- here 8 pairs -- per wave, which passes 64 KB; it runs on the any-H kernel.)"""
    assert len(load_table("1024x518").group_deg) == 2
    L = _lib.lib()
    fits = {}
    for name in ("2048x384", "648x324", "200x100", "1024x518"):
        code = Code(name)
        nl, mw, i8, f32 = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        _lib.check(L.ldpc_code_layer_info(code.handle, C.byref(nl), C.byref(mw), C.byref(i8), C.byref(f32)))
        fits[name] = bool(f32.value)
    assert fits == {"2048x384": False, "648x324": True, "200x100": True, "1024x518": False}, fits


def _et_iters(code):
    t = load_table(code)
    its = R.decode(t, et_input(code), ET_ITERS, "MS", 0.0, True)[2]
    assert its.tolist() == ET_ITERS_USED[code]
    return its


def test_early_termination_input_200x100():
    its = _et_iters("200x100")
    pairs = [(int(its[2 * p]), int(its[2 * p + 1])) for p in range(ET_BATCH // 2)]
    assert any((a < ET_ITERS) != (b < ET_ITERS) for a, b in pairs), "no pair with one half stopping, one never"
    assert any(a == ET_ITERS and b == ET_ITERS for a, b in pairs), "no pair that never stops"
    assert any(a < ET_ITERS and b < ET_ITERS and a != b for a, b in pairs), "no pair whose halves stop apart"
    assert its[ET_BATCH - 1] == ET_ITERS, "codeword 16, alone in its pair, must never stop"


def test_early_termination_input_648x324():
    its = _et_iters("648x324")
    assert ((its >= 3) & (its <= 12)).all()
    apart = sum(int(its[2 * p] != its[2 * p + 1]) for p in range(ET_BATCH // 2))
    assert apart >= 6


def test_switch_on_a_host_context():
    dec = Decoder(Code("648x324"), device=-1, max_batch=4)
    assert dec.f16_all_codes is False
    dec.set_f16_all_codes(True)
    assert dec.f16_all_codes is True
    x = R.make_input(4, 648)
    on = dec.decode_f16_soft(x, 2)
    dec.set_f16_all_codes(False)
    assert dec.f16_all_codes is False
    off = dec.decode_f16_soft(x, 2)
    assert all(np.array_equal(a, b) for a, b in zip(on, off))     # a host context decodes every code either way
    dec.close()
    dec = Decoder(Code("648x324"), device=-1, max_batch=4, f16_all_codes=True)
    assert dec.f16_all_codes is True
    dec.close()
    L = _lib.lib()
    on = C.c_int(5)
    assert L.ldpc_ctx_set_f16_all_codes(None, 1) == _lib.LDPC_EINVAL
    assert L.ldpc_ctx_get_f16_all_codes(None, C.byref(on)) == _lib.LDPC_EINVAL and on.value == 5


def ldsh_rule_shape(n, e, max_width, batch):
    """(lanes per pair, two lanes per check) of ldsh's shape rule, restated: the
    cost max(1, waves / capacity) * (0.82 with two lanes per check, else 1) over
    the shapes from the one the widest layer needs up to 64 lanes, a CU holding
    min(160 KB / LDS bytes of a wave, 12 waves with two lanes per check, 8
    without) waves; the least cost wins, ties go to the narrower shape."""
    pairs = (batch + 1) // 2
    lg0 = 3 if max_width <= 8 else 4 if max_width <= 16 else 5 if max_width <= 32 else 6
    best = None
    for lg in range(lg0, 7):
        split = (1 << lg) >= 2 * max_width
        lds = (2 * e + 15) // 16 * 16 + (64 >> lg) * (n + e) * 4
        cap = 256 * max(1, min(160 * 1024 // lds, 12 if split else 8))
        ppw = 64 >> lg
        waves = (pairs + ppw - 1) // ppw
        num, den = max(cap, waves) * (82 if split else 100), cap
        if best is None or num * best[1] < best[0] * den:
            best = (num, den, 1 << lg, split)
    return best[2], best[3]


def test_shape_rule_restated():
    """The library's rule equals the restatement, and picks what
    tools/f16_short_rate.py measured as fastest (profiles/f16_short_rate.json)."""
    L = _lib.lib()
    tables = [load_table(n) for n in ("648x324", "200x100", "576x288")] + [SD.synthetic(7, 12), SD.synthetic(3, 40)]
    for t in tables:
        code = Code(t)
        nl, mw, i8, f32 = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        _lib.check(L.ldpc_code_layer_info(code.handle, C.byref(nl), C.byref(mw), C.byref(i8), C.byref(f32)))
        e = len(t.edge_var)
        for batch in (1, 5, 17, 130, 1024, 4095, 4096, 8192, 16384, 16385, 65536, 200000):
            lanes, split = ldsh_rule_shape(t.n, e, mw.value, batch)
            assert 1 << L.ldpc_f16_lds_shape_rule(t.n, e, mw.value, (batch + 1) // 2) == lanes, (t.n, batch)
            assert split == (lanes >= 2 * mw.value)
    measured = {("648x324", 1024): 64, ("648x324", 4096): 64, ("648x324", 16384): 64, ("648x324", 65536): 64,
                ("200x100", 1024): 32, ("200x100", 4096): 32, ("200x100", 16384): 16, ("200x100", 65536): 16}
    widest = {"648x324": 27, "200x100": 9}
    for (name, batch), lanes in measured.items():
        t = load_table(name)
        assert ldsh_rule_shape(t.n, len(t.edge_var), widest[name], batch)[0] == lanes, (name, batch)
