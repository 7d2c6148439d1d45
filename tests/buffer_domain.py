"""Shared helpers of the buffer-contract tests (test_buffer_domain_cpu.py,
test_gpu_buffer_domain.py): how the library meets the caller's memory.  A
plain helper module, like param_domain.py; no test lives here.

The contract (include/ldpc_mi355x.h): a device buffer needs only the natural
alignment of its element type, rows beyond `batch` and bytes outside
[batch][N] are never written, node-major columns batch .. ld-1 are never read
as data.  Every buffer of a call is therefore carved out of a larger, canary
filled allocation at a chosen byte offset (`carve`), and every call is checked
three ways: against the oracle, against the same call on 256-byte aligned
buffers, and for untouched canaries.

Inputs and oracle results come from param_domain.py and float_domain.py; the
only arithmetic restated here is the quantiser's rule (`quantize_rule`).
"""
import numpy as np

import float_domain as FD
import oracle as O
import param_domain as PD

FRONT = 256                     # bytes in front of every payload: torch and numpy allocations are this aligned or
                                # are made so (carve asserts it), so a payload's address mod 16 is its byte_offset
OFFSETS_I8 = (0, 1, 4, 8)
OFFSETS_F32 = (0, 4, 8)
OFFSETS_I32 = (0, 4)            # the error counters (8 bytes each) always sit at offset 0
BATCHES = (1, 15, 16, 17, 63, 64, 65)      # the 16-codeword group and the 64-codeword stride, one below and one past
SWEEP_ORDER = (65, 1, 64, 15, 17, 63, 16)  # BATCHES in the order the sweep walks them on one context
MAX_BATCH = 128
ITERS = 2
ET_ITERS = 16
ALIGN_BATCH = 17                # one full 16-codeword group and a ragged one
PAD_BYTE, JUNK = 0x5A, 77       # canary of the input buffers; the node-major columns >= batch


def _layout(shape, itemsize, byte_offset):
    nbytes = int(np.prod(shape)) * itemsize
    row = (int(np.prod(shape[1:])) if len(shape) > 1 else 1) * itemsize
    assert 0 <= byte_offset < 16 and byte_offset % min(itemsize, 8) == 0, (byte_offset, itemsize)
    lo = FRONT + byte_offset
    return nbytes, lo, lo + nbytes + 256 + 2 * row + (16 - byte_offset)


def _report(outside_ok, lo, nbytes, what):
    bad = np.flatnonzero(~outside_ok)
    pos = int(bad[0])
    where = "%d bytes in front of" % (lo - pos) if pos < lo else "%d bytes past the end of" % (pos - lo - nbytes)
    raise AssertionError("%s: %d canary bytes outside the payload were overwritten, the first %s it (payload %d "
                         "bytes)" % (what, bad.size, where, nbytes))


def carve(torch, shape, dtype, byte_offset, fill, what="buffer"):
    """(view, check): a contiguous `dtype` tensor of `shape` whose first byte
    sits `byte_offset` bytes past a 256-byte aligned address, inside one flat
    uint8 device buffer: 256 bytes of front pad, the payload, a back pad of at
    least 256 bytes plus two rows.  Every byte of the buffer, the payload
    included, is `fill`; check() asserts that every byte outside the payload
    still is."""
    itemsize = torch.empty((), dtype=dtype).element_size()
    nbytes, lo, total = _layout(shape, itemsize, byte_offset)
    buf = torch.full((total,), fill, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % FRONT == 0
    view = buf[lo:lo + nbytes].view(dtype).view(*shape)
    assert view.is_contiguous() and (nbytes == 0 or view.data_ptr() == buf.data_ptr() + lo)

    def check():
        ok = (buf == fill)
        ok[lo:lo + nbytes] = True
        if not bool(ok.all()):
            _report(ok.cpu().numpy(), lo, nbytes, what)

    return view, check


def carve_host(shape, dtype, byte_offset, fill, what="buffer"):
    """carve for the host-buffer entry points: a numpy view and its check()."""
    dt = np.dtype(dtype)
    nbytes, lo, total = _layout(shape, dt.itemsize, byte_offset)
    raw = np.full(total + FRONT, fill, dtype=np.uint8)
    base = (-raw.ctypes.data) % FRONT
    buf = raw[base:base + total]
    view = buf[lo:lo + nbytes].view(dt).reshape(shape)
    assert view.flags.c_contiguous and view.ctypes.data % FRONT == lo % FRONT

    def check():
        ok = buf == fill
        ok[lo:lo + nbytes] = True
        if not ok.all():
            _report(ok, lo, nbytes, what)

    return view, check


# ---- inputs and oracle results, one per code, shared by every test ----------

def i8_input(code, kind="ext"):
    """The 65-codeword int8 input of the batch tests; the first B rows are
    param_domain.make_input(kind, B, n)."""
    return PD.make_input(kind, max(BATCHES), PD.load_table(code).n)


def i8_oracle(code, kind="ext", iters=ITERS):
    """(hard, soft, iters_used) of the oracle on i8_input, default parameters."""
    return PD.oracle_on(code, kind, max(BATCHES), PD.CONTROL, iters)


def et_input(code):
    """param_domain.et_input at the batch-edge recipe (param_domain.ET_EDGE)."""
    return PD.et_input(code, max(BATCHES), PD.ET_EDGE[code])


def et_oracle(code):
    return PD.oracle_decode(code, ("et_edge", max(BATCHES)), et_input(code), PD.CONTROL, ET_ITERS, early=True)


def f32_input(code, ebn0=None):
    """float_domain's fine grid, 65 codewords, at the code's EBN0 or `ebn0`."""
    return FD.grid_input(code, max(BATCHES), FD.EBN0[code] if ebn0 is None else ebn0, *FD.FINE)


def f32_oracle(code, iters=ITERS, early=False, ebn0=None):
    """The oracle's plain min-sum decode of f32_input."""
    return FD.oracle_f32(code, ("fine", max(BATCHES), ebn0), f32_input(code, ebn0), O.OMS, 0.0, iters, early)


def prefix(result, batch):
    """The first `batch` codewords of an oracle result (the oracle decodes
    every codeword on its own: test_buffer_domain_cpu.py)."""
    return tuple(a[:batch] for a in result)


def et_edge_conditions(its_a, its_b, iters=ET_ITERS):
    """What the early-termination edge tests need from the oracle's
    iterations used of two codes: in each, stopped and running codewords (or
    codewords stopping at different iterations) among the first 17; codeword
    64 stops early in exactly one of the two."""
    def mixed(its):
        f = its[:17]
        return bool(f.min() < f.max() < iters or f.min() < iters == f.max())
    return {"first 17 mixed, code a": mixed(its_a), "first 17 mixed, code b": mixed(its_b),
            "codeword 64 stops in exactly one": bool((its_a[64] < iters) != (its_b[64] < iters))}


# ---- the quantiser's rule, restated ----------------------------------------

QUANT_SETS = ((8, -31, 31), (1, -128, 127), (16, -7, 9))
# first count at which quantize_k's grid (at most 256 * 64 blocks of 256) walks its stride loop a second time
QUANT_COUNTS = (0, 1, 255, 256, 257, 256 * 64 * 256 + 257)


def quantize_rule(y, factor, sat_neg, sat_pos):
    """include/ldpc_mi355x.h: q = clamp((int)((float)factor * y), sat_neg,
    sat_pos), the product in float32, (int) truncating toward zero; NaN and
    |product| >= 2^31 give sat_neg (INT_MIN clamped)."""
    y = np.asarray(y, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        v = np.float32(factor) * y
        assert v.dtype == np.float32
        fits = np.abs(v) < np.float32(2147483648.0)           # False for NaN
        t = np.where(fits, np.trunc(np.where(fits, v, 0).astype(np.float64)), -2147483648.0)
    return np.clip(t, sat_neg, sat_pos).astype(np.int8)


def quantize_specials(factor):
    """NaN, -NaN, +-inf, +-0, a subnormal, +-2^31 / factor and the floats
    either side of each."""
    edge = np.float32(2147483648.0 / factor)
    near = [np.nextafter(edge, np.float32(0)), edge, np.nextafter(edge, np.float32(np.inf))]
    nan = np.array([0x7FC00000, 0xFFC00000], dtype=np.uint32).view(np.float32)
    x = np.array([np.inf, -np.inf, 0.0, -0.0, 1e-40, -1e-40] + near + [-v for v in near], dtype=np.float32)
    return np.concatenate([nan, x])


def quantize_input(count, factor):
    """float32 [count]: the specials first (as many as fit), then values
    uniform over +-20 from param_domain's splitmix64 stream 20."""
    y = ((PD._draw32(1, max(count, 1), 20)[0, :count].astype(np.float64) / 2.0 ** 32 - 0.5) * 40.0).astype(np.float32)
    s = quantize_specials(factor)[:count]
    y[:s.size] = s
    return y


def count_reference(hard, ref, k):
    """[bit errors, frame errors] over the first k positions: bit 0 of hard
    against bit 0 of ref (None: the all-zero codeword)."""
    r = np.zeros_like(hard) if ref is None else ref
    e = ((hard ^ r) & 1)[:, :k].astype(np.int64)
    return [int(e.sum()), int((e.sum(axis=1) > 0).sum())]


def bits(shape, stream):
    """uint8 0/1 array from param_domain's splitmix64 stream `stream`."""
    n = int(np.prod(shape))
    return (PD._draw32(1, n, stream)[0] >> np.uint64(31)).astype(np.uint8).reshape(shape)


# ---- section A: the alignment cases and the launch path each must select ----
# (entry, code, kernel, node-major pitch or None, byte offsets of llr / hard / soft / iters_used)

def _case(entry, code, kernel, ld, llr, hard, soft, its):
    return (entry, code, kernel, ld, (llr, hard, soft, its))


def case_id(case):
    entry, code, kernel, ld, (llr, hard, soft, its) = case
    return "%s-%s-k%d-%sllr%d-out%d.%d.%d" % (entry, code, kernel, "ld%d-" % ld if ld else "", llr, hard, soft, its)


def pytest_id(case):
    """The pytest id of an alignment case: its case_id and the kernel it pins."""
    return "%s=%s" % (case_id(case), EXPECTED_PATH[case_id(case)].split()[0].rstrip(":,"))


ALIGN_CASES = (
    # coop3's input transpose: the 16-byte kernel, and the byte kernel that only an unaligned pointer reaches
    [_case("i8", c, 8, None, o, 0, 0, 0) for c in ("dvbs2_r1_2", "dvbs2_r9_10") for o in OFFSETS_I8] +
    # the 64 x 64 tile transposes in front of and behind generic, windowed, windowed2 and coop
    [_case("i8", "dvbs2_r1_2", k, None, 1, 1, 1, 4) for k in (1, 2, 3, 5)] +
    # node-major input: 16-byte pieces with a ragged last one, bytes by pointer, bytes by pitch
    [_case("nm", c, k, ld, o, o, o, 4 * o)
     for c, ks in (("dvbs2_r1_2", (8, 5, 1)), ("576x288", (1, 7))) for k in ks for ld, o in ((64, 0), (64, 1), (50, 0))] +
    # lds_decode's LLR staging, int8: N % 16 == 0 (576) and 8 (648), pointer 0 / 1 / 8; generic beside it
    [_case("i8", c, k, None, o, o, o, 0) for c in ("576x288", "648x324") for k in (7, 1) for o in (0, 1, 8)] +
    # the same in float: 4 N % 16 == 0 for both codes, pointer 0 / 4 / 8; ldsep and generic beside it
    [_case("f32", c, k, None, o, 0, 4, 0)
     for c, ks in (("648x324", (7, 9, 1)), ("200x100", (7, 1))) for k in ks for o in OFFSETS_F32] +
    # stairf: float tile transposes
    [_case("f32", "dvbs2_r1_2", 11, None, 4, 0, 4, 4)])

_TILE = "interleave_k / deinterleave_k: element accesses through a 64 x 64 LDS tile"
_GRP_OUT = ", deinterleave_grp_k out"
EXPECTED_PATH = {}
EXPECTED_PATH.update({"i8-%s-k8-llr0-out0.0.0" % c: "interleave_grp_vec_k (16-byte loads)" + _GRP_OUT
                      for c in ("dvbs2_r1_2", "dvbs2_r9_10")})
EXPECTED_PATH.update({"i8-%s-k8-llr%d-out0.0.0" % (c, o): "interleave_grp_k (byte loads: pointer)" + _GRP_OUT
                      for c in ("dvbs2_r1_2", "dvbs2_r9_10") for o in (1, 4, 8)})
EXPECTED_PATH.update({"i8-dvbs2_r1_2-k%d-llr1-out1.1.4" % k: _TILE for k in (1, 2, 3, 5)})
for _c, _k in (("dvbs2_r1_2", 8), ("dvbs2_r1_2", 5), ("dvbs2_r1_2", 1), ("576x288", 1)):
    EXPECTED_PATH.update({
        "nm-%s-k%d-ld64-llr0-out0.0.0" % (_c, _k): "nm_pieces_k: 16-byte load of piece 0, masked bytes for the ragged piece 1",
        "nm-%s-k%d-ld64-llr1-out1.1.4" % (_c, _k): "nm_pieces_k: masked byte loads (pointer)",
        "nm-%s-k%d-ld50-llr0-out0.0.0" % (_c, _k): "nm_pieces_k: masked byte loads (pitch)"})
EXPECTED_PATH.update({"nm-576x288-k7-ld%d-llr%d-out%d.%d.%d" % (ld, o, o, o, 4 * o):
                      "deinterleave_k (bytes) to frame-major scratch, then lds_decode's 16-byte staging of the scratch"
                      for ld, o in ((64, 0), (64, 1), (50, 0))})
EXPECTED_PATH.update({"i8-576x288-k7-llr0-out0.0.0": "lds_decode: 16-byte LLR staging",
                      "i8-576x288-k7-llr1-out1.1.0": "lds_decode: element loop (pointer)",
                      "i8-576x288-k7-llr8-out8.8.0": "lds_decode: element loop (pointer)"})
EXPECTED_PATH.update({"i8-648x324-k7-llr%d-out%d.%d.0" % (o, o, o): "lds_decode: element loop (N % 16 == 8)"
                      for o in (0, 1, 8)})
EXPECTED_PATH.update({"i8-%s-k1-llr%d-out%d.%d.0" % (c, o, o, o): _TILE
                      for c in ("576x288", "648x324") for o in (0, 1, 8)})
for _c in ("648x324", "200x100"):
    EXPECTED_PATH.update({"f32-%s-k7-llr0-out0.4.0" % _c: "lds_decode: 16-byte LLR staging",
                          "f32-%s-k7-llr4-out0.4.0" % _c: "lds_decode: element loop (pointer)",
                          "f32-%s-k7-llr8-out0.4.0" % _c: "lds_decode: element loop (pointer)"})
    EXPECTED_PATH.update({"f32-%s-k1-llr%d-out0.4.0" % (_c, o): _TILE for o in OFFSETS_F32})
EXPECTED_PATH.update({"f32-648x324-k9-llr%d-out0.4.0" % o: "ldsep: element loads and stores" for o in OFFSETS_F32})
EXPECTED_PATH["f32-dvbs2_r1_2-k11-llr4-out0.4.4"] = _TILE + " around stairf"
# the other entry points
MIXED_OFFSETS = ((0, 0, 0), (1, 1, 4))     # llr, hard, iters_used
EXPECTED_PATH.update({
    "mixed-llr0-out0.0": "copy_rows_k: 16-byte gather and scatter of the rows; the 4-byte iteration rows by bytes",
    "mixed-llr1-out1.4": "copy_rows_k: byte gather (src) and byte scatter (dst); the 4-byte iteration rows by bytes"})
COUNT_CODES = {"dvbs2_r1_2": 32400, "576x288": 284, "9972x4986": 4986}    # code -> k
COUNT_OFFSETS = (0, 1, 4)


def count_id(code, off_hard, off_ref):
    return "count-%s-hard%d-ref%s" % (code, off_hard, off_ref)


for _h in COUNT_OFFSETS:
    for _r in COUNT_OFFSETS + (None,):      # None: no reference (a null pointer counts as aligned)
        _offs = (_h, _r or 0)
        EXPECTED_PATH[count_id("dvbs2_r1_2", _h, _r)] = (      # n and k multiples of 16: the pointers decide
            "count_errors_k: byte loads (pointer)" if 1 in _offs else
            "count_errors_k: dword loads (pointer)" if 4 in _offs else "count_errors_k: 16-byte loads")
        EXPECTED_PATH[count_id("576x288", _h, _r)] = (         # k % 16 == 12: never the 16-byte path
            "count_errors_k: byte loads (pointer)" if 1 in _offs else "count_errors_k: dword loads")
        EXPECTED_PATH[count_id("9972x4986", _h, _r)] = "count_errors_k: byte loads (k % 4 == 2)"
EXPECTED_PATH.update({
    "decode_count-648x324-f32-k9": "ldsep's fused count: bytes of ref at offset 1",
    "decode_count-648x324-f32-k7": "lds_decode, then count_errors_k: byte loads (ref at offset 1)",
    "decode_count-576x288-i8-k7": "lds_decode, then count_errors_k: byte loads (ref at offset 1)",
    "awgn-576x288-out1": "awgn_i8_k: byte stores",
    "quantize-576x288-in4-out1": "quantize_k: element loads and stores",
    "info_bits-576x288-out0": "info_bits_k: 8-byte stores",
    "info_bits-576x288-out1": "info_bits_k: byte stores (pointer)",
    "info_bits-9972x4986-out0": "info_bits_k: 8-byte stores and a 6-byte tail",
})
