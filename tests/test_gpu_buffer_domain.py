"""How the library meets the caller's memory (include/ldpc_mi355x.h, "Buffer
contract"): pointer alignment, writes past the batch, the batch
sizes around the 16-codeword group and the 64-codeword stride, and one context
serving many different calls.  The value domain of the kernels is covered by
test_gpu_param_domain.py, test_gpu_float_domain.py and
test_gpu_short_domain.py; every one of those passes tensors straight from the
allocator (256-byte aligned, exactly `batch` rows) to a context that only ever
sees one shape.

Every buffer here is carved out of a canary-filled allocation at a chosen byte
offset (buffer_domain.carve).  Every decode is compared bit for bit with the
oracle -- hard, soft, iterations used; float as test_gpu_float_domain.py does,
the sign of a zero included -- and every canary byte must survive.  No
tolerance anywhere.

A. Alignment: every device entry point at the offsets of
   buffer_domain.ALIGN_CASES; buffer_domain.EXPECTED_PATH names the launch path
   each case pins (interleave_grp_k, coop3's byte-wise input transpose, is
   reached by an unaligned pointer only).  Batch 17, 2 iterations.
B. Batch edges 1, 15, 16, 17, 63, 64, 65 on one context per (code, kernel), in
   an order that shrinks and grows; batch 0 and batch max_batch + 1; early
   termination at batch 1, 17, 65; literal call sequences that switch kernel,
   element type, batch, early termination and input layout on a live context.
C. The helper kernels: the quantiser on specials and past its grid cap, the
   channel past its grid cap, the error counter's accumulation and bounds.

test_buffer_domain_cpu.py shows what this file takes for granted: the oracle
decodes every codeword on its own (so a prefix of a 65-codeword result is the
result of the prefix), the early-termination inputs put stopped and running
codewords where the edges are, the quantiser restatement agrees with the
oracle's, and EXPECTED_PATH names every case generated here."""
import ctypes as C

import numpy as np
import pytest

import buffer_domain as BD
import float_domain as FD
import oracle as O
import param_domain as PD
from ldpcgputegra_amd import ALGO_MS, Code, Decoder, LdpcError, _lib, channel, default_params, load_table
from ldpcgputegra_amd.decoder import MixedDecoder
from test_gpu_float_domain import assert_same
from test_gpu_parity import kernels_for
from test_gpu_short_domain import assert_equal

pytestmark = pytest.mark.gpu

_decoders = {}
_baseline = {}


def _torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def decoder(code, kernel):
    if (code, kernel) not in _decoders:
        _decoders[(code, kernel)] = Decoder(Code(code), max_batch=BD.MAX_BATCH, kernel=kernel)
    return _decoders[(code, kernel)]


def upload(x, offset, what="llr"):
    """(view, check): the host array x in a carved device buffer at `offset`."""
    torch = _torch()
    dtype = {"int8": torch.int8, "uint8": torch.uint8, "float32": torch.float32}[x.dtype.name]
    view, check = BD.carve(torch, x.shape, dtype, offset, BD.PAD_BYTE, what)
    view.copy_(torch.from_numpy(np.array(x)))
    return view, check


def node_major(x, batch, ld):
    """[N][ld] with the first `batch` codewords of x in columns 0 .. batch-1 and junk in the others."""
    nm = np.full((x.shape[1], ld), BD.JUNK, dtype=np.int8)
    nm[:, :batch] = x[:batch].T
    return nm


def outputs(batch, n, f32, offsets=(0, 0, 0)):
    """Sentinel-filled carved outputs: ((hard, soft, iters_used), checks)."""
    torch = _torch()
    hard, c1 = BD.carve(torch, (batch, n), torch.uint8, offsets[0], 9, "hard")
    soft, c2 = BD.carve(torch, (batch, n), torch.float32 if f32 else torch.int8, offsets[1], 99, "soft")
    its, c3 = BD.carve(torch, (batch,), torch.int32, offsets[2], 0xF9, "iters_used")
    its.fill_(-7)
    return (hard, soft, its), (c1, c2, c3)


def params_of(entry, early=False):
    if entry == "f32":
        return default_params(algo=ALGO_MS, beta=0.0, early_term=int(early))
    return PD.CONTROL.product(early_term=int(early))


def call(dec, entry, d_llr, out, batch, iters, early):
    hard, soft, its = out
    p = params_of(entry, early)
    if entry == "nm":
        dec.decode_i8_nm_device(d_llr, hard, iters, batch=batch, params=p, soft=soft, iters_used=its)
    elif entry == "f32":
        dec.decode_f32_device(d_llr, hard, iters, params=p, soft=soft, iters_used=its)
    else:
        dec.decode_i8_device(d_llr, hard, iters, params=p, soft=soft, iters_used=its)


def decode(dec, entry, x, batch, iters, early=False, offsets=(0, 0, 0, 0), ld=None):
    """One device decode of the first `batch` codewords of x through carved
    buffers at `offsets` (llr, hard, soft, iters_used): (hard, soft,
    iters_used) as numpy, after every canary was checked."""
    torch = _torch()
    d_llr, c0 = upload(node_major(x, batch, ld) if entry == "nm" else x[:batch], offsets[0])
    out, checks = outputs(batch, dec.code.n, entry == "f32", offsets[1:])
    call(dec, entry, d_llr, out, batch, iters, early)
    torch.cuda.synchronize()
    got = tuple(t.cpu().numpy() for t in out)
    for check in (c0,) + checks:
        check()
    return got


def compare(entry, got, exp, where):
    if entry == "f32":
        assert_same(got, exp, where, bitwise=True)
    else:
        assert_equal(got, exp, where)


def source(entry, code, early=False):
    """(input, oracle result, iterations) of 65 codewords for this kind of call."""
    if entry == "f32":
        ebn0 = FD.EDGE_EBN0.get(code) if early else None
        iters = BD.ET_ITERS if early else BD.ITERS
        return BD.f32_input(code, ebn0), BD.f32_oracle(code, iters, early, ebn0), iters
    if early:
        return BD.et_input(code), BD.et_oracle(code), BD.ET_ITERS
    return BD.i8_input(code), BD.i8_oracle(code), BD.ITERS


def kernel_name(kernel):
    return Decoder.KERNEL_NAMES[kernel]


# ---- A. alignment and canaries ---------------------------------------------

ALIGN_IDS = [BD.case_id(c) for c in BD.ALIGN_CASES]


def test_kernels_exist_for_the_cases():
    """Every forced kernel of this file can schedule its code (none of the
    cases below may refuse)."""
    ks = {}
    for entry, code, kernel, _, _ in BD.ALIGN_CASES:
        if entry != "f32":
            ks.setdefault(code, set()).add(kernel)
    for code, need in ks.items():
        assert need <= set(kernels_for(code)), (code, need)
    assert len(set(ALIGN_IDS)) == len(ALIGN_IDS)


@pytest.mark.parametrize("case", BD.ALIGN_CASES, ids=BD.pytest_id)
def test_alignment_decode(case):
    """One decode entry point with its buffers at the case's byte offsets:
    (i) equal to the oracle, (ii) bit-identical to the same call on aligned
    buffers, (iii) every canary intact.  The id names the kernel the offsets
    select (buffer_domain.EXPECTED_PATH, from reading the launchers)."""
    entry, code, kernel, ld, offsets = case
    x, exp, iters = source(entry, code)
    B = BD.ALIGN_BATCH
    dec = decoder(code, kernel)
    where = "%s (%s)" % (BD.case_id(case), BD.EXPECTED_PATH[BD.case_id(case)])
    got = decode(dec, entry, x, B, iters, offsets=offsets, ld=ld)
    assert dec.last_kernel == kernel_name(kernel), where
    compare(entry, got, BD.prefix(exp, B), where)
    key = (entry, code, kernel, ld)
    if key not in _baseline:
        _baseline[key] = decode(dec, entry, x, B, iters, ld=ld)
    for g, b, what in zip(got, _baseline[key], ("hard", "soft", "iters_used")):
        assert g.tobytes() == b.tobytes(), "%s: %s differs from the aligned call" % (where, what)


_mixed = {}


def mixed(names):
    if names not in _mixed:
        _mixed[names] = MixedDecoder(list(names), max_batch=BD.MAX_BATCH)
    return _mixed[names]


def mixed_expected(names, x, ids, key):
    """hard decisions of the oracle, each codeword under its own code."""
    exp = np.empty(x.shape, dtype=np.uint8)
    for c, name in enumerate(names):
        sel = np.where(ids == c)[0]
        if sel.size:
            exp[sel] = PD.oracle_decode(name, key + (c,), x[sel], PD.CONTROL, BD.ITERS)[0]
    return exp


MIXED_CODES = ("dvbs2_r1_2", "dvbs2_r9_10")


@pytest.mark.parametrize("offsets", BD.MIXED_OFFSETS, ids=lambda o: "llr%d-out%d.%d" % o)
def test_alignment_mixed_decoder(offsets):
    """MixedDecoder: llr and hard at byte offset 1 send the gather and the
    scatter of copy_rows_k down its byte path (offset 0: the 16-byte path);
    the iterations-used scatter (row_bytes 4) takes the byte path always."""
    torch = _torch()
    assert "mixed-llr%d-out%d.%d" % offsets in BD.EXPECTED_PATH
    B = BD.ALIGN_BATCH
    x = BD.i8_input(MIXED_CODES[0])[:B]
    ids = (np.arange(B, dtype=np.int32) * 3 + 1) % 2
    mx = mixed(MIXED_CODES)
    d_llr, c0 = upload(x, offsets[0])
    (hard, _, its), checks = outputs(B, x.shape[1], False, (offsets[1], 0, offsets[2]))
    mx.decode_i8_device(d_llr, hard, ids, BD.ITERS, params=params_of("i8"), iters_used=its)
    torch.cuda.synchronize()
    for check in (c0,) + checks:
        check()
    assert mx.last_kernels() == ["coop3", "coop3"]
    got = hard.cpu().numpy()
    assert np.array_equal(got, mixed_expected(MIXED_CODES, x, ids, ("ext", B, "mixed-align")))
    assert (its.cpu().numpy() == BD.ITERS).all()
    _baseline.setdefault("mixed", got)
    assert np.array_equal(got, _baseline["mixed"])


def counters(preset=(0, 0)):
    torch = _torch()
    view, check = BD.carve(torch, (2,), torch.int64, 0, 0xC3, "counters")
    view.copy_(torch.tensor(preset, dtype=torch.int64))
    return view, check


@pytest.mark.parametrize("code", sorted(BD.COUNT_CODES))
def test_alignment_count_errors(code):
    """ldpc_count_errors_async with hard and ref at byte offsets 0, 1, 4: the
    16-byte, dword and byte paths of count_errors_k by shape (k) and by
    pointer, against a numpy count.  Junk in bits 1 .. 7 of a ref byte counts
    nothing: every path compares bit 0."""
    torch = _torch()
    n, k, B = load_table(code).n, BD.COUNT_CODES[code], 5
    dec = decoder(code, 0)
    hard, ref = BD.bits((B, n), 30), BD.bits((B, n), 31)
    ref[1] = hard[1]                       # a codeword without errors
    ref[3] = hard[3]
    ref[3, k - 1] ^= 1                     # one error, in the last counted position
    ref[3, k:] ^= 1                        # errors beyond k do not count
    junk = ref | (BD.bits((B, n), 32) << 1) | (BD.bits((B, n), 33) << 7)
    for oh in BD.COUNT_OFFSETS:
        d_hard, ch = upload(hard, oh, "hard")
        for orf in BD.COUNT_OFFSETS + (None,):
            assert BD.count_id(code, oh, orf) in BD.EXPECTED_PATH
            for r in (ref, junk) if orf is not None else (None,):
                d_ref, cr = upload(r, orf, "ref") if r is not None else (None, lambda: None)
                cnt, cc = counters()
                dec.count_errors_device(d_hard, k, cnt, ref=d_ref)
                torch.cuda.synchronize()
                where = "%s (%s)" % (BD.count_id(code, oh, orf), BD.EXPECTED_PATH[BD.count_id(code, oh, orf)])
                assert cnt.tolist() == BD.count_reference(hard, None if r is None else ref, k), where
                for check in (ch, cr, cc):
                    check()


@pytest.mark.parametrize("code,entry,kernel", [("648x324", "f32", 9), ("648x324", "f32", 7), ("576x288", "i8", 7)])
def test_alignment_decode_count(code, entry, kernel):
    """ldpc_decode_*_count_async with ref at byte offset 1 (junk in its upper
    bits): ldsep's fused count and the separate count launch give a numpy
    count over the oracle's hard decisions."""
    torch = _torch()
    assert "decode_count-%s-%s-k%d" % (code, entry, kernel) in BD.EXPECTED_PATH
    t = load_table(code)
    x, exp, iters = source(entry, code)
    B = BD.ALIGN_BATCH
    exp = BD.prefix(exp, B)
    ref = BD.bits((B, t.n), 34)
    ref[2] = exp[0][2]                     # a codeword without errors
    dec = decoder(code, kernel)
    for r in (ref | (BD.bits((B, t.n), 35) << 1), None):
        d_llr, c0 = upload(x[:B], 0)
        d_ref, cr = upload(r, 1, "ref") if r is not None else (None, lambda: None)
        out, checks = outputs(B, t.n, entry == "f32")
        cnt, cc = counters((5, 7))
        dec.decode_count_device(d_llr, out[0], iters, t.k_info, cnt, ref=d_ref, params=params_of(entry), soft=out[1],
                                iters_used=out[2])
        torch.cuda.synchronize()
        assert dec.last_kernel == kernel_name(kernel)
        compare(entry, tuple(o.cpu().numpy() for o in out), exp, "decode_count %s kernel %d" % (code, kernel))
        bit, frame = BD.count_reference(exp[0], None if r is None else ref, t.k_info)
        assert frame < B or r is None
        assert cnt.tolist() == [5 + bit, 7 + frame]
        for check in (c0, cr, cc) + checks:
            check()


def test_alignment_channel_quantiser_bit_source():
    """awgn_i8_device, quantize_device and info_bits_device writing at byte
    offset 1 (the quantiser reading floats at offset 4): equal to the host
    generators and to oracle.quantize; info_bits also at offset 0 (8-byte
    stores) and with a ragged tail (K * batch % 8 == 6)."""
    torch = _torch()
    code, B = "576x288", 5
    t = load_table(code)
    dec = decoder(code, 0)
    table = channel.i8_table(0.87)
    llr, c0 = BD.carve(torch, (B, t.n), torch.int8, 1, BD.PAD_BYTE, "awgn llr")
    dec.awgn_i8_device(llr, first_cw=123, seed=42, table=table)
    y = BD.quantize_input(B * t.n, 8)
    d_y, c1 = upload(y, 4, "quantiser input")
    q, c2 = BD.carve(torch, (B * t.n,), torch.int8, 1, BD.PAD_BYTE, "quantiser output")
    dec.quantize_device(d_y, q)
    torch.cuda.synchronize()
    assert np.array_equal(llr.cpu().numpy(), channel.awgn_i8_host(t.n, B, 42, table, first_cw=123))
    assert np.array_equal(q.cpu().numpy(), O.quantize(y))
    assert np.array_equal(q.cpu().numpy(), BD.quantize_rule(y, 8, -31, 31))
    for check in (c0, c1, c2):
        check()
    for name, batch, off in (("576x288", B, 0), ("576x288", B, 1), ("9972x4986", 3, 0)):
        assert "info_bits-%s-out%d" % (name, off) in BD.EXPECTED_PATH
        k = load_table(name).k_info
        info, ci = BD.carve(torch, (batch, k), torch.uint8, off, BD.PAD_BYTE, "info bits")
        decoder(name, 0).info_bits_device(info, first_cw=2 ** 33 + 5, seed=9)
        torch.cuda.synchronize()
        assert np.array_equal(info.cpu().numpy(), channel.info_bits_host(k, batch, 9, first_cw=2 ** 33 + 5)), (name, off)
        ci()


# ---- B. batch edges and context reuse ---------------------------------------

SWEEP = ([("i8", c, 8) for c in FD.DVBS2] +              # coop3_decode<D> is a template per first-group degree
         [("i8", "dvbs2_r1_2", k) for k in (1, 2, 3, 5)] + [("i8", "dvbs2_r9_10", k) for k in (1, 3)] +
         [("f32", c, 11) for c in ("dvbs2_r1_2", "dvbs2_r9_10")] + [("f32", "648x324", k) for k in (1, 7, 9)] +
         [("nm", "dvbs2_r1_2", 8)])


def refuses(dec, entry, batch):
    """The status of a decode of `batch` zero codewords that must be refused."""
    torch = _torch()
    n = dec.code.n
    d_llr = torch.zeros((n, batch) if entry == "nm" else (batch, n), dtype=torch.float32 if entry == "f32" else torch.int8,
                        device="cuda")
    out, checks = outputs(1, n, entry == "f32")
    with pytest.raises(LdpcError) as e:
        call(dec, entry, d_llr, out, batch, BD.ITERS, False)
    torch.cuda.synchronize()
    for check in checks:
        check()
    return e.value.status


def writes_nothing_at_batch_zero(dec, entry):
    torch = _torch()
    n = dec.code.n
    d_llr = torch.zeros((n, 4) if entry == "nm" else (0, n), dtype=torch.float32 if entry == "f32" else torch.int8,
                        device="cuda")
    (hard, soft, its), checks = outputs(1, n, entry == "f32")
    before = [t.clone() for t in (hard, soft, its)]
    call(dec, entry, d_llr, (hard, soft, its), 0, BD.ITERS, False)
    torch.cuda.synchronize()
    for a, b in zip((hard, soft, its), before):
        assert a.view(torch.uint8).equal(b.view(torch.uint8)), "batch 0 wrote to an output"
    for check in checks:
        check()


@pytest.mark.parametrize("entry,code,kernel", SWEEP, ids=lambda v: str(v))
def test_batch_sweep_on_one_context(entry, code, kernel):
    """Batches 65, 1, 64, 15, 17, 63, 16 in that order on one context of
    max_batch 128 (so the sweep shrinks and grows the scratch in use), outputs
    of exactly `batch` rows between canaries: every batch equals the first
    rows of the oracle's 65-codeword result.  The node-major entry runs with
    ld = batch + 3.  Then batch 0 (OK, nothing written) and batch 129
    (LDPC_EINVAL)."""
    x, exp, iters = source(entry, code)
    dec = decoder(code, kernel)
    for B in BD.SWEEP_ORDER:
        got = decode(dec, entry, x, B, iters, ld=B + 3 if entry == "nm" else None)
        where = "%s %s kernel %d batch %d" % (entry, code, kernel, B)
        assert dec.last_kernel == kernel_name(kernel), where
        compare(entry, got, BD.prefix(exp, B), where)
    writes_nothing_at_batch_zero(dec, entry)
    assert refuses(dec, entry, BD.MAX_BATCH + 1) == _lib.LDPC_EINVAL


ET_CASES = [("i8", "dvbs2_r1_2", 5, {}), ("i8", "dvbs2_r1_2", 8, {}), ("i8", "dvbs2_r8_9", 8, {}),
            ("f32", "dvbs2_r1_2", 11, {}), ("f32", "dvbs2_r8_9", 11, {}),
            # windowed and windowed2 write iterations used from inside the kernel, at the iteration a codeword stops
            ("i8", "dvbs2_r1_2", 2, {}), ("i8", "dvbs2_r1_2", 3, {}), ("i8", "dvbs2_r8_9", 3, {}),
            # coop's launch-per-iteration early termination keeps `live` in the context's scratch between launches
            # (as stairf always does); coop's default and coop3 keep it inside the kernel
            ("i8", "dvbs2_r1_2", 5, {"LDPC_COOP_ET_KERNEL": "0"})]


@pytest.mark.parametrize("entry,code,kernel,env", ET_CASES, ids=["%s-%s-%d%s" % (e, c, k, "-per-launch" if env else "") for e, c, k, env in ET_CASES])
def test_early_termination_at_batch_edges(entry, code, kernel, env, monkeypatch):
    """Early termination, 16 iterations, at batch 1, 17 and 65: the padding
    codewords of the last group are all-zero LLRs whose syndrome is 0 from the
    start, next to codewords that stop and codewords that never do
    (param_domain.ET_EDGE, float_domain.EDGE_EBN0; the conditions are checked
    on the oracle in test_buffer_domain_cpu.py).  coop (5) is built for r1/2
    only of the two codes.  The three batches run on one context, so the
    early-termination state of a call (live, bad, iterations used in the
    context's scratch: stairf, coop per launch) meets the next call's."""
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    x, exp, iters = source(entry, code, early=True)
    dec = decoder(code, kernel)
    for B in (1, 17, 65):
        got = decode(dec, entry, x, B, iters, early=True)
        where = "%s %s kernel %d early termination batch %d" % (entry, code, kernel, B)
        assert dec.last_kernel == kernel_name(kernel), where
        compare(entry, got, BD.prefix(exp, B), where)


# one context per code, max_batch 128, the kernel switched with set_kernel; every step is checked against the
# oracle before the next is issued; `same_as`: the step must also reproduce that earlier step's own output
SEQUENCES = {
    "dvbs2_r1_2": [
        dict(kernel=8, entry="i8", batch=65, early=True),
        dict(kernel=8, entry="i8", batch=17, early=False),
        dict(kernel=5, entry="i8", batch=64, early=True),
        dict(kernel=3, entry="i8", batch=1, early=False),
        dict(kernel=2, entry="i8", batch=65, early=False),
        dict(kernel=1, entry="i8", batch=16, early=False),
        dict(kernel=11, entry="f32", batch=17, early=True),
        dict(kernel=8, entry="nm", batch=63, ld=70, early=False),
        dict(kernel=8, entry="i8", batch=65, early=True, same_as=0),
    ],
    "648x324": [
        dict(kernel=7, entry="i8", batch=65, early=False),
        dict(kernel=9, entry="f32", batch=3, early=True),
        dict(kernel=1, entry="i8", batch=64, early=False),
        dict(kernel=7, entry="nm", batch=17, ld=20, early=False),   # the message scratch as transpose scratch
        dict(kernel=1, entry="f32", batch=65, early=False),
        dict(kernel=7, entry="i8", batch=65, early=False, same_as=0),
    ],
}


@pytest.mark.parametrize("code", sorted(SEQUENCES))
def test_call_sequence_on_one_context(code):
    """The scratch of a context (V, the message area that holds per-edge,
    compressed, float and transpose data in turn, the early-termination
    state) is shared by every kernel family: a literal sequence of calls that
    differ in kernel, element type, batch, early termination and input layout,
    each equal to the oracle, the last equal to the first."""
    dec = Decoder(Code(code), max_batch=BD.MAX_BATCH)
    done = []
    for i, step in enumerate(SEQUENCES[code]):
        x, exp, iters = source(step["entry"], code, step["early"])
        dec.set_kernel(step["kernel"])
        got = decode(dec, step["entry"], x, step["batch"], iters, early=step["early"], ld=step.get("ld"))
        where = "%s step %d: %r" % (code, i + 1, step)
        assert dec.last_kernel == kernel_name(step["kernel"]), where
        compare(step["entry"], got, BD.prefix(exp, step["batch"]), where)
        if "same_as" in step:
            for g, b in zip(got, done[step["same_as"]]):
                assert g.tobytes() == b.tobytes(), where
        done.append(got)
    dec.close()


def test_mixed_decoder_consecutive_calls():
    """Three mixed decodes with different id maps queued without a
    synchronisation in between (the pinned index arrays and the `pending`
    events are handed from call to call): the first is all one code -- the
    other code's context reports no kernel until the second call uses it --
    the second fills max_batch."""
    torch = _torch()
    n = load_table(MIXED_CODES[0]).n
    x = PD.make_input("ext", BD.MAX_BATCH, n)
    maps = [np.zeros(17, dtype=np.int32), (np.arange(BD.MAX_BATCH, dtype=np.int32) * 7 + 1) % 2,
            np.concatenate([np.ones(20, dtype=np.int32), np.arange(45, dtype=np.int32) % 2])]
    mx = MixedDecoder(list(MIXED_CODES), max_batch=BD.MAX_BATCH)
    assert mx.last_kernels() == ["none", "none"]
    queued = []
    for i, ids in enumerate(maps):
        B = ids.size
        d_llr, c0 = upload(x[:B], 0)
        (hard, _, its), checks = outputs(B, n, False)
        mx.decode_i8_device(d_llr, hard, ids, BD.ITERS, params=params_of("i8"), iters_used=its)
        assert mx.last_kernels() == ["coop3", "none" if i == 0 else "coop3"]
        queued.append((d_llr, hard, its, (c0,) + checks))
    torch.cuda.synchronize()
    for i, (ids, (_, hard, its, checks)) in enumerate(zip(maps, queued)):
        exp = mixed_expected(MIXED_CODES, x[:ids.size], ids, ("ext", BD.MAX_BATCH, "mixed-seq", i))
        assert np.array_equal(hard.cpu().numpy(), exp), "call %d" % (i + 1)
        assert (its.cpu().numpy() == BD.ITERS).all(), "call %d" % (i + 1)
        for check in checks:
            check()
    mx.close()


# ---- C. helper kernels -------------------------------------------------------

@pytest.mark.parametrize("factor,sat_neg,sat_pos", BD.QUANT_SETS)
def test_quantiser_specials_and_counts(factor, sat_neg, sat_pos):
    """NaN, -NaN, +-inf, +-0, subnormals, +-2^31 / factor and its neighbours,
    then uniform values, at counts 0, 1, 255, 256, 257 and the first count at
    which quantize_k's grid-stride loop makes a second pass: the device call,
    the host-buffer call and a host (device -1) context all equal the numpy
    restatement of the header's rule."""
    torch = _torch()
    dec = decoder("576x288", 0)
    host = Decoder(Code("576x288"), device=-1, max_batch=1)
    for count in BD.QUANT_COUNTS:
        y = BD.quantize_input(count, factor)
        exp = BD.quantize_rule(y, factor, sat_neg, sat_pos)
        if count >= 14:
            assert np.isnan(y[:2]).all() and (exp[:2] == sat_neg).all()
        d_y, c0 = upload(y, 0, "quantiser input")
        q, c1 = BD.carve(torch, (count,), torch.int8, 0, BD.PAD_BYTE, "quantiser output")
        dec.quantize_device(d_y, q, factor, sat_neg, sat_pos)
        torch.cuda.synchronize()
        for got, how in ((q.cpu().numpy(), "device"), (dec.quantize(y, factor, sat_neg, sat_pos), "host buffers"),
                         (host.quantize(y, factor, sat_neg, sat_pos), "host context")):
            diff = got != exp
            assert not diff.any(), "%s, count %d: %d values differ, the first at %d: y = %r gives %d, expected %d" % (
                how, count, int(diff.sum()), int(np.argmax(diff)), y[np.argmax(diff)], got[np.argmax(diff)],
                exp[np.argmax(diff)])
        c0()
        c1()
    host.close()


def test_channel_past_its_grid():
    """awgn_i8_device on 33 x 64800 LLRs (2,138,400 elements: more than the
    8192 x 256 threads of awgn_i8_k's grid, so it strides), random codewords,
    first_cw beyond 2^40, both tables of
    test_device_channel_matches_host_generator: equal to the host generator;
    batch 0 writes nothing."""
    torch = _torch()
    code, B, first = "dvbs2_r1_2", 33, 2 ** 40 + 3
    n = load_table(code).n
    assert B * n > 8192 * 256
    dec = decoder(code, 0)
    cw = BD.bits((B, n), 36)
    d_cw, c0 = upload(cw, 0, "codewords")
    for table in (channel.i8_table(0.87), channel.i8_table(0.87, 8, 31, amp=channel.QPSK, normalize=True)):
        llr, c1 = BD.carve(torch, (B, n), torch.int8, 0, BD.PAD_BYTE, "awgn llr")
        dec.awgn_i8_device(llr, first_cw=first, seed=42, table=table, codeword=d_cw)
        torch.cuda.synchronize()
        assert np.array_equal(llr.cpu().numpy(), channel.awgn_i8_host(n, B, 42, table, first_cw=first, codeword=cw))
        c0()
        c1()
    llr, c1 = BD.carve(torch, (1, n), torch.int8, 0, BD.PAD_BYTE, "awgn llr")
    t = np.ascontiguousarray(table, dtype=np.uint32)
    _lib.check(_lib.lib().ldpc_awgn_i8_async(dec._ctx, None, C.c_void_p(llr.data_ptr()), 0, first, 42, t.ctypes.data, None))
    torch.cuda.synchronize()
    assert bool((llr.view(torch.uint8) == BD.PAD_BYTE).all())
    c1()


def test_error_counter_accumulates_and_checks_its_bounds():
    """Counters preset to (5, 7) and accumulated over two calls; k = 0, 1 and
    n; batch 0 leaves them alone; k = n + 1 and k = -1 are LDPC_EINVAL."""
    torch = _torch()
    code, B = "576x288", 6
    n = load_table(code).n
    dec = decoder(code, 0)
    hard, ref = BD.bits((B, n), 37), BD.bits((B, n), 38)
    ref[4] = hard[4]
    d_hard, ch = upload(hard, 0, "hard")
    d_ref, cr = upload(ref, 0, "ref")
    for k in (0, 1, n):
        cnt, cc = counters((5, 7))
        dec.count_errors_device(d_hard, k, cnt, ref=d_ref)
        dec.count_errors_device(d_hard, k, cnt)
        torch.cuda.synchronize()
        a, b = BD.count_reference(hard, ref, k), BD.count_reference(hard, None, k)
        assert cnt.tolist() == [5 + a[0] + b[0], 7 + a[1] + b[1]], k
        assert k == 0 or a[0] > 0
        for check in (ch, cr, cc):
            check()
    cnt, cc = counters((5, 7))
    _lib.check(_lib.lib().ldpc_count_errors_async(dec._ctx, None, C.c_void_p(d_hard.data_ptr()), 0, n,
                                                  C.c_void_p(d_ref.data_ptr()), C.c_void_p(cnt.data_ptr())))
    for k in (n + 1, -1):
        with pytest.raises(LdpcError) as e:
            dec.count_errors_device(d_hard, k, cnt, ref=d_ref)
        assert e.value.status == _lib.LDPC_EINVAL
    torch.cuda.synchronize()
    assert cnt.tolist() == [5, 7]
    cc()
