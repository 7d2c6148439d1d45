"""Which kernel family every decode request ends up on, as one table.

For six codes, seven parameter sets, two batch sizes (16 and 65: stride 64 and
128) and every requested kernel 0 .. 11, one context per code takes the
requests in a fixed order and a recorder notes, per request: the status of
set_kernel, the status of the decode, whether the decode's error message says
"not applicable", and last_kernel, last_skipped, last_et_stage and
last_lds_shape afterwards -- on success and on failure (a rejected set_kernel
leaves the previous request's kernel in force, and the row shows that).

The expected rows, tests/golden/selection_table.json, were recorded with this
recorder on the build before the decode dispatcher was split into selection,
scratch plan and launch bodies; `python tests/test_gpu_selection_table.py`
on a GPU regenerates the file.  Outputs are not compared here: the parity,
configs and domain suites do that.
"""
import ctypes as C
import json
import os

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "selection_table.json")

CODES = ("576x288", "2048x384", "20000x10000", "16200x7560", "dvbs2_r1_2", "dvbs2_r8_9")
# (name, float, ldpc_params fields on top of the entry point's defaults)
CASES = (
    ("i8", False, {}),
    ("i8_msg_max_100", False, {"msg_max": 100}),
    ("i8_nms", False, {"algo": 1}),
    ("i8_var_min_-128", False, {"var_min": -128}),
    ("i8_early", False, {"early_term": 1}),
    ("f32", True, {}),
    ("f32_early", True, {"early_term": 1}),
)
BATCHES = (16, 65)
KERNELS = tuple(range(12))
MAX_BATCH, ITERS, SEED, EBN0 = 128, 1, 20260, 2.0
COLUMNS = ("case", "batch", "kernel", "set_kernel_status", "decode_status", "not_applicable", "last_kernel",
           "last_skipped", "last_et_stage", "lds_lanes", "lds_split")


def _getters(dec):
    from ldpcgputegra_amd import _lib
    L, out = _lib.lib(), []
    for fn in (L.ldpc_ctx_last_kernel, L.ldpc_ctx_last_skipped, L.ldpc_ctx_last_et_stage):
        k = C.c_int()
        _lib.check(fn(dec._ctx, C.byref(k)))
        out.append(k.value)
    lanes, split = C.c_int(), C.c_int()
    _lib.check(L.ldpc_ctx_last_lds_shape(dec._ctx, C.byref(lanes), C.byref(split)))
    return out + [lanes.value, split.value]


def record(code):
    """The rows of one code (lists in COLUMNS order), all on one context."""
    import torch
    from ldpcgputegra_amd import ALGO_MS, Code, Decoder, LdpcError, channel, default_params, load_table
    t = load_table(code)
    table = channel.i8_table(channel.sigma_from_ebn0(EBN0, t.k_info / t.n))
    dec = Decoder(Code(code), max_batch=MAX_BATCH)
    llr_i8 = torch.empty((max(BATCHES), t.n), dtype=torch.int8, device="cuda")
    dec.awgn_i8_device(llr_i8, 0, SEED, table)
    llr_f32 = llr_i8.float()
    hard = torch.empty((max(BATCHES), t.n), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    rows = []
    for name, is_float, fields in CASES:
        p = default_params(algo=ALGO_MS, **fields) if is_float else default_params(**fields)
        for batch in BATCHES:
            for kernel in KERNELS:
                set_status = decode_status = 0
                not_applicable = False
                try:
                    dec.set_kernel(kernel)
                except LdpcError as e:
                    set_status = e.status
                try:
                    if is_float:
                        dec.decode_f32_device(llr_f32[:batch], hard[:batch], ITERS, params=p)
                    else:
                        dec.decode_i8_device(llr_i8[:batch], hard[:batch], ITERS, params=p)
                except LdpcError as e:
                    decode_status = e.status
                    not_applicable = "not applicable" in str(e)
                torch.cuda.synchronize()   # a kernel fault ends the recording here
                rows.append([name, batch, kernel, set_status, decode_status, not_applicable] + _getters(dec))
    dec.close()
    return rows


def _expected():
    with open(FIXTURE) as f:
        return json.load(f)


@pytest.mark.gpu
@pytest.mark.parametrize("code", CODES)
def test_selection_table(code):
    fixture = _expected()
    assert tuple(fixture["columns"]) == COLUMNS
    expected, got = fixture["rows"][code], record(code)
    assert len(expected) == len(CASES) * len(BATCHES) * len(KERNELS) == len(got)
    for exp, row in zip(expected, got):
        assert row == exp, "%s: %s" % (code, dict(zip(COLUMNS, row)))


if __name__ == "__main__":
    import sys
    sys.path.insert(0, os.path.dirname(HERE))
    out = sys.argv[1] if len(sys.argv) > 1 else FIXTURE
    table = {"columns": list(COLUMNS), "rows": {}}
    for code_name in CODES:
        table["rows"][code_name] = record(code_name)
        print(code_name, len(table["rows"][code_name]), "rows", flush=True)
    with open(out, "w") as f:
        f.write('{"columns": %s,\n "rows": {\n' % json.dumps(table["columns"]))
        f.write(",\n".join('  "%s": [\n%s\n  ]' % (c, ",\n".join("   " + json.dumps(r) for r in table["rows"][c]))
                           for c in CODES))
        f.write("\n }}\n")
