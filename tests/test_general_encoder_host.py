"""The general GF(2) encoder on the host (csrc/genc_host.cpp): the canonical
parity / information positions of every shipped table against figures worked
out with numpy from the rule in include/ldpc_mi355x.h, the codewords against
H, against an independent numpy solve and against the IRA encoder, and the
error codes of the new entry points as far as they go without a GPU."""
import ctypes as C
import functools

import numpy as np
import pytest

from ldpcgputegra_amd import Code, Decoder, Encoder, LdpcError, _lib, load_table
from test_gpu_encoder import SMALL, write_small_table

# code -> (rank, systematic, lowest parity position or None where it was not worked out), from a numpy
# restatement of the canonical rule
FACTS = {
    "576x288": (288, True, 288), "648x324": (324, True, 324), "1200x600": (600, True, 600),
    "1248x624": (624, True, 624), "1944x972": (972, True, 972), "2304x1152": (1152, True, 1152),
    "200x100": (100, False, 90), "816x408": (408, False, 407), "1024x518": (518, False, 504),
    "4000x2000": (2000, False, None), "8000x4000": (4000, False, None), "9972x4986": (4986, False, None),
    "2048x384": (325, False, None), "4896x2448": (2422, False, None),
}
LARGE = ["16200x7560", "20000x10000"]   # 5 s and 3 s to build on the development host: 2 codewords each


@functools.lru_cache(maxsize=None)
def encoder(name):
    """One encoder per code for the whole module (read only)."""
    return Code(name).encoder()


@pytest.mark.parametrize("name", sorted(FACTS))
def test_structure(name):
    rank, systematic, lowest = FACTS[name]
    enc = encoder(name)
    n, m = enc.code.n, enc.code.m
    k = n - m
    assert (enc.n, enc.k) == (n, k)
    assert enc.rank == rank and enc.systematic == systematic
    ip, pp = enc.info_pos, enc.parity_pos
    assert ip.shape == (k,) and pp.shape == (rank,)
    assert (np.diff(ip) > 0).all() and (np.diff(pp) > 0).all()
    assert ip.min() >= 0 and pp.min() >= 0 and max(ip.max(), pp.max()) < n
    assert not set(ip.tolist()) & set(pp.tolist())
    if lowest is not None:
        assert int(pp.min()) == lowest
    if systematic:
        assert np.array_equal(ip, np.arange(k)) and np.array_equal(pp, np.arange(k, n))
    # the information positions are the K lowest columns that are no parity position
    free = np.setdiff1d(np.arange(n), pp)
    assert np.array_equal(ip, free[:k]) and free.size - k == m - rank


def check_codewords(name, batch, seed):
    enc = encoder(name)
    t = load_table(name)
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 2, size=(batch, enc.k), dtype=np.uint8)
    cw = enc.encode(a)
    assert cw.shape == (batch, t.n) and cw.dtype == np.uint8 and cw.max() <= 1
    assert np.array_equal(t.syndrome(cw), np.zeros(batch, dtype=np.int64))
    assert np.array_equal(cw[:, enc.info_pos], a)
    forced = np.setdiff1d(np.arange(t.n), np.concatenate([enc.info_pos, enc.parity_pos]))
    assert forced.size == t.m - enc.rank
    assert not cw[:, forced].any()
    return enc, a, cw, rng


@pytest.mark.parametrize("name", sorted(FACTS))
def test_codewords_satisfy_h_and_are_linear(name):
    enc, a, cw, rng = check_codewords(name, 64, seed=3)
    b = rng.integers(0, 2, size=a.shape, dtype=np.uint8)
    assert np.array_equal(cw ^ enc.encode(b), enc.encode(a ^ b))
    # bytes are taken & 1, one codeword at a time equals the batch
    assert np.array_equal(enc.encode(a | 0xFE), cw)
    assert np.array_equal(enc.encode(a[5:6]), cw[5:6])


@pytest.mark.parametrize("name", LARGE)
def test_large_codes(name):
    enc, _, _, _ = check_codewords(name, 2, seed=4)
    assert enc.rank == enc.code.m and enc.systematic


def solve_parity_numpy(t, info):
    """Independent of the library: p with H_p p = H_i u for H = [H_i | H_p],
    by Gauss-Jordan elimination of [H_p | H_i u] over GF(2), rows bit-packed
    with numpy.  H_p must be invertible (a systematic code of full rank)."""
    n, m = t.n, t.m
    k = n - m
    H = np.zeros((m, n), dtype=np.uint8)
    for r, (_, v) in enumerate(t.checks()):
        np.bitwise_xor.at(H[r], v, 1)
    rhs = (H[:, :k].astype(np.int64) @ info.T.astype(np.int64) & 1).astype(np.uint8)   # [m, batch]
    A = np.packbits(np.concatenate([H[:, k:], rhs], axis=1), axis=1)
    used = np.zeros(m, dtype=bool)
    row_of = np.empty(m, dtype=np.int64)
    for c in range(m):
        has = (A[:, c >> 3] & (0x80 >> (c & 7))) != 0
        cand = np.nonzero(has & ~used)[0]
        assert cand.size, "H_p is singular"
        pr = cand[0]
        used[pr] = True
        row_of[c] = pr
        has[pr] = False
        A[has] ^= A[pr]
    sol = np.unpackbits(A, axis=1)[:, m:m + info.shape[0]]    # row r: parity row_of^-1(r) of every codeword
    return sol[row_of].T


@pytest.mark.parametrize("name", ["576x288", "648x324", "1944x972"])
def test_systematic_codes_equal_numpy_solve(name):
    enc = encoder(name)
    t = load_table(name)
    info = np.random.default_rng(9).integers(0, 2, size=(64, enc.k), dtype=np.uint8)
    exp = np.concatenate([info, solve_parity_numpy(t, info)], axis=1)
    assert np.array_equal(enc.encode(info), exp)


@pytest.mark.parametrize("key", ["q1", "q3"])
def test_small_annex_b_tables_equal_ira_encoder(key, tmp_path):
    q, c = SMALL[key]
    write_small_table(tmp_path / (key + ".txt"), q, c, seed=17)
    code = Code(str(tmp_path / (key + ".txt")))
    enc = code.encoder()
    assert enc.systematic and enc.rank == code.m == 360 * q
    assert np.array_equal(enc.parity_pos, np.arange(code.k_info, code.n))
    info = np.random.default_rng(2).integers(0, 2, size=(7, code.k_info), dtype=np.uint8)
    assert np.array_equal(enc.encode(info), code.encode(info))


def test_small_annex_b_table_is_what_elimination_gives(tmp_path):
    """The delegation's claim: the staircase columns are the canonical parity
    positions.  The same H handed over as a plain table goes through the
    elimination and must give the same encoder."""
    q, c = SMALL["q3"]
    write_small_table(tmp_path / "q3.txt", q, c, seed=17)
    code = Code(str(tmp_path / "q3.txt"))
    plain = Code(code.table())               # ldpc_code_create: no Annex-B rows kept
    enc = plain.encoder()
    assert enc.systematic and enc.rank == code.m
    info = np.random.default_rng(3).integers(0, 2, size=(5, code.k_info), dtype=np.uint8)
    assert np.array_equal(enc.encode(info), code.encode(info))


def test_dvbs2_delegation():
    code = Code("dvbs2_r9_10")
    enc = code.encoder()
    assert enc.systematic and enc.rank == code.m
    assert np.array_equal(enc.info_pos, np.arange(code.k_info))
    info = np.random.default_rng(4).integers(0, 256, size=(3, code.k_info), dtype=np.uint8)
    assert np.array_equal(enc.encode(info), code.encode(info))


def test_dense_matrix_cap():
    """64800 x 32400 as a plain table (no Annex-B rows) is 262 MB dense: refused."""
    plain = Code(Code("dvbs2_r1_2").table())
    with pytest.raises(LdpcError) as ei:
        plain.encoder()
    assert ei.value.status == _lib.LDPC_EUNSUPPORTED
    assert "capped" in str(ei.value)


def test_errors():
    L = _lib.lib()
    enc = encoder("200x100")
    code = enc.code
    h = C.c_void_p()
    assert L.ldpc_encoder_create(None, C.byref(h)) == _lib.LDPC_EINVAL
    assert L.ldpc_encoder_create(code.handle, None) == _lib.LDPC_EINVAL
    assert L.ldpc_encoder_info(None, None, None, None, None) == _lib.LDPC_EINVAL
    assert L.ldpc_encoder_info(enc.handle, None, None, None, None) == _lib.LDPC_OK
    assert L.ldpc_encoder_positions(None, None, None) == _lib.LDPC_EINVAL
    assert L.ldpc_encoder_positions(enc.handle, None, None) == _lib.LDPC_OK
    L.ldpc_encoder_destroy(None)
    a = np.zeros(enc.k, dtype=np.uint8)
    b = np.zeros(enc.n, dtype=np.uint8)
    assert L.ldpc_encode(None, a.ctypes.data, b.ctypes.data, 1) == _lib.LDPC_EINVAL
    assert L.ldpc_encode(enc.handle, None, b.ctypes.data, 1) == _lib.LDPC_EINVAL
    assert L.ldpc_encode(enc.handle, a.ctypes.data, None, 1) == _lib.LDPC_EINVAL
    assert L.ldpc_encode(enc.handle, a.ctypes.data, b.ctypes.data, -1) == _lib.LDPC_EINVAL
    assert L.ldpc_encode(enc.handle, None, None, 0) == _lib.LDPC_OK


def test_async_entry_points_on_a_host_context():
    L = _lib.lib()
    enc = encoder("200x100")
    dec = Decoder(enc.code, device=-1, max_batch=4)
    a = np.zeros(enc.k, dtype=np.uint8)      # never dereferenced: the context is checked first
    b = np.zeros(enc.n, dtype=np.uint8)
    assert L.ldpc_encode_async(dec._ctx, None, a.ctypes.data, b.ctypes.data, 1) == _lib.LDPC_EUNSUPPORTED
    assert b"host context" in L.ldpc_last_error()
    assert L.ldpc_ctx_set_encoder(dec._ctx, enc.handle) == _lib.LDPC_EUNSUPPORTED
    assert b"host context" in L.ldpc_last_error()
    # argument checks come first
    assert L.ldpc_encode_async(None, None, a.ctypes.data, b.ctypes.data, 1) == _lib.LDPC_EINVAL
    assert L.ldpc_encode_async(dec._ctx, None, None, b.ctypes.data, 1) == _lib.LDPC_EINVAL
    assert L.ldpc_encode_async(dec._ctx, None, a.ctypes.data, None, 1) == _lib.LDPC_EINVAL
    assert L.ldpc_encode_async(dec._ctx, None, a.ctypes.data, b.ctypes.data, -1) == _lib.LDPC_EINVAL
    assert L.ldpc_ctx_set_encoder(None, enc.handle) == _lib.LDPC_EINVAL
    assert L.ldpc_ctx_set_encoder(dec._ctx, None) == _lib.LDPC_EINVAL
    dec.close()


def test_set_encoder_of_another_code():
    dec = Decoder(Code("648x324"), device=-1, max_batch=4)
    with pytest.raises(LdpcError) as ei:
        dec.set_encoder(encoder("576x288"))
    assert ei.value.status == _lib.LDPC_EINVAL and "another code" in str(ei.value)
    with pytest.raises(LdpcError) as ei:        # same shape, another H
        dec.set_encoder(Encoder(Code(permuted_648())))
    assert ei.value.status == _lib.LDPC_EINVAL
    # the same code loaded twice is the same code: only the host context stands in the way
    with pytest.raises(LdpcError) as ei:
        dec.set_encoder(Code("648x324").encoder())
    assert ei.value.status == _lib.LDPC_EUNSUPPORTED
    dec.close()


def permuted_648():
    from ldpcgputegra_amd import Table
    t = load_table("648x324")
    ev = t.edge_var.copy()
    first, last = ev == 0, ev == 647        # swap two columns of H
    ev[first], ev[last] = 647, 0
    return Table(t.n, t.m, t.groups, ev)
