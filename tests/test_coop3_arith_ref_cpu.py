"""The scalar reference of coop3's arithmetic (tests/cpp/coop3_arith_ref.h,
compiled for the host as libc3ref_host.so) pinned against two authorities that
exist already: test_coop2_arith.ref_check (the numpy statement of SURVEY.md
8(a), here with NMS) and oracle.decode_i8 on one-check and short staircase
tables.  test_gpu_coop3_arith.py runs the same header on the device beside the
kernel's packed functions; two checkers that agree over the domain leave a
mismatch there to the kernel.  No GPU.
"""
import ctypes as C
import os

import numpy as np
import pytest

import oracle as O
import param_domain as PD
import test_coop2_arith as A2
from ldpcgputegra_amd.codes import Table

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
_lib = None


def ref_lib():
    global _lib
    if _lib is None:
        L = C.CDLL(os.path.join(ROOT, "ldpcgputegra_amd", "libc3ref_host.so"))
        P = C.c_void_p
        L.c3ref_check.argtypes = [C.c_int] * 6 + [P] * 4
        L.c3ref_chain_step.argtypes = [C.c_int] * 4 + [P] * 6
        L.c3ref_bits.argtypes = [P, C.c_int, P, P, P]
        L.c3ref_bits.restype = None
        _lib = L
    return _lib


def ref_check(params, first, v, m):
    """(new V, new messages) int8 [B, D] of c3ref::check."""
    algo, param = params.oracle
    v = np.ascontiguousarray(v, np.int8)
    m = np.ascontiguousarray(m, np.int8)
    vn, mn = np.empty_like(v), np.empty_like(m)
    rc = ref_lib().c3ref_check(int(algo == O.NMS), param, params.msg_max, int(first), v.shape[1], v.shape[0],
                               v.ctypes.data, m.ctypes.data, vn.ctypes.data, mn.ctypes.data)
    assert rc == 0
    return vn, mn


# the corners of param_domain.GRID that coop3 accepts
PARAMS = PD.IN_DOMAIN
DEGREES = (2, 3, 6, 7, 10, 27, 30)


def vectors(D, seed):
    """V over the whole int8 range with ties and the extremes, messages in -63 .. 63."""
    n = 4096
    r = PD.splitmix64(np.arange(2 * n * D, dtype=np.uint64) ^ np.uint64(0xC3A5 + seed)).reshape(2, n, D)
    v = (r[0] >> np.uint64(56)).astype(np.uint8).view(np.int8).astype(np.int64)
    small = (r[0] >> np.uint64(20)) & np.uint64(3)
    v = np.where(small == 0, v % 4, np.where(small == 1, np.sign(v) * 127, v))
    v[:8] = np.array([-128, -127, -1, 0, 1, 126, 127, 63])[:, None]
    m = (r[1] >> np.uint64(40)).astype(np.int64) % 127 - 63
    m[::3] = 0
    return v, m


@pytest.mark.parametrize("first", [True, False], ids=["first", "later"])
@pytest.mark.parametrize("p", PARAMS, ids=[p.id for p in PARAMS])
def test_reference_check_equals_numpy_statement(p, first):
    algo, param = p.oracle
    for D in DEGREES:
        v, m = vectors(D, D)
        m = np.clip(m, -p.msg_max if algo != O.NMS else -63, p.msg_max if algo != O.NMS else 63)
        ev, em = A2.ref_check(v, m, param, p.msg_max, not first, factor=param if algo == O.NMS else None)
        gv, gm = ref_check(p, first, v, m)
        bad = np.argwhere((gv != ev) | (gm != em))
        assert bad.size == 0, "c3ref::check degree %d, row %d: V %s m %s -> got %s / %s, expected %s / %s" % (
            D, bad[0][0], v[bad[0][0]], m[bad[0][0]], gv[bad[0][0]], gm[bad[0][0]], ev[bad[0][0]], em[bad[0][0]])


def layered(table, llr, iters, p):
    """The layered decode of `table` with c3ref::check as its check update: soft output int8 [B, N]."""
    V = np.array(llr, np.int8)
    msg = np.zeros((V.shape[0], table.e), np.int8)
    for _ in range(iters):
        pos = 0
        for g, (d, cnt) in enumerate(table.groups):
            for _ in range(cnt):
                var = table.edge_var[pos:pos + d].astype(np.int64)
                V[:, var], msg[:, pos:pos + d] = ref_check(p, g == 0, V[:, var], msg[:, pos:pos + d])
                pos += d
    return V


def one_check(d):
    return Table(d, 1, [(d, 1)], np.arange(d, dtype=np.uint32))


def staircase(X, m):
    """m checks in a parity staircase (X information variables each, every one
    in two checks), the last of degree X + 1: the layout of a DVB-S2 table."""
    k = m * X // 2
    chk = []
    for i in range(m):
        info = sorted((i * X + j) % k for j in range(X))
        chk.append(info + ([k + i, k + i + 1] if i < m - 1 else [k]))
    return Table(k + m, m, [(X + 2, m - 1), (X + 1, 1)], np.array([x for c in chk for x in c], dtype=np.uint32))


TABLES = {"one7": one_check(7), "one30": one_check(30), "one3": one_check(3), "stair5x6": staircase(5, 6),
          "stair8x4": staircase(8, 4)}


@pytest.mark.parametrize("iters", [2, 3])
@pytest.mark.parametrize("name", sorted(TABLES))
@pytest.mark.parametrize("p", PARAMS, ids=[p.id for p in PARAMS])
def test_reference_check_equals_oracle_decode(p, name, iters):
    t = TABLES[name]
    algo, param = p.oracle
    for kind in ("u128", "ext", "ties"):
        llr = PD.make_input(kind, 256, t.n)
        _, soft, _ = O.decode_i8(t, llr, iters, algo, param, var_min=p.var_min, msg_max=p.msg_max, return_soft=True)
        got = layered(t, llr, iters, p)
        bad = np.argwhere(got != soft)
        assert bad.size == 0, "%s %s: codeword %d variable %d: got %d, oracle %d" % (
            name, kind, bad[0][0], bad[0][1], got[tuple(bad[0])], soft[tuple(bad[0])])


@pytest.mark.parametrize("p", PARAMS, ids=[p.id for p in PARAMS])
def test_reference_chain_step_is_the_o_edge_of_a_check(p):
    """c3ref::chain_step against c3ref::check on checks whose information
    edges carry the minimum tmin and the parity eps: the o edge's new V."""
    algo, param = p.oracle
    n = 1 << 16
    r = PD.splitmix64(np.arange(5 * n, dtype=np.uint64) ^ np.uint64(0x51E9)).reshape(5, n)
    y = (r[0] % np.uint64(255)).astype(np.int64) - 127
    mx = (r[1] % np.uint64(127)).astype(np.int64) - 63
    co = (r[2] % np.uint64(255)).astype(np.int64) - 127
    tm = (r[3] % np.uint64(128)).astype(np.int64)
    eps = np.where(r[4] & np.uint64(1), -1, 1).astype(np.int64)
    # a check of degree 4 (even: no flip): info edges (eps * tm, 127), x, o; old messages 0 but the x edge's
    v = np.stack([np.where(eps < 0, -tm, tm), np.full(n, 127), y, co], axis=1)
    # eps * tm == 0 carries no sign: put the parity on the second info edge instead
    v[:, 1] = np.where((eps < 0) & (tm == 0), -127, 127)
    m = np.stack([np.zeros(n), np.zeros(n), mx, np.zeros(n)], axis=1).astype(np.int64)
    ev, _ = ref_check(p, True, v, m)
    out = np.empty(n, np.int32)
    arrs = [np.ascontiguousarray(a, np.int32) for a in (y, mx, co, tm, eps)]
    ref_lib().c3ref_chain_step(int(algo == O.NMS), param, p.msg_max, n, *[a.ctypes.data for a in arrs], out.ctypes.data)
    bad = np.argwhere(out != ev[:, 3])
    assert bad.size == 0, "chain_step (Y, m_x, c_o, tmin, eps) = %s: got %d, check %d" % (
        [int(a[bad[0][0]]) for a in arrs], out[bad[0][0]], ev[bad[0][0], 3])
