"""Synthetic quasi-cyclic tables in the two compiled shapes of kernel family 9
(the edge-parallel kernels, csrc/ldsep_common.h: 12 layers x up to 4 passes of
8 checks, 11 layers x up to 6 passes), shared by test_f16_ep_cpu.py and
test_gpu_f16_ep.py.  A plain helper module, built like short_domain.synthetic.

* 12 block rows over 24 column blocks, the first six rows of check degree d,
  the last six of max(2, d - 1), d = 2 .. 8, at
    Z = 8    one exactly full pass (the other three passes of the shape empty),
    Z = 27   four passes, the last with 3 live and 5 empty check slots,
    Z = 32   four full passes;
* 11 block rows (six of degree d, five of max(2, d - 1)) over 24 column blocks
  at Z = 41: six passes, the last holding one check.

The smallest tables at which padding lanes (d = 2: six per check), empty check
slots and both compiled shapes are all exercised."""
import numpy as np

import param_domain as PD
from ldpcgputegra_amd.codes import Table

COL_BLOCKS = 24
DEGREES = tuple(range(2, 9))
SHAPES = ((12, 8), (12, 27), (12, 32), (11, 41))      # (block rows, Z)
FIRST_ROWS = 6                                        # block rows of degree d; the rest have max(2, d - 1)
_tables = {}


def synthetic(d, rows, Z):
    """Table of a quasi-cyclic code with N = 24 Z.  Check i of block row r uses
    the variables Z cb_j + (i + s_j) mod Z of deg distinct column blocks cb_j:
    column block 0 (every block row covers it whole, so consecutive block rows
    never merge into one layer) and the first deg - 1 of the others in the
    order of their splitmix64 values, keyed like the shifts s_j by
    (d, rows, Z, r).  A block row is one layer of Z checks sharing no variable."""
    key_ = (d, rows, Z)
    if key_ not in _tables:
        assert 2 <= d <= 8 and FIRST_ROWS < rows
        low = max(2, d - 1)
        groups = [(d, FIRST_ROWS * Z), (low, (rows - FIRST_ROWS) * Z)]
        edges = []
        for r in range(rows):
            deg = d if r < FIRST_ROWS else low
            key = np.uint64((d << 44) | (rows << 36) | (Z << 20) | (r << 8))
            draw = PD.splitmix64(key + np.arange(2 * COL_BLOCKS, dtype=np.uint64))
            others = [int(c) for c in np.argsort(draw[:COL_BLOCKS], kind="stable") if int(c) != 0]
            cb = np.array([0] + others[:deg - 1], dtype=np.int64)
            s = (draw[COL_BLOCKS:COL_BLOCKS + deg] % np.uint64(Z)).astype(np.int64)
            i = np.arange(Z, dtype=np.int64)[:, None]
            edges.append((Z * cb[None, :] + (i + s[None, :]) % Z).ravel())
        _tables[key_] = Table(COL_BLOCKS * Z, rows * Z, groups, np.concatenate(edges).astype(np.uint32))
    return _tables[key_]


def synthetic_name(d, rows, Z):
    return "ep_d%d_r%d_z%d" % (d, rows, Z)


ALL = [(d, rows, Z) for rows, Z in SHAPES for d in DEGREES]
