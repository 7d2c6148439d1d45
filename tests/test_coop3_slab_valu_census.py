"""Slab-wave instruction counts of coop3_decode<7, 6, 2> (DVB-S2 r1/2, the
bench kernel) after the trim of DESIGN.md §8 r09, read back from the built
library with tools/isa_census.py and set against the census of the parent
commit built with the same compiler (profiles/r09_parent_isa_census.json,
taken with the same tool; the parent has no pass-through branch, so its
*_skip paths equal its full paths):

* every slab path of every unrolled steady period -- the path of a wave that
  runs the pre's pass-through block -- has at least 4 VALU fewer than the
  parent's (three packed unsigned saturating subtracts for max(x - coff, 0),
  one multiply for eps * m_x);
* the path of a wave that branches around the block has at least 9 fewer;
* no path has more s_nop than the parent's.

Skipped where the library has not been built."""
import json
import os
import sys

import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import check_vmcnt  # noqa: E402
import isa_census  # noqa: E402

LIB = os.path.join(ROOT, "ldpcgputegra_amd", "libldpc_mi355x.so")
KERNEL = "coop3_decodeILi7ELi6ELi2ELb0ELb0ELb0E"
PARENT = os.path.join(ROOT, "profiles", "r09_parent_isa_census.json")
KINDS = ("post_first", "pre_first")


@pytest.fixture(scope="module")
def paths():
    if not os.path.exists(LIB):
        pytest.skip("libldpc_mi355x.so is not built")
    cur = isa_census.coop3_census(check_vmcnt.functions(check_vmcnt.disassemble(LIB)), KERNEL)
    with open(PARENT) as f:
        par = json.load(f)
    cur, par = cur["slab_paths_per_unrolled_period"], par["slab_paths_per_unrolled_period"]
    assert len(cur) == len(par) == 3, (cur, par)
    return cur, par


def test_parent_census_is_the_parents(paths):
    """The committed figures are the ones DESIGN.md §8 (r08a) and the chain
    census test quote for the parent: 198 / 199 / 199 and 199 / 202 / 203."""
    _, par = paths
    assert [p["post_first"]["valu"] for p in par] == [198, 199, 199]
    assert [p["pre_first"]["valu"] for p in par] == [199, 202, 203]
    assert all(p["pass_through_branches"] == 0 for p in par)


def test_every_path_has_4_valu_fewer(paths):
    cur, par = paths
    for c, p in zip(cur, par):
        for k in KINDS:
            print(k, "valu", c[k]["valu"], "parent", p[k]["valu"])
            assert c[k]["valu"] <= p[k]["valu"] - 4, (k, c, p)


def test_paths_around_the_pass_through_block_have_9_fewer(paths):
    cur, par = paths
    for c, p in zip(cur, par):
        assert c["pass_through_branches"] == 2, c   # one per pre of the two fast paths
        for k in KINDS:
            print(k, "valu without the block", c[k + "_skip"]["valu"], "parent", p[k]["valu"])
            assert c["pt_valu"][k] >= 6, c
            assert c[k + "_skip"]["valu"] <= p[k]["valu"] - 9, (k, c, p)


def test_no_more_nops_than_the_parent(paths):
    cur, par = paths
    for c, p in zip(cur, par):
        for k in KINDS:
            print(k, "s_nop", c[k]["nop"], "parent", p[k]["nop"])
            assert c[k]["nop"] <= p[k]["nop"] and c[k + "_skip"]["nop"] <= p[k]["nop"], (k, c, p)
