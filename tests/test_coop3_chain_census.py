"""The instruction schedule of coop3_decode<7, 6, 2> (DVB-S2 r1/2, the bench
kernel) read back from the built library with tools/isa_census.py -- counts
from the emitted ISA, not timings -- so that a compiler or source change that
undoes it is seen:

* slab waves (LDPC_C3_POST_STAGE7): the fast period's VALU count is what it
  was before the post ran new_v stage by stage (at most 199 on the post-first
  path and 203 on the pre-first path) with fewer s_nop than the edge-after-edge
  post left in the third unrolled period (14 / 12);
* the census finds the memory wave's steady periods (the regions holding its
  s_sleep and the period's 24 vector-memory instructions, not the prologue's
  18 gathers) and the chain window: 48 steps of 3 VALU in 6 blocks, each block
  with its one x-input write, 48 constant reads in all.

Skipped where the library has not been built."""
import os
import sys

import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import check_vmcnt  # noqa: E402
import isa_census  # noqa: E402

LIB = os.path.join(ROOT, "ldpcgputegra_amd", "libldpc_mi355x.so")
KERNEL = "coop3_decodeILi7ELi6ELi2ELb0ELb0ELb0E"


@pytest.fixture(scope="module")
def census():
    if not os.path.exists(LIB):
        pytest.skip("libldpc_mi355x.so is not built")
    return isa_census.coop3_census(check_vmcnt.functions(check_vmcnt.disassemble(LIB)), KERNEL)


def test_slab_fast_period_valu_and_nops(census):
    paths = census["slab_paths_per_unrolled_period"]
    assert len(paths) == 3, paths
    assert max(p["post_first"]["valu"] for p in paths) <= 199 and max(p["pre_first"]["valu"] for p in paths) <= 203, paths
    assert paths[-1]["post_first"]["nop"] < 14 and paths[-1]["pre_first"]["nop"] < 12, paths


def test_memory_wave_steady_periods_are_found(census):
    mem = census["memory_wave_periods"]
    assert len(mem) >= 3 and all(p["vmem"] == 24 and p["lds"] >= 30 for p in mem), mem


def test_chain_window_is_found(census):
    cw = census["chain_window"]
    assert cw is not None and cw["steps"] == 48 and len(cw["blocks"]) == 6, cw
    assert cw["vmem"] == 0 and cw["lds"] == 54, cw   # 48 constant reads + 6 x-input writes
    assert all(b["writes"] == 1 and 24 <= b["valu"] <= 26 for b in cw["blocks"]), cw["blocks"]
    assert cw["all"] == sum(cw[k] for k in ("valu", "salu", "lds", "vmem", "waitcnt", "nop")), cw
