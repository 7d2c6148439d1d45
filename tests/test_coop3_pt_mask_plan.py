"""The pass-through mask of the coop3 schedule (no GPU): in steady periods only
the slab waves named in Coop3Host::pt_mask run the pre's pass-through block,
so every inactive slot of every window but the tail's has to lie in one of
them.  Replayed here from the kernel's final records (ldpc_code_coop3_slots)
for every packaged code that has a coop3 schedule; DVB-S2 r1/2 (windows of
about 45 checks in 48 slots, the inactive slots last) needs one wave only."""
import numpy as np
import pytest

from ldpcgputegra_amd import Code
from ldpcgputegra_amd.codes import available

COOP3 = ("dvbs2_r1_2", "dvbs2_r2_3", "dvbs2shape_r3_4", "dvbs2shape_r5_6", "dvbs2_r8_9", "dvbs2_r9_10")

_slots = {}


def slots(name):
    if name not in _slots:
        _slots[name] = Code(name).coop3_slots()
    return _slots[name]


@pytest.mark.parametrize("name", sorted(available()))
def test_inactive_slots_lie_in_masked_waves(name):
    s = slots(name)
    assert (s is not None) == (name in COOP3)
    if s is None:
        return
    act, spw, mask = s["active"], s["slots_per_wave"], s["pt_mask"]
    assert act.shape == (s["windows"], s["S"]) and s["S"] % spw == 0 and 0 <= s["tail"] < s["windows"]
    assert mask >> (s["S"] // spw) == 0
    seen = 0
    for u in range(s["windows"]):
        if u == s["tail"]:
            continue
        for k in np.flatnonzero(act[u] == 0):
            assert (mask >> (k // spw)) & 1, (name, u, int(k), hex(mask))
            seen |= 1 << (k // spw)
    assert seen == mask   # and no wave is named for nothing
    assert act[s["tail"]].sum() >= 1


def test_r12_mask_is_one_wave():
    s = slots("dvbs2_r1_2")
    assert s["S"] == 48 and s["slots_per_wave"] == 8
    assert bin(s["pt_mask"]).count("1") == 1, hex(s["pt_mask"])
