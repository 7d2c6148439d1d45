"""The kernel families are named once: the LDPC_KERNEL_* enumerators of
include/ldpc_mi355x.h and Decoder.KERNEL_NAMES carry the same numbers and,
lower-cased, the same names; the retired 4 and 6 are no enumerators."""
import os
import re

from conftest import ROOT
from ldpcgputegra_amd.decoder import Decoder

# enumerator (lower-cased, prefix dropped) -> KERNEL_NAMES string, where they differ
NAME_MAP = {"auto": "none", "windowed2": "windowed2_s16"}


def header_enumerators():
    txt = open(os.path.join(ROOT, "include", "ldpc_mi355x.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    body = re.search(r"typedef\s+enum\s+ldpc_kernel\s*\{(.*?)\}\s*ldpc_kernel\s*;", txt, flags=re.S).group(1)
    items = [e.strip() for e in body.split(",") if e.strip()]
    pairs = [re.fullmatch(r"LDPC_KERNEL_([A-Z0-9_]+)\s*=\s*(\d+)", e) for e in items]
    assert all(pairs), items
    return {m.group(1): int(m.group(2)) for m in pairs}


def test_header_enum_matches_kernel_names():
    enum = header_enumerators()
    assert enum == {"AUTO": 0, "GENERIC": 1, "WINDOWED": 2, "WINDOWED2": 3, "COOP": 5, "LDS": 7, "COOP3": 8,
                    "LDSEP": 9, "HOST": 10, "STAIRF": 11}
    assert len(set(enum.values())) == len(enum)
    for name, value in enum.items():
        lower = name.lower()
        assert Decoder.KERNEL_NAMES[value] == NAME_MAP.get(lower, lower), name
    # every name the Python side knows is an enumerator, except the two retired families
    assert set(Decoder.KERNEL_NAMES) - set(enum.values()) == {4, 6}


def test_retired_families_are_not_enumerators():
    assert not {4, 6} & set(header_enumerators().values())
    assert Decoder.KERNEL_NAMES[4] == "windowed2_s32" and Decoder.KERNEL_NAMES[6] == "coop2"
