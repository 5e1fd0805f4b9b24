"""The attention kernels' shared device helpers have one definition (csrc/attn_common.h), on the CPU: the forward, the short backward
and the two long backward passes must regenerate the same dropout mask bit for bit and agree on the LDS row geometry, which a second
copy of a helper in one of the .hip files could silently break."""
import glob
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "vl-pet_amd", "csrc")
ATTN_FILES = ("attn.hip", "attn_long.hip", "attn_long_bwd.hip")
SHARED = ("hash_elem", "row_key", "keep_elem", "store_rows_T", "tr_acc_order")


def _sources():
    files = sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.h")))
    assert len(files) > 30, files
    return {os.path.basename(f): open(f).read() for f in files}


def test_the_shared_helpers_are_defined_once_in_the_header():
    src = _sources()
    for name in SHARED:
        # a definition: "<qualifiers and return type> name(<parameters>) {" with nothing of an expression ('=', ';', '(') before the name
        pat = re.compile(r"^[^\n=;(]*[\w\*&>][ \t\*&]+" + name + r"\s*\([^;{}()]*\)\s*\{", re.M)
        where = [f for f, text in src.items() for _ in pat.finditer(text)]
        assert where == ["attn_common.h"], (name, where)


def test_the_attention_kernels_include_the_header():
    src = _sources()
    for f in ATTN_FILES:
        assert re.search(r'^#include "attn_common\.h"$', src[f], re.M), f
