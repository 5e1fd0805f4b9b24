"""What the K1 / K2 / K3 backward plans at a shape, as far as the C ABI shows it without a GPU: vlpet_bwd_workspace_bytes (with and
without a gate), vlpet_adapter_gate_bwd_form and vlpet_adapter_gate_bwd_finalize_launch over a grid of shapes.

The grid holds the boundaries of every rule behind csrc/api.hip bwd_plan and bwd_ws: 4,096, 8,192, 16,384 and 32,768 rows, the
six-block limit ((M + 127) / 128) * 6 <= 256 (5,376 / 5,377 rows), d / 64 divisible by 4 or 6, d % 128, one / three / six tiles, both
IO dtypes.  The table next to this file (bwd_plan_abi_table.json) was recorded (``python tests/test_bwd_plan_abi.py --generate``) from
the library of the commit BEFORE the choice of form moved into bwd_plan: the move must not change an answer, nor the workspace by a
byte.  Only numbers go in and come out -- no pointer is passed -- so the test runs wherever the library loads."""
import itertools
import json
import os
import sys

import pytest

MS = (1, 33, 128, 129, 4096, 4097, 5376, 5377, 8191, 8192, 8193, 16384, 16385, 18250, 28000, 32768, 32769, 46648)
DS = (64, 128, 192, 256, 384, 768, 1024, 4096)
TILES = (1, 3, 6)
IOS = (0, 1)        # VLPET_F32, VLPET_BF16
TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "bwd_plan_abi_table.json")


def shapes():
    return list(itertools.product(MS, DS, TILES, IOS))


def answers(lib, M, d, tiles, io):
    """[workspace bytes without a gate, with a gate, form, finalize launch]"""
    return [lib.vlpet_bwd_workspace_bytes(M, d, tiles, 0, io), lib.vlpet_bwd_workspace_bytes(M, d, tiles, 1, io),
            lib.vlpet_adapter_gate_bwd_form(M, d, tiles, io), lib.vlpet_adapter_gate_bwd_finalize_launch(M, d, tiles, io)]


def load_table():
    with open(TABLE) as f:
        return json.load(f)


def key(M, d, tiles, io):
    return f"{M},{d},{tiles},{io}"


@pytest.mark.parametrize("tiles", TILES)
@pytest.mark.parametrize("io", IOS)
def test_plan_answers_are_the_recorded_ones(tiles, io):
    from vlpet_amd import _lib
    lib, table = _lib.load(), load_table()
    bad = {}
    for M, d, t, i in shapes():
        if (t, i) != (tiles, io):
            continue
        got = answers(lib, M, d, t, i)
        if got != table[key(M, d, t, i)]:
            bad[key(M, d, t, i)] = (got, table[key(M, d, t, i)])
    assert not bad, f"{len(bad)} shapes differ (got, recorded): {dict(list(bad.items())[:8])}"


def test_table_is_the_whole_grid_and_reaches_every_answer():
    """Every combination the entry check accepts is in the table (the grid has none it refuses), and the rows are not vacuous: each
    form and both finalize answers occur, and a gate costs workspace everywhere."""
    table = load_table()
    assert sorted(table) == sorted(key(*s) for s in shapes())
    rows = list(table.values())
    assert {r[2] for r in rows} == {0, 1, 2} and {r[3] for r in rows} == {0, 1}
    assert all(0 < r[0] < r[1] for r in rows)
    assert any(r[2] == 2 and r[3] == 0 for r in rows) and any(r[2] == 2 and r[3] == 1 for r in rows)


if __name__ == "__main__" and "--generate" in sys.argv:
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from vlpet_amd import _lib
    lib = _lib.load()
    out = {key(*s): answers(lib, *s) for s in shapes()}
    assert all(v[0] > 0 and v[2] >= 0 and v[3] >= 0 for v in out.values()), "the entry check refused a grid shape"
    with open(TABLE, "w") as f:
        f.write("{\n" + ",\n".join(f'"{k}": {json.dumps(v)}' for k, v in out.items()) + "\n}\n")
    print(f"{len(out)} shapes -> {TABLE}")
