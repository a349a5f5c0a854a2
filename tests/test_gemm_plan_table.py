"""dp_gemm_plan against its recorded plan table (host only: the planner runs without a device).

tests/golden/gemm_plan_table.npz holds (rc, tile, grid) of every row of the list that
tools/gemm_plan_table.py generates -- the frame's launches and perturbations around them, under
every tile hint, with and without a workspace, and under each planner-read debug bit -- as the
library answered when the table was last recorded.  The planner must answer the same, row for row:
a pull request that re-routes a launch on purpose re-records the table
(python tools/gemm_plan_table.py --write), and its diff shows which launches moved.
"""

import functools

import numpy as np

from depth_pro import _lib
from tools import gemm_plan_table as gpt


@functools.lru_cache(maxsize=None)
def planned():
    rows = gpt.Rows()
    return (rows,) + rows.plan(_lib.load())[:3]


@functools.lru_cache(maxsize=None)
def table():
    t = np.load(gpt.TABLE)
    return {k: t[k] for k in t.files}


def test_table_was_recorded_for_this_list():
    rows = planned()[0]
    assert str(table()["digest"]) == rows.digest(), "the generated list changed: re-record the table"
    assert table()["rc"].dtype == np.int8 and table()["tile"].dtype == np.int8 and table()["grid"].dtype == np.int32
    assert len(table()["rc"]) == len(table()["tile"]) == len(table()["grid"]) == len(rows.problem)


def test_planner_answers_as_recorded():
    rows, rc, tile, grid = planned()
    n, lines = gpt.differences(rows, table(), rc, tile, grid)
    assert n == 0, f"{n} of {len(rc)} launches plan differently (was -> is), the first:\n" + "\n".join(lines)


def test_table_covers_the_planner():
    """The recorded table itself: every engine DP_TILE_AUTO can choose, every error code, every hint accepted."""
    rows, t = planned()[0], table()
    rc, tile, hint = t["rc"], t["tile"], rows.hint
    assert len(gpt.AUTO_TILES) == 16
    for name in gpt.AUTO_TILES:
        want = getattr(_lib, "DP_TILE_" + name)
        assert ((hint == 0) & (rc == 0) & (tile == want)).any(), f"DP_TILE_AUTO never plans {name}"
    for code in (1000, 1001, 1002, 1003):
        assert (rc == gpt.RC_CODE[code]).any(), f"no row returns {code}"
    for h in range(1, gpt.N_TILES):
        assert ((hint == h) & (rc == 0) & (tile >= 0)).any(), f"hint {h} is never accepted"
    for bit in gpt.DEBUG_BITS:
        assert (rows.dbg == bit).any()
    assert set(np.unique(rows.ws)) == {0, 1}
