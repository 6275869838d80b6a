"""Pin tests/graph_reference.py (the CPU yardstick of the explicit-graph
retrograde) to the golden tables: tic-tac-toe from the reference's own module
and the Connect Four 3x3 / connect-3 fixture, each from the host enumeration
of the game file, and the errors it must raise."""
import os

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, load_table
from graph_reference import (DRAW, LOSS, TIE, UNDECIDED, WIN, GraphCycle, NoMoves, reduce_children, solve_graph)

GAMES = os.path.join(ROOT, "tests", "games")


def _load(path):
    from gamesmanmpi_amd.solver_launcher import ensure_src_utils, load_game
    ensure_src_utils()
    return load_game(path)


def test_reference_reproduces_tic_tac_toe_golden(golden_summary):
    from gamesmanmpi_amd.generic import enumerate_game
    g = enumerate_game(_load(os.path.join(GAMES, "grid_tictactoe.py")), keep_positions=True)
    w = np.array(solve_graph(g.prim, g.offsets, g.children), np.uint32)
    info = golden_summary["tic_tac_toe_np"]
    assert (g.n, g.edges) == (info["positions"], info["edges"])
    assert "%s in %d moves" % (("WIN", "LOSS", "TIE", "DRAW")[w[0] & 3], w[0] >> 2) == info["root_line"]
    t = load_table("tic_tac_toe_np")
    canon = [np.asarray(p, np.int8).tobytes() for p in g.positions]
    order = sorted(range(g.n), key=lambda i: canon[i])
    np.testing.assert_array_equal((w & 3)[order], t["value"])
    np.testing.assert_array_equal((w >> 2)[order], t["remoteness"])


def test_reference_reproduces_connect_four_3x3_fixture():
    from gamesmanmpi_amd.generic import enumerate_game
    mod = _load(os.path.join(ROOT, "gamesmanmpi_amd", "games", "connect_four.py"))
    mod.length, mod.height, mod.connect = 3, 3, 3
    g = enumerate_game(mod)
    w = np.array(solve_graph(g.prim, g.offsets, g.children), np.uint32)
    z = np.load(os.path.join(GOLDEN, "connect_four", "3x3_3.npz"))
    keys = []
    for name in g.names:  # the fixture's key: X plane in bits [0, 9), O plane in bits [9, 18)
        keys.append(sum(1 << i for i, c in enumerate(name) if c == "X")
                    + sum(1 << (9 + i) for i, c in enumerate(name) if c == "O"))
    order = np.argsort(np.array(keys, np.uint64))
    np.testing.assert_array_equal(np.array(keys, np.uint64)[order], z["keys"])
    np.testing.assert_array_equal((w & 3)[order], z["value"])
    np.testing.assert_array_equal((w >> 2)[order], z["remoteness"])
    np.testing.assert_array_equal(np.diff(g.offsets)[order], z["nchild"])
    assert set((w & 3).tolist()) == {WIN, LOSS, TIE}


def test_reference_raises_on_a_cycle():
    from gamesmanmpi_amd.generic import enumerate_game
    g = enumerate_game(_load(os.path.join(GAMES, "two_cycle.py")))
    with pytest.raises(GraphCycle):
        solve_graph(g.prim, g.offsets, g.children)
    with pytest.raises(GraphCycle):  # a position that is its own child
        solve_graph([UNDECIDED, LOSS], [0, 2, 2], [1, 0])


def test_reference_raises_on_an_undecided_leaf():
    with pytest.raises(NoMoves):
        solve_graph([UNDECIDED, UNDECIDED], [0, 1, 1], [1])


def test_reducers_by_hand():
    """The reducers on hand-worked children, the pairings of
    src/process.py:199-220 among them."""
    assert reduce_children([(WIN, 0)]) == (LOSS, 1)
    assert reduce_children([(LOSS, 4)]) == (WIN, 5)
    assert reduce_children([(WIN, 9), (LOSS, 4), (LOSS, 2), (TIE, 0)]) == (WIN, 3)   # least LOSS, the rest dropped
    assert reduce_children([(WIN, 9), (WIN, 3)]) == (LOSS, 10)                         # every move loses: the longest
    assert reduce_children([(TIE, 1), (WIN, 7)]) == (TIE, 8)                           # the WIN child's remoteness counts
    assert reduce_children([(DRAW, 0), (TIE, 2), (WIN, 1)]) == (TIE, 3)                # TIE before DRAW
    assert reduce_children([(DRAW, 0), (WIN, 5)]) == (DRAW, 6)
    assert reduce_children([(LOSS, 3), (LOSS, 3)]) == (WIN, 4)                         # a child listed twice
    # a deep chain: no recursion limit in the way
    n = 5000
    w = solve_graph([UNDECIDED] * (n - 1) + [LOSS], list(range(n)) + [n - 1], list(range(1, n)))
    assert w[0] == ((n - 1) % 2 == 0) * LOSS | (n - 1) << 2
