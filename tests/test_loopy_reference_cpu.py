"""No GPU: pins tests/loopy_reference.py, the yardstick of the loopy graph
retrograde (gm_graph_solve_loopy), to graph_reference on
graphs without cycles and to the five hand graphs of the design; then the
host side of the feature: the launcher's refusals, the exported symbol and
its header text, and the loopy game file's graph."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from graph_reference import DRAW, LOSS, TIE, UNDECIDED, WIN, GraphCycle, NoMoves, solve_graph
from loopy_reference import HAND_GRAPHS, csr, solve_loopy

GAMES = os.path.join(ROOT, "tests", "games")


def _load(path):
    from gamesmanmpi_amd.solver_launcher import ensure_src_utils, load_game
    ensure_src_utils()
    return load_game(path)


def test_acyclic_grid_tictactoe_equals_graph_reference():
    from gamesmanmpi_amd.generic import enumerate_game
    g = enumerate_game(_load(os.path.join(GAMES, "grid_tictactoe.py")))
    words, counts = solve_loopy(g.prim, g.offsets, g.children)
    assert words == solve_graph(g.prim, g.offsets, g.children)
    assert counts == (g.n, 0, 0, 0) and g.n == 5478


def test_acyclic_sum_game_equals_graph_reference():
    from gamesmanmpi_amd.generic import enumerate_game
    import gamesmanmpi_amd.games.sum_four_to_one as mod
    _load(os.path.join(ROOT, "gamesmanmpi_amd", "games", "sum_four_to_one.py"))
    saved = mod.HEAPS
    try:
        mod.HEAPS = (7, 7, 7, 7)
        g = enumerate_game(mod)
    finally:
        mod.HEAPS = saved
    words, counts = solve_loopy(g.prim, g.offsets, g.children)
    assert words == solve_graph(g.prim, g.offsets, g.children)
    assert counts == (8 ** 4, 0, 0, 0)


@pytest.mark.parametrize("k", range(len(HAND_GRAPHS)))
def test_hand_graphs_word_for_word(k):
    prim, kids, words, counts = HAND_GRAPHS[k]
    p, off, ch = csr(prim, kids)
    assert solve_loopy(p, off, ch) == (words, counts)
    assert sum(counts) == len(prim)
    with pytest.raises(GraphCycle):  # each of them has a cycle: the old rule refuses it
        solve_graph(p, off, ch)


def test_hand_graphs_say_what_the_design_says():
    w4, w5 = HAND_GRAPHS[3][2], HAND_GRAPHS[4][2]
    assert w4[5] == (TIE | 2 << 2) and w4[0] == (TIE | 1 << 2)  # founded: the largest; unfounded: the least
    assert w5[0] == (WIN | 3 << 2) and w5[2] == (LOSS | 4 << 2) and w5[1] == (LOSS | 2 << 2)


def test_two_cycle_and_self_loop_are_draws():
    from gamesmanmpi_amd.generic import enumerate_game
    g = enumerate_game(_load(os.path.join(GAMES, "two_cycle.py")))
    assert solve_loopy(g.prim, g.offsets, g.children) == ([3, 3, 3], (0, 0, 0, 3))
    assert solve_loopy(*csr([UNDECIDED], {0: [0]})) == ([DRAW], (0, 0, 0, 1))


def test_undecided_leaf_stays_an_error():
    with pytest.raises(NoMoves):
        solve_loopy(*csr([UNDECIDED, UNDECIDED, UNDECIDED], {0: [1, 2], 1: [0]}))


def test_duplicate_children_count_twice():
    """0 -> 1, 1, 2 with 1 a WIN (through a LOSS leaf) and 2 -> 0: position 0
    is not LOSS while its child 2 is open, however often 1 is listed."""
    words, counts = solve_loopy(*csr([4, 4, 4, 1], {0: [1, 1, 2], 1: [3], 2: [0]}))
    assert words == [3, WIN | 1 << 2, 3, LOSS] and counts == (2, 0, 0, 2)
    # 2 -> 0, 3: 2 is an unfounded WIN in 1, and then all three child slots of 0 are WIN
    words, counts = solve_loopy(*csr([4, 4, 4, 1], {0: [1, 1, 2], 1: [3], 2: [0, 3]}))
    assert words == [LOSS | 2 << 2, WIN | 1 << 2, WIN | 1 << 2, LOSS] and counts == (2, 2, 0, 0)


def test_cat_and_mouse_graph():
    """The loopy game file: under 5,000 positions, all four values, a DRAW,
    and an unfounded WIN of remoteness >= 3."""
    from gamesmanmpi_amd.generic import enumerate_game
    g = enumerate_game(_load(os.path.join(GAMES, "cat_and_mouse.py")))
    assert 100 < g.n < 5000
    with pytest.raises(GraphCycle):
        solve_graph(g.prim, g.offsets, g.children)
    words, counts = solve_loopy(g.prim, g.offsets, g.children)
    w = np.array(words, np.uint32)
    val, rem = w & 3, w >> 2
    assert set(val.tolist()) == {WIN, LOSS, TIE, DRAW}
    assert sum(counts) == g.n and counts[3] == int((val == DRAW).sum()) > 0
    assert (rem[val == DRAW] == 0).all()
    # founded positions: those a DAG-only pass reaches; a WIN in >= 3 outside them
    founded = np.zeros(g.n, bool)
    founded[g.prim != UNDECIDED] = True
    while True:
        more = [i for i in np.flatnonzero(~founded)
                if founded[g.children[g.offsets[i]:g.offsets[i + 1]]].all()]
        if not more:
            break
        founded[more] = True
    assert founded.sum() == counts[0]
    assert ((val == WIN) & ~founded & (rem >= 3)).any()


# ---- the host side ------------------------------------------------------------
def test_launcher_refuses_loopy_with_a_descriptor_layout():
    from gamesmanmpi_amd import solver_launcher as sl
    game = os.path.join(ROOT, "gamesmanmpi_amd", "games", "sum_four_to_one.py")
    for extra in ([], ["--layout", "dense"], ["--layout", "hashed"]):
        with pytest.raises(SystemExit) as e:
            sl.main([game, "--loopy", "--no-verify"] + extra)
        assert "--loopy" in str(e.value)
    a = sl.build_parser().parse_args(["g.py", "--loopy"])
    assert a.loopy and not sl.build_parser().parse_args(["g.py"]).loopy
    sl.check_loopy_args(a, descriptor=False)                       # no descriptor: the graph path
    a.layout = "graph"
    sl.check_loopy_args(a)                                         # a descriptor game on the graph path
    a.loopy, a.layout = False, "dense"
    sl.check_loopy_args(a)


def test_symbol_is_exported_and_documented():
    import ctypes
    from gamesmanmpi_amd import _lib
    assert "gm_graph_solve_loopy" in _lib.EXPORTS
    fn = _lib.load().gm_graph_solve_loopy
    assert len(fn.argtypes) == 10 and fn.argtypes[-1] == ctypes.POINTER(ctypes.c_uint64)
    assert fn.argtypes[:9] == _lib.load().gm_graph_solve.argtypes
    with open(os.path.join(ROOT, "include", "gamesman.h")) as f:
        text = f.read()
    decl = re.search(r"int gm_graph_solve_loopy\(([^;]*)\);", text)
    assert decl and "uint64_t counts[4]" in decl.group(1)
    doc = text[text.index("The same graph, cycles allowed"):decl.start()]
    for rule in ("  A  ", "  B  ", "  C  ", "  D  "):
        assert rule in doc
    assert "GM_DRAW in 0" in doc and "LEAST" in doc and "2 n + 8" in doc
    from gamesmanmpi_amd.generic import loopy_scratch_bytes
    assert "#define GM_GRAPH_LOOPY_SCRATCH_BYTES(n) (4096 + 8 * (uint64_t)(n))" in text
    assert loopy_scratch_bytes(1000) == 4096 + 8000


def test_loopy_is_off_by_default():
    import inspect
    from gamesmanmpi_amd import generic
    assert inspect.signature(generic.solve_module).parameters["loopy"].default is False
    assert inspect.signature(generic.GenericSolver.__init__).parameters["loopy"].default is False
