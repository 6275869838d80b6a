"""Connect Four in the RANKED layout (csrc/gm_ranked_connect.h, layout=
"ranked") on the GPU, against the same yardsticks as the keyed layouts
(test_gpu_connect_four.py): the game file solved through the graph path, the
fixtures generated from the module, and the BUCKETED solve's checksum."""
import io
import json
from contextlib import redirect_stdout

import numpy as np
import pytest

from test_connect_four_cpu import GAME_FILE, c4_summary, c4_table
from test_connect_four_ranked_cpu import NON_POSITIONS_4x4
from test_gpu_connect_four import WORD_BOARDS, graph_words, name_of, solved, sorted_dump, spec_of

pytestmark = pytest.mark.gpu


def golden_words(t):
    return t["value"].astype(np.uint32) | (t["remoteness"].astype(np.uint32) << 2)


@pytest.mark.parametrize("board", WORD_BOARDS)
def test_single_table_word_for_word(board):
    keys, words, gr = graph_words(board)
    s, r = solved(board, "ranked")
    assert (r.positions, r.edges, r.primitives, r.root_line) == (gr.positions, gr.edges, gr.primitives, gr.root_line)
    info = c4_summary()[name_of(board)]
    assert (r.positions, r.edges, r.root_line) == (info["positions"], info["edges"], info["root_line"])
    k, w = sorted_dump([s.dump()])
    np.testing.assert_array_equal(k, keys)
    np.testing.assert_array_equal(w, words)
    if board == (4, 4, 4):  # the committed table
        t = c4_table(name_of(board))
        np.testing.assert_array_equal(k, t["keys"])
        np.testing.assert_array_equal(w, golden_words(t))


@pytest.mark.parametrize("board", [(2, 2, 2), (3, 2, 3), (1, 4, 4), (4, 1, 4)])
def test_degenerate_boards(board):
    """every level below 6: the per-slot forward; C <= H and H = 1"""
    info = c4_summary()[name_of(board)]
    s, r = solved(board, "ranked")
    assert (r.positions, r.edges, r.primitives, r.root_line) == (
        info["positions"], info["edges"], info["primitives"], info["root_line"])
    t = c4_table(name_of(board))
    k, w = sorted_dump([s.dump()])
    np.testing.assert_array_equal(k, t["keys"])
    np.testing.assert_array_equal(w, golden_words(t))


def test_columns_no_more_than_rows():
    """(3,4,3): C < H, the loop form of the plane spread, against the module"""
    from gamesmanmpi_amd.generic import GenericSolver
    from test_connect_four_cpu import c4_graph, py_key
    board = (3, 4, 3)
    g = GenericSolver(c4_graph(*board))
    gr = g.solve()
    names, val, rem = g.dump()
    keys = np.array([py_key(n) for n in names], np.uint64)
    order = np.argsort(keys)
    s, r = solved(board, "ranked")
    assert (r.positions, r.edges, r.primitives, r.root_line) == (gr.positions, gr.edges, gr.primitives, gr.root_line)
    k, w = sorted_dump([s.dump()])
    np.testing.assert_array_equal(k, keys[order])
    np.testing.assert_array_equal(w, (val.astype(np.uint32) | (rem.astype(np.uint32) << 2))[order])


def test_5x4_counts_root_and_checksum():
    """deep levels with blocks wider than a backward tile: the one-block /
    open-columns path"""
    s, r = solved((5, 4, 4), "ranked")
    assert (r.positions, r.edges, r.primitives, r.root_line) == (3945711, 8757625, 845332, "TIE in 20 moves")
    b, _ = solved((5, 4, 4), "bucketed")
    assert s.checksum() == b.checksum()


def test_poisoned_table():
    """a solve writes every byte and bit it later reads"""
    from gamesmanmpi_amd.solver import Solver
    board = (4, 4, 4)
    t = c4_table(name_of(board))
    s = Solver(spec_of(board), layout="ranked")
    s.buffers[0].fill_(0xAA)
    r = s.solve()
    assert r.positions == len(t["keys"])
    k, w = sorted_dump([s.dump()])
    np.testing.assert_array_equal(k, t["keys"])
    np.testing.assert_array_equal(w, golden_words(t))
    s.buffers[0].fill_(0x55)
    s.solve()
    k, w = sorted_dump([s.dump()])
    np.testing.assert_array_equal(k, t["keys"])
    np.testing.assert_array_equal(w, golden_words(t))


def test_readers_on_the_ranked_table(tmp_path):
    from gamesmanmpi_amd import _lib, db
    board = (4, 4, 4)
    t = c4_table(name_of(board))
    info = c4_summary()[name_of(board)]
    words = golden_words(t)
    s, r = solved(board, "ranked")
    a = s.audit()
    assert (a["mismatches"], a["positions"], a["edges"]) == (0, info["positions"], info["edges"])
    c = s.census()
    np.testing.assert_array_equal(c["by_level"].sum(axis=0), info["value_hist_WLTD"])
    np.testing.assert_array_equal(c["by_level"].sum(axis=1)[:len(info["level_hist"])], info["level_hist"])
    np.testing.assert_array_equal(c["by_remoteness"].sum(axis=0), np.bincount(t["value"], minlength=4))
    at = np.arange(0, len(t["keys"]), 101)
    keys = t["keys"][at]
    ch, wd, nc, best = s.moves(keys)
    np.testing.assert_array_equal(nc, t["nchild"][at])
    pr, hn, hc = s.spec.host_expand(keys)
    for i in range(len(keys)):
        n = int(nc[i])
        assert ch[i, :n].tolist() == hc[i, :n].tolist()
        assert wd[i, :n].tolist() == words[np.searchsorted(t["keys"], ch[i, :n])].tolist()
        assert (best[i] == -1) == (n == 0)
    lk, lv, lr = s.best_line()
    assert int(lk[0]) == 0 and len(lk) == r.root_remoteness + 1 == 17
    assert lr.tolist() == list(range(16, -1, -1))
    np.testing.assert_array_equal(s.query(t["keys"]), words)
    bad = np.array([NON_POSITIONS_4x4[k] for k in sorted(NON_POSITIONS_4x4)], np.uint64)
    assert s.query(bad).tolist() == [_lib.GM_NO_WORD] * 4
    with pytest.raises(_lib.GmError):
        s.spec.tb_index_space()  # the indexed tablebase stays refused
    d = tmp_path / "stats" / "0"
    d.mkdir(parents=True)
    out = s.export_keyed_tablebase(str(d / db.TK_NAME))
    assert out["positions"] == len(t["keys"])
    (d / "meta.json").write_text(json.dumps({"game": s.spec.name, "params": s.spec.params, "format": "gmtk"}))
    sdb = db.SolutionDB(str(tmp_path))
    np.testing.assert_array_equal(sdb.tablebase.lookup_keys(t["keys"]), words)


def test_checkpoint_mid_forward_and_mid_backward(tmp_path):
    from gamesmanmpi_amd import checkpoint
    from gamesmanmpi_amd.solver import Solver
    board = (4, 3, 3)
    keys, words, gr = graph_words(board)
    T = spec_of(board).max_levels
    for cut in (T // 2, T + T // 2):
        s = Solver(spec_of(board), layout="ranked")
        assert 0 < cut < s.steps
        assert s.solve_steps(0, cut) is None
        ck = str(tmp_path / ("ck%d" % cut))
        checkpoint.save(s, ck, cut)
        del s
        s2, step = checkpoint.restore(ck)
        assert step == cut and s2.layout == "ranked"
        r = s2.solve_steps(step, 0)
        assert r.extra["layout"] == "ranked"
        assert (r.positions, r.edges, r.root_line) == (gr.positions, gr.edges, gr.root_line)
        k, w = sorted_dump([s2.dump()])
        np.testing.assert_array_equal(k, keys)
        np.testing.assert_array_equal(w, words)


def test_launcher(tmp_path):
    from gamesmanmpi_amd import solver_launcher as sl
    game = tmp_path / "connect_four.py"
    with open(GAME_FILE) as f:
        src = f.read()
    assert "length = 5" in src
    game.write_text(src.replace("length = 5", "length = 4", 1))
    out = io.StringIO()
    with redirect_stdout(out):
        rc = sl.main([str(game), "--layout", "ranked", "--line", "--census", "--audit"])
    text = out.getvalue()
    assert rc == 0 and text.splitlines()[0] == "TIE in 16 moves", text


def test_refusals():
    from gamesmanmpi_amd import _lib
    from gamesmanmpi_amd.solver import Solver
    with pytest.raises(_lib.GmError, match="board_symmetry=1 has no ranked layout"):
        Solver(spec_of((4, 3, 3), True), layout="ranked")
    with pytest.raises(_lib.GmError):
        Solver(spec_of((4, 3, 3)), layout="ranked", rank=0, world=2)
    from gamesmanmpi_amd.games import GameSpec
    with pytest.raises(ValueError, match="connect four"):
        Solver(GameSpec("tic_tac_toe_np"), layout="ranked")


def test_toot_ranked_still_matches_its_golden():
    """the shared host code (run_ranked, the views' dispatch) on toot 4x3"""
    from conftest import GOLDEN
    import os
    from gamesmanmpi_amd.games import GameSpec
    from gamesmanmpi_amd.solver import Solver
    z = np.load(os.path.join(GOLDEN, "tables", "toot_4x3.npz"))
    spec = GameSpec("toot_and_otto_bitstring", "length=4,height=3")
    s = Solver(spec, layout="ranked")
    r = s.solve()
    assert r.extra["layout"] == "ranked" and r.positions == len(z["value"])
    keys = spec.encode_batch(z["canon"], z["clen"])
    w = s.query(keys)
    np.testing.assert_array_equal(w, z["value"].astype(np.uint32) | (z["remoteness"].astype(np.uint32) << 2))
    c = s.census()
    np.testing.assert_array_equal(c["by_level"].sum(axis=0), np.bincount(z["value"], minlength=4))
