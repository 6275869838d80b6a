"""GPU: gm_graph_solve_loopy (gm_graph_loopy.h), the retrograde of game files
whose positions repeat, against tests/loopy_reference.py (rules A to D of
DESIGN.md §7k as heap worklists; pinned by tests/test_loopy_reference_cpu.py).
Every word and the four counts are compared exactly."""
import ctypes
import io
import json
import os
from contextlib import redirect_stdout

import numpy as np
import pytest

from conftest import ROOT
from graph_reference import DRAW, LOSS, TIE, UNDECIDED, WIN
from loopy_reference import HAND_GRAPHS, csr, solve_loopy

pytestmark = pytest.mark.gpu
GAMES = os.path.join(ROOT, "tests", "games")
ALL = (WIN, LOSS, TIE, DRAW)


def _load(path):
    from gamesmanmpi_amd.solver_launcher import ensure_src_utils, load_game
    ensure_src_utils()
    return load_game(path)


def raw_solve(prim, offsets, children, root=0, fill=None):
    """gm_graph_solve_loopy through the raw ABI: (rc, gm_result, words u32,
    counts tuple).  fill: the words buffer's content before the call."""
    import torch
    from gamesmanmpi_amd import _lib
    from gamesmanmpi_amd.generic import loopy_scratch_bytes
    dev = torch.device("cuda")
    n = len(prim)
    p = torch.from_numpy(np.ascontiguousarray(prim, np.uint8)).to(dev)
    off = torch.from_numpy(np.ascontiguousarray(offsets, np.int64)).to(dev)
    ch = np.ascontiguousarray(children, np.uint32)
    ch = torch.from_numpy((ch if len(ch) else np.zeros(1, np.uint32)).view(np.int32)).to(dev)
    words = torch.full((n,), 0x55 if fill is None else fill, dtype=torch.int32, device=dev)
    scratch = torch.zeros(loopy_scratch_bytes(n), dtype=torch.uint8, device=dev)
    r = _lib.gm_result()
    counts = (ctypes.c_uint64 * 4)(7, 7, 7, 7)
    rc = _lib.load().gm_graph_solve_loopy(p.data_ptr(), off.data_ptr(), ch.data_ptr(), n, root, words.data_ptr(),
                                          scratch.data_ptr(), torch.cuda.current_stream(dev).cuda_stream,
                                          ctypes.byref(r), counts)
    torch.cuda.synchronize(dev)
    return rc, r, words.cpu().numpy().view(np.uint32), tuple(int(c) for c in counts)


def check(prim, offsets, children):
    """Solve on the GPU and compare words, counts, counters and root with the
    yardstick; returns (gm_result, words, counts)."""
    want, want_counts = solve_loopy(prim, offsets, children)
    rc, r, words, counts = raw_solve(prim, offsets, children)
    assert rc == 0
    np.testing.assert_array_equal(words, np.array(want, np.uint32))
    assert counts == want_counts and sum(counts) == len(prim)
    assert (r.positions, r.edges, r.primitives) == (len(prim), len(children), int((np.asarray(prim) != UNDECIDED).sum()))
    assert (r.root_word, r.root_value, r.root_remoteness) == (want[0], want[0] & 3, want[0] >> 2)
    assert 1 <= r.levels == r.n_resolve_launches <= 2 * len(prim) + 8
    return r, words, counts


# ---- 1. the hand graphs -------------------------------------------------------
@pytest.mark.parametrize("k", range(len(HAND_GRAPHS)))
def test_hand_graphs(k):
    prim, kids, words, counts = HAND_GRAPHS[k]
    rc, r, got, got_counts = raw_solve(*csr(prim, kids))
    assert rc == 0 and got.tolist() == words and got_counts == counts
    assert (r.root_value, r.root_remoteness) == (words[0] & 3, words[0] >> 2)
    check(*csr(prim, kids))


def test_two_cycle_and_self_loop_are_draws():
    from gamesmanmpi_amd.generic import enumerate_game
    g = enumerate_game(_load(os.path.join(GAMES, "two_cycle.py")))
    rc, r, words, counts = raw_solve(g.prim, g.offsets, g.children)
    assert rc == 0 and words.tolist() == [3, 3, 3] and counts == (0, 0, 0, 3)
    assert (r.root_value, r.root_remoteness, r.edges) == (DRAW, 0, 3)
    rc, r, words, counts = raw_solve(*csr([UNDECIDED], {0: [0]}))
    assert rc == 0 and words.tolist() == [3] and counts == (0, 0, 0, 1)


def test_counts_may_be_null():
    import torch
    from gamesmanmpi_amd import _lib
    from gamesmanmpi_amd.generic import loopy_scratch_bytes
    dev = torch.device("cuda")
    prim, off, ch = csr(*HAND_GRAPHS[4][:2])
    t = [torch.from_numpy(a).to(dev) for a in (prim, off, ch.view(np.int32))]
    words = torch.zeros(len(prim), dtype=torch.int32, device=dev)
    scratch = torch.zeros(loopy_scratch_bytes(len(prim)), dtype=torch.uint8, device=dev)
    r = _lib.gm_result()
    assert _lib.load().gm_graph_solve_loopy(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), len(prim), 0,
                                            words.data_ptr(), scratch.data_ptr(),
                                            torch.cuda.current_stream(dev).cuda_stream, ctypes.byref(r), None) == 0
    assert words.cpu().tolist() == HAND_GRAPHS[4][2]


def test_founded_words_far_away_are_reached_in_a_few_rounds():
    """a <-> b beside a founded chain 40 deep: a's only LOSS child has
    remoteness 40, so rounds 1 .. 40 of phase B could resolve nothing; the
    host goes from round 1 to round 41 (the least remoteness the round
    ignored, + 1).  Phase A needs at most 42 rounds, B three."""
    depth = 40
    kids = {i: [i + 1] for i in range(depth)}      # 0 .. 40: the chain, 40 a LOSS primitive
    a, b = depth + 1, depth + 2
    kids[a], kids[b] = [b, 0], [a]
    prim = [UNDECIDED] * depth + [LOSS, UNDECIDED, UNDECIDED]
    r, words, counts = check(*csr(prim, kids))
    assert words[0] == (LOSS | depth << 2)
    assert words[a] == (WIN | (depth + 1) << 2) and words[b] == (LOSS | (depth + 2) << 2)
    assert counts == (depth + 1, 2, 0, 0)
    assert r.levels <= depth + 2 + 3


# ---- 2. a graph without cycles: the old entry's words --------------------------
def test_dag_grid_tictactoe_is_bit_identical():
    from gamesmanmpi_amd.generic import GenericSolver, enumerate_game
    g = enumerate_game(_load(os.path.join(GAMES, "grid_tictactoe.py")))
    old, new = GenericSolver(g), GenericSolver(g, loopy=True)
    r0, r1 = old.solve(), new.solve()
    np.testing.assert_array_equal(new.words, old.words)
    assert "loopy" not in r0.extra
    assert {k: r1.extra[k] for k in ("loopy", "founded", "attractor", "tie", "draw")} == {
        "loopy": True, "founded": g.n, "attractor": 0, "tie": 0, "draw": 0}
    assert (r1.positions, r1.edges, r1.primitives, r1.root_line) == (r0.positions, r0.edges, r0.primitives, r0.root_line)
    # phase A is the old loop and nothing follows it: at most height + 1 rounds (a round may pick up more)
    assert 1 <= r1.levels == r1.n_resolve_launches <= 10


def test_dag_fuzz_20000_is_bit_identical():
    from gamesmanmpi_amd.generic import GenericSolver
    from test_gpu_graph_fuzz import random_dag
    rng = np.random.default_rng(29)
    g = random_dag(rng, 20000, window=200).graph(rng)
    old = GenericSolver(g)
    r0 = old.solve()
    rc, r, words, counts = raw_solve(g.prim, g.offsets, g.children)
    assert rc == 0 and counts == (g.n, 0, 0, 0)
    np.testing.assert_array_equal(words, old.words)
    assert (r.positions, r.edges, r.primitives) == (r0.positions, r0.edges, r0.primitives)
    assert set((words & 3).tolist()) == set(ALL)


# ---- 3. fuzz -------------------------------------------------------------------
def random_loopy(rng, n, codes=ALL, p=0.05):
    """n positions; each code of `codes` with probability p, else 1 .. 4
    children drawn uniformly over ALL positions: back edges, self loops and
    duplicate children wherever they fall, and a few of each put in by hand."""
    u = rng.random(n)
    prim = np.full(n, UNDECIDED, np.uint8)
    for j, c in enumerate(codes):
        prim[(u >= j * p) & (u < (j + 1) * p)] = c
    deg = np.where(prim == UNDECIDED, rng.integers(1, 5, n), 0)
    offsets = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    children = rng.integers(0, n, int(offsets[-1])).astype(np.uint32)
    inner = np.flatnonzero(deg >= 2)
    for i in inner[:: max(1, len(inner) // 16)]:
        a = offsets[i]
        if i % 2:
            children[a] = i                      # a self loop
        else:
            children[a + 1] = children[a]        # the same child twice
    return prim, offsets, children


def _dups_and_loops(prim, offsets, children):
    dups = loops = 0
    for i in np.flatnonzero(prim == UNDECIDED):
        c = children[offsets[i]:offsets[i + 1]].tolist()
        dups += len(c) - len(set(c))
        loops += i in c
    return dups, loops


@pytest.mark.parametrize("seed", range(10))
def test_fuzz_against_the_yardstick(seed):
    rng = np.random.default_rng(1000 + seed)
    g = random_loopy(rng, 3000)
    dups, loops = _dups_and_loops(*g)
    assert dups >= 4 and loops >= 4
    _, words, counts = check(*g)
    # cycles are everywhere; phases B and C together resolve more than half of what A
    # left open, so the open list is compacted again on the way (at 1,024 entries or more)
    assert counts[0] < 1000 and counts[3] < (3000 - counts[0]) // 2
    assert set((words & 3).tolist()) == set(ALL)


@pytest.mark.parametrize("n", [255, 256, 257])
def test_fuzz_sizes_around_one_block(n):
    rng = np.random.default_rng(n)
    _, _, counts = check(*random_loopy(rng, n))
    assert counts[0] < n


@pytest.mark.parametrize("seed", range(3))
def test_fuzz_long_attractor_chains(seed):
    """LOSS primitives only, at 0.02: nearly everything is unfounded, the
    attractor's WIN / LOSS words come in chains from the few primitives, and
    the rest -- most of the graph -- is DRAW."""
    rng = np.random.default_rng(2000 + seed)
    g = random_loopy(rng, 3000, codes=(LOSS,), p=0.02)
    _, words, counts = check(*g)
    assert counts[2] == 0 and counts[1] > 200 and counts[3] > 1500
    assert int((words >> 2).max()) >= 6


# ---- 4. a long ring ------------------------------------------------------------
def test_ring_of_3000_with_one_exit():
    """0 -> 1 -> .. -> 2999 -> 0, and 2999 -> 3000, a LOSS primitive: 2999 is
    WIN in 1, 2998 LOSS in 2, .. position 0 in 3000, one position per round.
    Relabelled at random, so the scan order says nothing.  The rounds: 2 of
    phase A, 3000 of phase B -- inside the cap of 2 n + 8."""
    m = 3000
    rng = np.random.default_rng(41)
    perm = np.concatenate([[0], 1 + rng.permutation(m)])
    kids = {int(perm[i]): [int(perm[i + 1])] for i in range(m - 1)}
    kids[int(perm[m - 1])] = [int(perm[0]), int(perm[m])]
    prim = np.full(m + 1, UNDECIDED, np.uint8)
    prim[perm[m]] = LOSS
    r, words, counts = check(*csr(prim, kids))
    assert counts == (1, m, 0, 0)
    assert words[0] == ((LOSS if m % 2 == 0 else WIN) | m << 2)
    assert sorted((words >> 2).tolist()) == list(range(m + 1))
    assert m <= r.levels <= m + 4


# ---- 5. the loopy game file ----------------------------------------------------
def test_cat_and_mouse_through_solve_module():
    from gamesmanmpi_amd import _lib
    from gamesmanmpi_amd.generic import solve_module
    mod = _load(os.path.join(GAMES, "cat_and_mouse.py"))
    with pytest.raises(_lib.GmError, match="never resolve"):  # the default is unchanged
        solve_module(mod)
    result, solver = solve_module(mod, loopy=True)
    g = solver.graph
    want, counts = solve_loopy(g.prim, g.offsets, g.children)
    np.testing.assert_array_equal(solver.words, np.array(want, np.uint32))
    assert tuple(result.extra[k] for k in ("founded", "attractor", "tie", "draw")) == counts
    assert result.extra["loopy"] is True and result.positions == g.n and result.edges == g.edges
    names, val, rem = solver.dump()
    assert set(val.tolist()) == set(ALL) and (rem[val == DRAW] == 0).all()
    assert (result.root_value, result.root_remoteness) == (want[0] & 3, want[0] >> 2)


def test_cat_and_mouse_through_the_launcher(tmp_path):
    from gamesmanmpi_amd import solver_launcher as sl
    from gamesmanmpi_amd.generic import enumerate_game
    from gamesmanmpi_amd.solver import NAMES
    game = os.path.join(GAMES, "cat_and_mouse.py")
    g = enumerate_game(_load(game))
    want, counts = solve_loopy(g.prim, g.offsets, g.children)
    want = np.array(want, np.uint32)
    out = io.StringIO()
    with redirect_stdout(out):
        rc = sl.main([game, "--loopy", "--census", "--json", "-sd", str(tmp_path / "sd")])
    assert rc == 0
    lines = out.getvalue().splitlines()
    assert lines[0] == "%s in %d moves" % (NAMES[want[0] & 3], want[0] >> 2)  # the root line as ever
    row = json.loads(next(ln for ln in lines if ln.startswith("{")))
    assert row["loopy"] is True and row["layout"] == "graph" and row["positions"] == g.n
    assert (row["founded"], row["attractor"], row["tie"], row["draw"]) == counts
    assert row["founded"] + row["attractor"] + row["tie"] + row["draw"] == row["positions"]
    # the Draw column: every DRAW in row 0 of the remoteness table, in the JSON and in the text
    by_rem = np.array(row["census"]["by_remoteness"])
    assert by_rem[:, 3].sum() == by_rem[0, 3] == counts[3] > 0
    assert by_rem.sum(axis=0).tolist() == [int(((want & 3) == v).sum()) for v in ALL]
    head = next(i for i, ln in enumerate(lines) if ln.split()[:1] == ["Remoteness"])
    assert lines[head].split() == ["Remoteness", "Win", "Lose", "Tie", "Draw", "Total"]
    assert int(lines[head + 1].split()[4]) == counts[3] and lines[head + 1].split()[0] == "0"
    total = next(ln for ln in lines[head:] if ln.split()[:1] == ["Total"])
    assert int(total.split()[4]) == counts[3] and int(total.split()[5]) == g.n
    assert any(ln.startswith("longest DRAW: ") and ln.endswith(" in 0 moves") for ln in lines)
    d = tmp_path / "sd" / "stats" / "0"
    with open(d / "meta.json") as f:
        meta = json.load(f)
    assert meta["loopy"] is True and meta["value_codes"]["DRAW"] == 3 and meta["positions"] == g.n
    assert (meta["founded"], meta["attractor"], meta["tie"], meta["draw"]) == counts
    z = np.load(d / "solution.npz")
    assert z["names"].tolist() == g.names
    np.testing.assert_array_equal(z["value"], (want & 3).astype(np.uint8))
    np.testing.assert_array_equal(z["remoteness"], want >> 2)


def test_launcher_loopy_on_a_descriptor_game_through_the_graph_layout(tmp_path):
    """--layout graph --loopy on a game without cycles: the words of any graph
    solve, and no "loopy" key without the flag."""
    from gamesmanmpi_amd import solver_launcher as sl
    game = os.path.join(GAMES, "descriptor_ttt", "tic_tac_toe_np.py")
    rows = []
    for flags in (["--loopy"], []):
        out = io.StringIO()
        with redirect_stdout(out):
            assert sl.main([game, "--layout", "graph", "--json", "--no-verify"] + flags) == 0
        lines = out.getvalue().splitlines()
        assert lines[0] == "TIE in 9 moves"
        rows.append(json.loads(lines[1]))
    assert rows[0]["loopy"] is True and (rows[0]["founded"], rows[0]["draw"]) == (5478, 0)
    assert "loopy" not in rows[1] and "founded" not in rows[1]


# ---- 6. kept behaviour ---------------------------------------------------------
@pytest.mark.parametrize("root", [3, 4, 1 << 40])
def test_root_outside_the_graph_is_refused(root):
    from gamesmanmpi_amd import _lib
    g = csr([UNDECIDED, UNDECIDED, LOSS], {0: [1], 1: [0, 2]})
    rc, _, words, counts = raw_solve(*g, root=root)
    assert rc == _lib.GM_EINVAL
    assert (words == 0x55).all() and counts == (7, 7, 7, 7)  # nothing ran
    rc, r, words, _ = raw_solve(*g, root=2)
    assert rc == 0 and (r.root_value, r.root_remoteness) == (LOSS, 0)
    rc, r, words, _ = raw_solve(*g, root=1)
    assert rc == 0 and (r.root_value, r.root_remoteness) == (WIN, 1) and words.tolist() == [9, 4, 1]


def test_undecided_leaf_is_the_old_error():
    from gamesmanmpi_amd import _lib
    from gamesmanmpi_amd.generic import GameGraph, GenericSolver
    rng = np.random.default_rng(23)
    prim, offsets, children = random_loopy(rng, 5000)
    leaf = int(np.flatnonzero(prim != UNDECIDED)[-7])
    prim[leaf] = UNDECIDED
    g = GameGraph([str(i) for i in range(len(prim))], prim, offsets, children)
    with pytest.raises(_lib.GmError, match="non-primitive-without-moves") as err:
        GenericSolver(g, loopy=True).solve()
    assert err.value.code == _lib.GM_ECORRUPT
    with pytest.raises(_lib.GmError, match="non-primitive-without-moves"):
        GenericSolver(g).solve()
