"""The three table readers (gm_solver_query / _positions / _checksum,
gm_table.h) on every layout and word form, against each other and against
the census, whose layout kernels share nothing with them: positions() lists
every position once, query() finds each of them and nothing else,
checksum() counts what query(positions()) holds, a short `cap` answers
GM_EFULL without writing, and two shards add up to the one table."""
import ctypes
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

NO_WORD = 0xFFFFFFFF
SUM = "sum_four_to_one"
TTT = "tic_tac_toe_np"

# id -> (game, params, layout, plane word bits or None).  The library reports a PLANES
# table's word bits but not which 8-bit form it holds; the form follows from the root
# digit sum alone (gm_plane.h; tests/test_abi_host.py test_planes_word_width_by_root_sum):
# absolute order words up to 253, relative ones from 254 to 505, 16-bit words beyond.
# solved() asserts the bits the library reports and the range the shape's root sum is in.
PLANE_FORM_BY_ROOT_SUM = {(8, "order"): range(0, 254), (8, "relative"): range(254, 506), (16, "order"): range(506, 1 << 16)}
CASES = {
    "ttt_hashed": (TTT, "", "hashed", None),
    "ttt_bucketed": (TTT, "", "bucketed", None),
    "ttt_bucketed_sym": (TTT, "board_symmetry=1", "bucketed", None),
    "planes_31_31_1_127": (SUM, "heaps=31:31:1:127", "planes", (8, "order")),
    "planes_31_31_444": (SUM, "heaps=31:31:444", "planes", (16, "order")),
    "planes_31_31_192": (SUM, "heaps=31:31:192", "planes", (8, "relative")),  # root sum 254: the first relative one
    "planes_31_31_3_63": (SUM, "heaps=31:31:3:63", "planes", (8, "order")),  # two outer heaps
    "dense_0": (SUM, "heaps=0", "dense", None),  # one position
    "dense_2_5_0_6": (SUM, "heaps=2:5:0:6", "dense", None),  # more than one block, no power of two
    "toot_3x4_ranked": ("toot_and_otto_bitstring", "length=3,height=4", "ranked", None),
}

_solved = {}


def solved(case):
    """(spec, solver, SolveResult, positions(), query(positions())): one solve
    per case for the whole module; no test changes it."""
    if case not in _solved:
        from gamesmanmpi_amd.games import GameSpec
        from gamesmanmpi_amd.solver import Solver
        game, params, layout, form = CASES[case]
        spec = GameSpec(game, params)
        s = Solver(spec, layout=layout)
        r = s.solve()
        assert r.extra["layout"] == layout
        if form:
            assert r.extra["word_bits"] == form[0]
            assert sum(int(h) for h in params.split("=")[1].split(":")) in PLANE_FORM_BY_ROOT_SUM[form]
        keys = s.positions()
        _solved[case] = (spec, s, r, keys, s.query(keys))
    return _solved[case]


def histogram(words):
    """{positions, win, loss, tie, draw} of an array of words."""
    n = np.bincount((words & 3).astype(np.int64), minlength=4)
    return {"positions": len(words), "win": int(n[0]), "loss": int(n[1]), "tie": int(n[2]), "draw": int(n[3])}


def non_positions(spec, keys):
    """A few keys that are no reachable position of the game."""
    if spec.name == SUM:
        total = int(np.prod([int(h) + 1 for h in spec.params.split("=")[1].split(":")], dtype=np.int64))
        out = [total, total + 1, total + 12345, (1 << 63) + 5]  # past the last rank
    elif spec.name == TTT:
        out = [0x15555, 0x2AAAA, 0x3FFFF, 1 << 40]  # nine marks of one player; bits past the board
    else:
        # toot 3x4: a T in the top row over an empty column; a position with a stray high bit
        out = [spec.root_key | (1 << (3 * 3 + 1)), int(keys[len(keys) // 2]) | (1 << 63)]
    out = np.array(out, np.uint64)
    assert not np.isin(out, keys).any()
    return out


@pytest.mark.parametrize("case", sorted(CASES))
def test_positions_are_the_solve_s_positions_once_each(case):
    _, _, r, keys, _ = solved(case)
    assert len(keys) == r.positions
    assert len(np.unique(keys)) == len(keys)


@pytest.mark.parametrize("case", sorted(CASES))
def test_query_finds_every_position_and_nothing_else(case):
    spec, s, _, keys, words = solved(case)
    assert not (words == NO_WORD).any()
    assert (s.query(non_positions(spec, keys)) == NO_WORD).all()


@pytest.mark.parametrize("case", sorted(CASES))
def test_checksum_counts_what_query_of_positions_holds(case):
    spec, s, _, _, words = solved(case)
    ck = s.checksum()
    want = histogram(words)
    assert {k: ck[k] for k in want} == want
    by_value = s.census()["by_remoteness"].sum(axis=0)
    assert [int(x) for x in by_value] == [want["win"], want["loss"], want["tie"], want["draw"]]
    with open(os.path.join(GOLDEN, "checksums.json")) as f:
        gold = [e for e in json.load(f).values() if (e["game"], e["params"]) == (spec.name, spec.params)]
    for e in gold:
        assert ck["checksum"] == e["checksum"]


@pytest.mark.parametrize("case", sorted(CASES))
def test_positions_short_cap_is_efull_and_writes_nothing(case):
    """cap = n - 1: GM_EFULL, *n = n, the buffer (cap slots and a guard
    element behind them) untouched; then cap = n fills exactly n slots."""
    import torch
    from gamesmanmpi_amd import _lib
    _, s, r, keys, _ = solved(case)
    L = _lib.load()
    n = r.positions
    fill = -0x0123456789ABCDEF
    buf = torch.full((n + 1,), fill, dtype=torch.int64, device=s.device)
    got = ctypes.c_uint64()
    with torch.cuda.device(s.device):
        rc = L.gm_solver_positions(s._h, buf.data_ptr(), n - 1, ctypes.byref(got))
        torch.cuda.synchronize()
        assert rc == _lib.GM_EFULL and got.value == n
        assert bool((buf == fill).all())
        rc = L.gm_solver_positions(s._h, buf.data_ptr(), n, ctypes.byref(got))
        torch.cuda.synchronize()
    assert rc == 0 and got.value == n
    out = buf.cpu().numpy()
    assert out[n] == fill
    np.testing.assert_array_equal(np.sort(out[:n].view(np.uint64)), np.sort(keys))


# two shards of one table: DENSE slices; the PLANES row deal (heap 1 of 64 values: two
# shards of 32 rows, which one table holds only on the DENSE layout).
# id -> (params, the one table's layout, the shards' layout)
SHARD_CASES = {"dense": ("heaps=7:7:7:15", "dense", "dense"), "planes_rows": ("heaps=31:63:7", "dense", "planes")}


@pytest.mark.parametrize("case", sorted(SHARD_CASES))
def test_two_shards_add_up_to_the_one_table(case):
    from gamesmanmpi_amd.dist import group_solve
    from gamesmanmpi_amd.games import GameSpec
    from gamesmanmpi_amd.solver import Solver
    params, one_layout, layout = SHARD_CASES[case]
    spec = GameSpec(SUM, params)
    one = Solver(spec, layout=one_layout)
    r1 = one.solve()
    rg, shards = group_solve(spec, 2, layout=layout)
    assert (r1.extra["layout"], rg.extra["layout"]) == (one_layout, layout) and rg.positions == r1.positions
    ck1, cks = one.checksum(), [sh.checksum() for sh in shards]
    assert "%016x" % (sum(int(c["checksum"], 16) for c in cks) % (1 << 64)) == ck1["checksum"]
    for k in ("positions", "win", "loss", "tie", "draw"):
        assert sum(c[k] for c in cks) == ck1[k]
    parts = [sh.positions() for sh in shards]
    assert [len(p) for p in parts] == [c["positions"] for c in cks] and all(len(p) for p in parts)
    union = np.concatenate(parts)
    assert len(union) == r1.positions
    np.testing.assert_array_equal(np.sort(union), np.sort(one.positions()))
