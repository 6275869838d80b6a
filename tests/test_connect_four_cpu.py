"""Connect Four (gamesmanmpi_amd/games/connect_four.py, K_CONNECT in
csrc/gm_games.h) on the host: the module's position counts, the descriptor
against the module on every position of small boards (where a line mask that
wrapped a row would show), the compile-time boards against the generic form,
the md5 owners, the mirror, and the refusals.  The yardstick is the module
and the fixtures tests/golden/make_connect_four.py generated from it."""
import functools
import hashlib
import json
import os
import random

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

C4_GOLDEN = os.path.join(GOLDEN, "connect_four")
GAME_FILE = os.path.join(ROOT, "gamesmanmpi_amd", "games", "connect_four.py")


def c4_params(L, H, K):
    return "length=%d,height=%d,connect=%d" % (L, H, K)


def c4_module(L, H, K):
    """The game file loaded as the launcher loads it, with the three
    constants set (they are read at call time)."""
    from gamesmanmpi_amd.solver_launcher import ensure_src_utils, load_game
    ensure_src_utils()
    mod = load_game(GAME_FILE)
    mod.length, mod.height, mod.connect = L, H, K
    return mod


def c4_summary():
    with open(os.path.join(C4_GOLDEN, "summary.json")) as f:
        return json.load(f)


def c4_table(name):
    z = np.load(os.path.join(C4_GOLDEN, name + ".npz"))
    return {k: z[k] for k in z.files}


def py_key(pos):
    """The key of the issue's layout, restated: X plane in bits [0, A), O
    plane in bits [A, 2A), cell bit = string index."""
    A, k = len(pos), 0
    for i, c in enumerate(pos):
        if c == "X":
            k |= 1 << i
        elif c == "O":
            k |= 1 << (A + i)
    return k


def np_mirror(keys, L, H):
    """x -> L - 1 - x of both planes, per cell."""
    keys = np.asarray(keys, np.uint64)
    out = np.zeros_like(keys)
    A = L * H
    for plane in range(2):
        for y in range(H):
            for x in range(L):
                src, dst = plane * A + L * y + x, plane * A + L * y + (L - 1 - x)
                out |= ((keys >> np.uint64(src)) & np.uint64(1)) << np.uint64(dst)
    return out


@functools.lru_cache(maxsize=None)
def c4_graph(L, H, K):
    from gamesmanmpi_amd.generic import enumerate_game
    return enumerate_game(c4_module(L, H, K))


@pytest.mark.parametrize("board,count", [((4, 4, 4), 161029), ((4, 3, 3), 7157)])
def test_module_enumeration(board, count):
    g = c4_graph(*board)
    info = c4_summary()["%dx%d_%d" % board]
    assert g.n == count == info["positions"]
    assert g.edges == info["edges"]
    assert int((g.prim != 4).sum()) == info["primitives"]


def test_fixtures_reproduce_the_enumerated_table():
    """positions / widest level / primitives of the boards enumerated when the
    rules were fixed; 161,029 and 3,945,711 are the published counts too."""
    want = {"2x2_2": (13, 6, 6), "3x2_3": (115, 33, 21), "1x4_4": (5, 1, 1), "4x1_4": (35, 12, 6),
            "3x3_3": (694, 176, 189), "4x3_3": (7157, 1598, 2526), "4x4_3": (41750, 8268, 17820),
            "4x4_4": (161029, 28922, 26740), "5x4_4": (3945711, 620337, 845332)}
    s = c4_summary()
    for name, row in want.items():
        assert (s[name]["positions"], s[name]["max_level_width"], s[name]["primitives"]) == row, name


@pytest.mark.parametrize("board", [(4, 3, 3), (4, 4, 4), (5, 4, 4), (6, 5, 4), (1, 4, 4), (4, 1, 4), (3, 2, 3)])
def test_verify(board):
    from gamesmanmpi_amd.games import GameSpec, spec_for_module
    mod = c4_module(*board)
    spec = spec_for_module(mod, "connect_four")
    assert (spec.name, spec.params) == ("connect_four", c4_params(*board))
    assert spec.max_levels == board[0] * board[1] + 1 and spec.key_bits == 2 * board[0] * board[1]
    assert spec.verify(mod, samples=300) == 300
    sym = GameSpec("connect_four", c4_params(*board) + ",board_symmetry=1")
    assert sym.verify(mod, samples=300) == 300


@pytest.mark.parametrize("board", [(4, 3, 3), (4, 4, 3)])
def test_host_descriptor_against_the_module_everywhere(board):
    from gamesmanmpi_amd.games import GameSpec
    L, H, K = board
    g = c4_graph(*board)
    spec = GameSpec("connect_four", c4_params(*board))
    keys = np.array([py_key(n) for n in g.names], np.uint64)
    assert spec.root_key == 0 == int(keys[0])
    # encode / decode / str(pos)
    canon = np.array([list(n.encode("ascii")) for n in g.names], np.uint8)
    np.testing.assert_array_equal(spec.encode_batch(canon, np.full(g.n, L * H, np.uint8)), keys)
    back, lens = spec.decode_batch(keys, stride=32)
    assert (lens == L * H).all()
    np.testing.assert_array_equal(back[:, :L * H], canon)
    for i in range(0, g.n, 97):
        assert spec.str_utf8(int(keys[i])) == g.names[i].encode("utf-8")
        assert spec.key_of(g.names[i]) == int(keys[i]) and spec.pos_of(int(keys[i])) == g.names[i]
    # primitive, children in gen_moves order, level
    pr, nc, ch = spec.host_expand(keys)
    np.testing.assert_array_equal(pr, g.prim)
    np.testing.assert_array_equal(nc, np.diff(g.offsets))
    flat = ch[np.arange(ch.shape[1])[None, :] < nc[:, None]]
    np.testing.assert_array_equal(flat, keys[g.children])
    pieces = np.array([L * H - n.count("-") for n in g.names], np.int32)
    np.testing.assert_array_equal(spec.host_level(keys), pieces)


def test_fixed_boards_against_the_generic_descriptor():
    """ConnectFixed<5,4,4> / <6,5,4> (gm_fixed_expand) and the generic
    descriptor on playouts: the same primitive codes and children."""
    from gamesmanmpi_amd import _lib
    from gamesmanmpi_amd.games import GameSpec
    for L, H in ((5, 4), (6, 5)):
        for extra in ("", ",board_symmetry=1"):
            spec = GameSpec("connect_four", c4_params(L, H, 4) + extra)
            rng = random.Random(L)
            seen = {spec.root_key}
            for _ in range(200):
                k = spec.root_key
                while True:
                    pr, nc, ch = spec.host_expand(np.array([k], np.uint64))
                    if pr[0] != 4:
                        break
                    k = int(ch[0, rng.randrange(nc[0])])
                    seen.add(k)
            keys = np.array(sorted(seen), np.uint64)
            pr, nc, ch = spec.host_expand(keys)
            fch = np.zeros_like(ch)
            fnc, fpr = np.zeros_like(nc), np.zeros_like(pr)
            _lib.check(_lib.load().gm_host_expand_fixed(spec.id, keys.ctypes.data, len(keys), fch.ctypes.data,
                                                        fnc.ctypes.data, fpr.ctypes.data))
            np.testing.assert_array_equal(fpr, pr)
            np.testing.assert_array_equal(fnc, nc)
            np.testing.assert_array_equal(fch, ch)
            assert (pr != 4).any() and (nc > 0).any()


def test_md5_owners():
    from gamesmanmpi_amd.games import GameSpec
    g = c4_graph(4, 3, 3)
    spec = GameSpec("connect_four", c4_params(4, 3, 3))
    at = list(range(0, g.n, 13))
    keys = np.array([py_key(g.names[i]) for i in at], np.uint64)
    for P in range(1, 9):
        want = [int(hashlib.md5(g.names[i].encode("utf-8")).hexdigest(), 16) % P for i in at]
        assert spec.owners_host(keys, P).tolist() == want
    # a 30-cell board: the longest str(pos)
    big = GameSpec("connect_four", c4_params(6, 5, 4))
    pos = ("XOXOXO" * 2 + "OXOXOX" * 2 + "XO----")
    assert len(pos) == 30
    for P in (2, 3, 7, 8):
        assert int(big.owners_host([py_key(pos)], P)[0]) == int(hashlib.md5(pos.encode()).hexdigest(), 16) % P


@pytest.mark.parametrize("board", [(4, 3, 3), (5, 4, 4), (3, 2, 3), (1, 4, 4)])
def test_symmetry(board):
    from gamesmanmpi_amd.games import GameSpec
    L, H, K = board
    plain = GameSpec("connect_four", c4_params(*board))
    sym = GameSpec("connect_four", c4_params(*board) + ",board_symmetry=1")
    assert sym.symmetry_count() == 1 and plain.symmetry_count() == 0
    rng = random.Random(7)
    seen = {0}
    for _ in range(100):
        k = 0
        while True:
            pr, nc, ch = plain.host_expand(np.array([k], np.uint64))
            if pr[0] != 4:
                break
            k = int(ch[0, rng.randrange(nc[0])])
            seen.add(k)
    keys = np.array(sorted(seen), np.uint64)
    img = sym.symmetry(keys, 0)
    np.testing.assert_array_equal(img, np_mirror(keys, L, H))
    np.testing.assert_array_equal(sym.symmetry(img, 0), keys)          # an involution
    assert int(sym.symmetry(np.array([sym.root_key], np.uint64), 0)[0]) == sym.root_key == 0
    np.testing.assert_array_equal(sym.symmetry(keys), np.minimum(keys, img))
    # the mirror commutes with the moves, up to their order
    pr, nc, ch = plain.host_expand(keys)
    pi, ni, ci = plain.host_expand(img)
    np.testing.assert_array_equal(pr, pi)
    np.testing.assert_array_equal(nc, ni)
    for i in range(len(keys)):
        assert sorted(np_mirror(ch[i, :nc[i]], L, H).tolist()) == sorted(ci[i, :ni[i]].tolist())
    # the symmetric descriptor emits the representatives of the same children
    reps = np.unique(np.minimum(keys, img))
    ps, ns, cs = sym.host_expand(reps)
    pp, npl, cp = plain.host_expand(reps)
    for i in range(len(reps)):
        c = cp[i, :npl[i]]
        assert np.minimum(c, np_mirror(c, L, H)).tolist() == cs[i, :ns[i]].tolist()


@pytest.mark.parametrize("params", [
    "length=7,height=6,connect=4",      # 42 cells
    "length=6,height=6,connect=4",      # 36 cells
    "length=9,height=3,connect=4",      # more than 8 columns
    "length=4,height=4,connect=5",      # no such line
    "length=4,height=4,connect=0",
    "length=0,height=4,connect=1",
    "length=4,height=4,connect=4,symmetry=1",   # the module defines no symmetry_functions()
])
def test_refusals(params):
    from gamesmanmpi_amd import _lib
    from gamesmanmpi_amd.games import GameSpec
    with pytest.raises(_lib.GmError) as e:
        GameSpec("connect_four", params)
    assert e.value.code == _lib.GM_EINVAL


def test_no_indexed_tablebase_and_position_bounds():
    from gamesmanmpi_amd import _lib
    from gamesmanmpi_amd.games import GameSpec
    with pytest.raises(_lib.GmError) as e:
        GameSpec("connect_four", c4_params(4, 4, 4)).tb_index_space()
    assert e.value.code == _lib.GM_EINVAL
    assert GameSpec("connect_four", c4_params(4, 4, 4)).positions_bound == 161029
    assert GameSpec("connect_four", "").positions_bound == 3945711  # the default board: 5x4, connect 4
    # other boards: the gravity fillings with balanced colours, wins ignored
    s = c4_summary()
    for name in ("2x2_2", "3x2_3", "1x4_4", "4x1_4", "3x3_3", "4x3_3", "4x4_3"):
        L, H, K = s[name]["length"], s[name]["height"], s[name]["connect"]
        ways = [1] + [0] * (L * H)
        for _ in range(L):
            ways = [sum(ways[n - h] for h in range(H + 1) if n - h >= 0) for n in range(L * H + 1)]
        from math import comb
        bound = sum(w * comb(n, n // 2) for n, w in enumerate(ways))
        assert GameSpec("connect_four", c4_params(L, H, K)).positions_bound == bound >= s[name]["positions"]
    # (1x4: 1 + 1 + 2 + 3 + 6 colourings of the one stack, alternation ignored)
    assert GameSpec("connect_four", c4_params(1, 4, 4)).positions_bound == 13
