"""Every arm of the kind dispatch (csrc/gm_games.h: GenericKinds,
BucketedKinds, kind_dispatch_sym) solves once, at the smallest board that
reaches it: the five generic kinds, and the fixed boards toot 4x4 and connect
four 5x4, each plain and with board_symmetry=1 where the game has a board.

One descriptor is solved on BUCKETED (where it applies), on HASHED, and --
boards of at most 1e5 positions -- as two md5 shards of either keyed layout;
all of them must agree on gm_solver_checksum, and the position count must be
the enumerated one: SURVEY Appendix B, tests/golden/connect_four/summary.json,
the product of the heap bases for the sum, and for symmetric runs the
orbit count derived on the CPU (test_board_symmetry_cpu.ORBITS; numpy mirror
images of the golden keys for connect 3x3; of the plain solve's own keys for
the two fixed boards, which have no committed table).  Neither yardstick is
the code under test: BUCKETED and HASHED run different instantiations (fixed
against generic), and the counts come from the reference modules."""
import functools

import numpy as np
import pytest

from test_board_symmetry_cpu import ORBITS
from test_connect_four_cpu import c4_summary, c4_table, np_mirror

pytestmark = pytest.mark.gpu

# name: (game, params, positions, board (L, H) of a mirror-symmetric game or None)
KINDS = {
    "sum": ("sum_four_to_one", "heaps=3:2", 4 * 3, None),
    "ttt": ("tic_tac_toe_np", "", 5478, None),
    "toot_3x3": ("toot_and_otto_bitstring", "length=3,height=3", 11097, (3, 3)),
    "othello_4x4": ("othello_bit_new", "length=4,height=4", 54089, None),
    "connect_3x3": ("connect_four", "length=3,height=3,connect=3", 694, (3, 3)),
    "toot_4x4": ("toot_and_otto_bitstring", "length=4,height=4", 3468773, (4, 4)),
    "connect_5x4": ("connect_four", "length=5,height=4,connect=4", 3945711, (5, 4)),
}
FIXED = ("toot_4x4", "connect_5x4")
RUNS = [(n, s) for n in KINDS for s in (False, True) if not (s and n == "sum")]


def spec_of(name, sym):
    from gamesmanmpi_amd.games import GameSpec
    game, params = KINDS[name][:2]
    return GameSpec(game, (params + ",board_symmetry=1").lstrip(",") if sym else params)


@functools.lru_cache(maxsize=None)
def single(name, sym, layout):
    from gamesmanmpi_amd.solver import Solver
    s = Solver(spec_of(name, sym), layout=layout)
    r = s.solve()
    assert r.extra["layout"] == layout
    return s, r


def cell_mirror(keys, L, H):
    """x -> L - 1 - x of both planes' cells; the bits above them stay."""
    cells = np.uint64((1 << (2 * L * H)) - 1)
    return (keys & ~cells) | np_mirror(keys & cells, L, H)


def orbit_count(name):
    if name in ("ttt", "toot_3x3", "othello_4x4"):
        return ORBITS["tic_tac_toe_np" if name == "ttt" else name]
    L, H = KINDS[name][3]
    keys = c4_table("3x3_3")["keys"] if name == "connect_3x3" else single(name, False, "hashed")[0].dump()[0]
    return len(np.unique(np.minimum(keys, cell_mirror(keys, L, H))))


def test_recorded_counts():
    assert c4_summary()["3x3_3"]["positions"] == KINDS["connect_3x3"][2]
    assert c4_summary()["5x4_4"]["positions"] == KINDS["connect_5x4"][2]


@pytest.mark.parametrize("name,sym", RUNS)
def test_every_path_agrees(name, sym):
    from gamesmanmpi_amd.keyed import group_keyed_solve
    positions = orbit_count(name) if sym else KINDS[name][2]
    layouts = ["hashed"] if name == "sum" else ["bucketed", "hashed"]
    sums = {}
    for layout in layouts:
        s, r = single(name, sym, layout)
        c = s.checksum()
        assert r.positions == c["positions"] == positions, layout
        sums[layout] = c
    if name not in FIXED:
        for layout in layouts:
            r, shards = group_keyed_solve(spec_of(name, sym), 2, layout=layout)
            assert r.positions == positions, layout
            cs = [(sh.solver if layout == "hashed" else sh).checksum() for sh in shards]
            total = {k: sum(c[k] for c in cs) for k in ("positions", "win", "loss", "tie", "draw")}
            total["checksum"] = "%016x" % (sum(int(c["checksum"], 16) for c in cs) % (1 << 64))
            sums["2 shards, " + layout] = total
    first = sums[layouts[0]]
    for path, c in sums.items():
        assert c == first, (path, c, first)
