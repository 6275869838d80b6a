"""GPU: sum_four_to_one at the root digit sums where a table changes its
word form, every position against the CPU oracle's row solver
(oracle/oracle_mt.c, pinned to the DFS oracle at these sums by
tests/test_oracle_edges_cpu.py).

PLANES (plane_form, gm_plane_run.h): absolute 8-bit order forms up to sum
253 -- the one-launch backward k_plane_flow runs only on these --, relative
8-bit forms from 254 to kPlaneRelMaxSum = 505 (their parent rule and frame
shift depend on the digit sum mod 4: 254 .. 257 put the root in each class),
16-bit words above.  DENSE (dense_plan_bits, gm_solver.hip): 8-bit words up
to 253 when base[1] >= 16, else 16-bit.

One outer heap of 192 values is a 192-level chain of one plane per level:
the longest ready-flag chain k_plane_flow can meet, three of the four planes
of every visit pads and seven of the eight XCD chunks of every level empty.

Every oracle solve here takes under a second on the CPU (the slowest,
31:31:3:192 with 790,528 positions: 0.05 s for the solve, 0.6 s to read the
words out), so every table is compared word for word, the ones above 500,000
positions too; each shape's oracle words are read once and shared."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LEVELS, X1, W16, NO_RUNS, W32, SCALAR = 65536, 1024, 64, 8192, 4, 8  # gamesmanmpi_amd/_lib.py GM_F_*


def _solve(heaps, layout="planes", flags=0):
    from gamesmanmpi_amd.games import GameSpec
    from gamesmanmpi_amd.solver import Solver
    s = Solver(GameSpec("sum_four_to_one", "heaps=" + heaps), layout=layout, flags=flags)
    return s, s.solve()


@functools.lru_cache(maxsize=None)
def _oracle(heaps):
    """(row solution with checksum, words u32 by rank -- read-only)"""
    from oracle.oracle import Game
    sol = Game("sum_four_to_one", "heaps=" + heaps).solve_rows()
    sol.refresh(True)
    w = np.array([sol.word(k) for k in range(sol.count)], np.uint32)
    w.setflags(write=False)
    assert sum(int(h) for h in heaps.split(":")) in (253, 254, 255, 256, 257, 506)
    return sol, w


def _check(s, r, heaps, bits, kernel, layout="planes"):
    """Counts, root line, form and kernel, every word, the fingerprint and
    20,000 sampled words (the query path on scattered keys) against the
    oracle; returns the table's words by rank."""
    sol, want = _oracle(heaps)
    assert (r.extra["layout"], r.extra["word_bits"], r.extra["resolve_kernel"]) == (layout, bits, kernel)
    assert (r.positions, r.edges, r.primitives, r.root_line) == (sol.count, sol.edges, sol.stats["primitives"],
                                                                  sol.root_line)
    got = s.query(np.arange(sol.count, dtype=np.uint64))
    np.testing.assert_array_equal(got, want)
    ck = s.checksum()
    assert (ck["checksum"], ck["positions"], ck["win"], ck["loss"]) == (
        "%016x" % sol.stats["checksum"], sol.count, sol.stats["win"], sol.stats["loss"])
    keys = np.random.default_rng(6).integers(0, sol.count, 20000, dtype=np.uint64)
    np.testing.assert_array_equal(s.query(keys), want[keys.astype(np.int64)])
    return got


# ---- PLANES, one table -------------------------------------------------------
ABS_SHAPES = ["31:31:191",        # 192 planes, one per level: the pure chain
              "31:31:3:188",      # 774,144 positions
              "31:31:1:1:189"]    # 778,240 positions, three outer digits
ABS_FAMILIES = [(0, 8, "k_plane_flow"), (LEVELS, 8, "k_plane_resolve_x2"), (X1, 8, "k_plane_resolve"),
                (W16, 16, "k_plane_resolve")]


@pytest.mark.parametrize("flags,bits,kernel", ABS_FAMILIES)
@pytest.mark.parametrize("heaps", ABS_SHAPES)
def test_planes_last_absolute_sum(heaps, flags, bits, kernel):
    """Root digit sum 253, the last of the absolute 8-bit forms: the
    one-launch backward, one launch per level, the one-plane kernel and the
    16-bit forms each equal the oracle (so the 16-bit table equals the 8-bit
    one word for word by query)."""
    s, r = _solve(heaps, flags=flags)
    _check(s, r, heaps, bits, kernel)


def test_planes_chain_queued_solves():
    """The 192-plane chain solved four times back to back (solve_async /
    collect): the ready flags are reused under new epochs; each result has
    the blocking solve's counts, root and fingerprint, and the table left
    behind is the oracle's."""
    heaps = "31:31:191"
    s, r0 = _solve(heaps)
    _check(s, r0, heaps, 8, "k_plane_flow")
    ck0 = s.checksum()
    tickets = [s.solve_async() for _ in range(4)]
    for t in tickets:
        r = s.collect(t)
        assert (r.positions, r.edges, r.primitives, r.root_line) == (r0.positions, r0.edges, r0.primitives,
                                                                      r0.root_line)
        assert r.extra["resolve_kernel"] == "k_plane_flow" and r.extra["word_bits"] == 8
        assert s.checksum() == ck0
    _check(s, r, heaps, 8, "k_plane_flow")


REL_SHAPES = ["31:31:192", "31:31:193", "31:31:194", "31:31:195",           # sums 254 .. 257
              "31:31:3:189", "31:31:3:190", "31:31:3:191", "31:31:3:192"]


@pytest.mark.parametrize("heaps", REL_SHAPES)
def test_planes_first_relative_sums(heaps):
    """Root digit sums 254 .. 257, the first of the relative 8-bit forms, the
    root in each class of the digit sum mod 4."""
    s, r = _solve(heaps)
    _check(s, r, heaps, 8, "k_plane_resolve_x2")


@pytest.mark.parametrize("heaps", ["31:31:192", "31:31:3:189"])
def test_planes_first_relative_sum_without_runs(heaps):
    """One grid launch per level (GM_F_PLANE_NO_RUNS) instead of
    one-workgroup runs: the oracle's words, hence the default's."""
    s, r = _solve(heaps, flags=NO_RUNS)
    w = _check(s, r, heaps, 8, "k_plane_resolve_x2")
    sd, rd = _solve(heaps)
    assert rd.root_line == r.root_line and sd.checksum() == s.checksum()
    np.testing.assert_array_equal(sd.query(np.arange(len(w), dtype=np.uint64)), w)


def test_planes_first_sixteen_bit_sum():
    """Root digit sum 506, one past kPlaneRelMaxSum: 16-bit words."""
    heaps = "31:31:444"
    s, r = _solve(heaps)
    _check(s, r, heaps, 16, "k_plane_resolve")


@pytest.mark.parametrize("heaps,bits,kernel", [("31:31:191", 8, "k_plane_flow"),
                                               ("31:31:192", 8, "k_plane_resolve_x2")])
def test_planes_census_and_dump_at_the_edge(heaps, bits, kernel):
    """The census' decode of the stored forms (gm_census.h) and dump() at
    e = 253 / 254: per value and remoteness, the counts of the oracle's words
    (a decode off by one window would move a whole row)."""
    s, r = _solve(heaps)
    sol, want = _oracle(heaps)
    assert (r.extra["word_bits"], r.extra["resolve_kernel"]) == (bits, kernel)
    top = int((want >> 2).max())
    hist = np.stack([np.bincount((want >> 2)[(want & 3) == v], minlength=top + 2) for v in range(4)], axis=1)
    keys, val, rem = s.dump()
    assert len(keys) == sol.count
    got = np.stack([np.bincount(rem[val == v], minlength=top + 2) for v in range(4)], axis=1)
    np.testing.assert_array_equal(got, hist)
    np.testing.assert_array_equal(val | rem << 2, want[keys.astype(np.int64)])
    c = s.census(rem_bins=top + 1)
    np.testing.assert_array_equal(c["by_remoteness"], hist.astype(np.uint64))
    assert c["by_remoteness"][-1].sum() == 0  # nothing beyond the oracle's largest remoteness
    for v in (0, 1):
        assert c["extremes"][v]["count"] == hist[:, v].sum()
        assert c["extremes"][v]["max_remoteness"] == int((want >> 2)[(want & 3) == v].max())


# ---- PLANES, shards ----------------------------------------------------------
# The deal each case takes, from plane_shape (gm_plane_run.h): the row deal
# when heap 1 holds 32 values per rank; else the staged pipeline when the top
# heap's E = heap + 1 values split into `world` whole blocks of >= 2 (E %
# world == 0); else blocks of 8, which E must be a multiple of.  31:31:3:188
# has E = 189 = 3 * 63: two ranks get no whole blocks (nor blocks of 8), the
# plan refuses it (test_planes_two_shards_of_an_odd_top_heap_are_refused), so
# sum 253 is solved on 3 staged shards of that shape and on 2 staged shards of
# 31:31:2:189 (E = 190) besides.
SHARD_CASES = [
    (3, "31:31:3:188", 253, "staged"),
    (2, "31:31:2:189", 253, "staged"),
    (2, "31:31:3:189", 254, "staged"),
    (4, "31:31:3:191", 256, "staged"),
    (2, "31:63:159", 253, "rows"),
    (2, "31:63:160", 254, "rows"),
]


def _halo_rows(spec, world):
    """Per rank, the halo plan's rows that move anything (host only)."""
    from gamesmanmpi_amd.dist import plane_halo_plan
    return [np.flatnonzero(plane_halo_plan(spec, g, world).sum(axis=(1, 2))) for g in range(world)]


@pytest.mark.parametrize("world,heaps,total,deal", SHARD_CASES)
def test_planes_shards_at_the_form_edge(world, heaps, total, deal):
    """Shards at the last absolute and the first relative sums: every position
    answered by exactly one shard, with the oracle's word."""
    from gamesmanmpi_amd.dist import group_solve
    from gamesmanmpi_amd.games import GameSpec
    h = [int(x) for x in heaps.split(":")]
    assert sum(h) == total
    spec = GameSpec("sum_four_to_one", "heaps=" + heaps)
    # the deal, read off the host-side halo plan: the staged pipeline and the
    # row deal move halos to the next rank only, in one step per lower digit
    # sum (staged: sums of the digits below the top; rows: every plane level)
    rows = _halo_rows(spec, world)
    steps = sum(h[2:-1]) + 1 if deal == "staged" else sum(h[2:]) + 1
    assert (h[1] + 1 == 32 * world) == (deal == "rows")
    assert all(len(r) and r[-1] < steps for r in rows)
    rg, shards = group_solve(spec, world)
    sol, want = _oracle(heaps)
    assert (rg.extra["layout"], rg.extra["word_bits"]) == ("planes", 8)
    assert (rg.positions, rg.edges, rg.primitives, rg.root_line) == (sol.count, sol.edges, sol.stats["primitives"],
                                                                     sol.root_line)
    keys = np.arange(sol.count, dtype=np.uint64)
    got = np.full(sol.count, 0xFFFFFFFF, np.uint32)
    hits = np.zeros(sol.count, np.int64)
    for sh in shards:
        w = sh.query(keys)
        own = w != 0xFFFFFFFF
        got[own] = w[own]
        hits += own
    assert (hits == 1).all()
    np.testing.assert_array_equal(got, want)
    cks = [sh.checksum() for sh in shards]
    assert "%016x" % (sum(int(c["checksum"], 16) for c in cks) % (1 << 64)) == "%016x" % sol.stats["checksum"]
    assert (sum(c["win"] for c in cks), sum(c["loss"] for c in cks)) == (sol.stats["win"], sol.stats["loss"])


def test_planes_two_shards_of_an_odd_top_heap_are_refused():
    """31:31:3:188 on two ranks: 189 top values give neither two whole blocks
    nor blocks of 8 -- refused at plan time with GM_EINVAL, not dealt
    unevenly."""
    from gamesmanmpi_amd import _lib
    from gamesmanmpi_amd.games import GameSpec
    from gamesmanmpi_amd.solver import Solver
    with pytest.raises(_lib.GmError, match="whole blocks") as e:
        Solver(GameSpec("sum_four_to_one", "heaps=31:31:3:188"), rank=0, world=2)
    assert e.value.code == _lib.GM_EINVAL


# ---- DENSE -------------------------------------------------------------------
# dense_plan_bits gives the narrow forms only to tables whose bases are ALL
# powers of two (the octet and 16-prefix kernels read digits as bit fields);
# any other table has 32-bit words and the one-prefix kernel whatever its sum
# and flags.  So the switch at 253 / 254 is met by heaps of 2^k - 1 only: the
# smallest such table of sum 253 is 63:63:127:0 (2^19 positions; a heap of 0
# is a digit of base 1), its neighbour at 254 is 63:63:127:1, and 0:127:127
# is the smallest of sum 254.  With base[1] < 16 the smallest table of sum 253
# has 2^30 positions: not here.
DENSE_CASES = [
    ("63:63:127:0", 0, 8, "k_dense_resolve16p"),     # sum 253: the last 8-bit sum
    ("63:63:127:0", W16, 16, "k_dense_resolve8p"),
    ("63:63:127:0", W32, 32, "k_dense_resolve4p"),
    ("63:63:127:0", SCALAR, 32, "k_dense_resolve"),
    ("63:63:127:1", 0, 16, "k_dense_resolve8p"),     # sum 254: the first 16-bit sum
    ("0:127:127", 0, 16, "k_dense_resolve8p"),       # sum 254, heap 0 of one value
    # sums 253 / 254 on other bases: 32-bit words, whatever the flags ask for
    ("15:15:223", 0, 32, "k_dense_resolve"),         # sum 253, 57,344 positions
    ("15:15:224", 0, 32, "k_dense_resolve"),         # sum 254
    ("15:14:224", 0, 32, "k_dense_resolve"),         # sum 253, base[1] = 15
    ("3:15:235", 0, 32, "k_dense_resolve"),          # sum 253, few columns
    ("15:15:223", W16, 32, "k_dense_resolve"),
    ("15:15:223", W32, 32, "k_dense_resolve"),
    ("15:15:223", SCALAR, 32, "k_dense_resolve"),
]


@pytest.mark.parametrize("heaps,flags,bits,kernel", DENSE_CASES)
def test_dense_at_the_form_edge(heaps, flags, bits, kernel):
    """The level-major DENSE table at sums 253 / 254, each kernel family
    against the oracle."""
    s, r = _solve(heaps, layout="dense", flags=flags)
    _check(s, r, heaps, bits, kernel, layout="dense")


def test_hashed_at_the_form_edge():
    """The hashed layout (no word-width limit) as a cross-check at sum 253."""
    s, r = _solve("15:15:223", layout="hashed")
    sol, want = _oracle("15:15:223")
    assert r.extra["layout"] == "hashed"
    assert (r.positions, r.edges, r.primitives, r.root_line) == (sol.count, sol.edges, sol.stats["primitives"],
                                                                  sol.root_line)
    np.testing.assert_array_equal(s.query(np.arange(sol.count, dtype=np.uint64)), want)
    ck = s.checksum()
    assert (ck["checksum"], ck["win"], ck["loss"]) == ("%016x" % sol.stats["checksum"], sol.stats["win"],
                                                       sol.stats["loss"])
