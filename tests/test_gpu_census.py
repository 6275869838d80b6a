"""The census of a solved table (gm_solver_census, Solver.census): positions by
value and remoteness, by value and level, and the hardest position of each
value, on every layout.  The expected census is binned here from Solver.dump()
(the positions and query paths the other suites pin to the oracle) and
GameSpec.host_level, and for the small sum shapes from the oracle's own words
with the level taken as root digit sum - digit sum in numpy.  The direct
PLANES and RANKED kernels are also compared with the generic path, element
for element."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

X1, PLANE_LEVELS = 1024, 65536  # GM_F_PLANE_X1, GM_F_PLANE_LEVELS
SUM, TOOT, OTH = "sum_four_to_one", "toot_and_otto_bitstring", "othello_bit_new"

# id -> (game, params, layout, flags)
PLANES = {
    "planes_31_31": (SUM, "heaps=31:31", "planes", 0),                      # no outer digit
    "planes_31_31_3": (SUM, "heaps=31:31:3", "planes", 0),
    "planes_31_31_2_5": (SUM, "heaps=31:31:2:5", "planes", 0),              # mixed bases
    "planes_31_31_4_0_2": (SUM, "heaps=31:31:4:0:2", "planes", 0),          # a zero-height heap
    "planes_31_31_1x6": (SUM, "heaps=31:31:1:1:1:1:1:1", "planes", 0),      # six outer digits
    "planes_31_31_200_rel": (SUM, "heaps=31:31:200", "planes", 0),          # 8-bit relative words
    "planes_31_31_444_w16": (SUM, "heaps=31:31:444", "planes", 0),          # 16-bit words
    "planes_31_31_15_15": (SUM, "heaps=31:31:15:15", "planes", 0),
    "planes_31_31_15_15_x1": (SUM, "heaps=31:31:15:15", "planes", X1),
    "planes_31_31_15_15_levels": (SUM, "heaps=31:31:15:15", "planes", PLANE_LEVELS),
}
RANKED = {
    "toot_3x3_ranked": (TOOT, "length=3,height=3", "ranked", 0),
    "toot_3x4_ranked": (TOOT, "length=3,height=4", "ranked", 0),
    "toot_4x3_ranked": (TOOT, "length=4,height=3", "ranked", 0),
    "toot_4x4_ranked": (TOOT, "length=4,height=4", "ranked", 0),  # ~1 slot in 6 reached
}
GENERIC = {
    "ttt_hashed": ("tic_tac_toe_np", "", "hashed", 0),
    "ttt_bucketed": ("tic_tac_toe_np", "", "bucketed", 0),
    "othello_4x4_hashed": (OTH, "length=4,height=4", "hashed", 0),      # passes: a level without a piece
    "othello_4x4_bucketed": (OTH, "length=4,height=4", "bucketed", 0),
    "toot_3x4_bucketed": (TOOT, "length=3,height=4", "bucketed", 0),
    "sum_6_6_6_6_hashed": (SUM, "heaps=6:6:6:6", "hashed", 0),
    "sum_6_6_6_6_dense": (SUM, "heaps=6:6:6:6", "dense", 0),
    "four_to_one_20_hashed": ("four_to_one", "start=20", "hashed", 0),  # two-level moves, the back stack
    "four_to_one_20_dense": ("four_to_one", "start=20", "dense", 0),
}
CASES = {**PLANES, **RANKED, **GENERIC}
DIRECT = {**PLANES, **RANKED}
BIN_CASES = ["planes_31_31_3", "toot_3x4_ranked", "ttt_hashed"]
ORACLE_MAX = 210_000  # sum shapes up to ~10^5 positions (heaps=31:31:200, 205,824, is the largest)

_solved = {}


def _bin(index, value, rows):
    out = np.zeros((rows, 4), np.uint64)
    np.add.at(out, (index.astype(np.int64), value.astype(np.int64)), 1)
    return out


def solved(case):
    """One solve per case for the whole module: spec, solver, SolveResult, the
    dump (keys, value, remoteness), the keys' levels and the default census."""
    if case not in _solved:
        from gamesmanmpi_amd.games import GameSpec
        from gamesmanmpi_amd.solver import Solver
        game, params, layout, flags = CASES[case]
        spec = GameSpec(game, params)
        s = Solver(spec, layout=layout, flags=flags)
        r = s.solve()
        assert r.extra["layout"] == layout
        keys, val, rem = s.dump()
        _solved[case] = dict(spec=spec, s=s, r=r, keys=keys, val=val, rem=rem,
                             lev=spec.host_level(keys), census=s.census())
    return _solved[case]


def expected(c, rem_bins):
    """(by_remoteness, by_level, extremes) from the dump."""
    nlev = int(c["s"].plan.max_levels)
    by_rem = _bin(np.minimum(c["rem"], rem_bins), c["val"], rem_bins + 1)
    by_lev = _bin(c["lev"], c["val"], nlev)
    ext = []
    for v in range(4):
        m = c["val"] == v
        if not m.any():
            ext.append({"count": 0, "max_remoteness": 0, "key": None})
            continue
        top = int(c["rem"][m].max())
        ext.append({"count": int(m.sum()), "max_remoteness": top,
                    "key": int(c["keys"][m & (c["rem"] == top)].min())})
    return by_rem, by_lev, ext


def assert_census(got, want):
    by_rem, by_lev, ext = want
    assert got["by_remoteness"].dtype == np.uint64 and got["by_remoteness"].shape == by_rem.shape
    np.testing.assert_array_equal(got["by_remoteness"], by_rem)
    if by_lev is not None:
        assert got["by_level"].dtype == np.uint64 and got["by_level"].shape == by_lev.shape
        np.testing.assert_array_equal(got["by_level"], by_lev)
    if ext is not None:
        assert got["extremes"] == ext


def same_census(a, b):
    np.testing.assert_array_equal(a["by_remoteness"], b["by_remoteness"])
    np.testing.assert_array_equal(a["by_level"], b["by_level"])
    assert a["extremes"] == b["extremes"]


@pytest.mark.parametrize("case", sorted(CASES))
def test_census_matches_dump(case):
    c = solved(case)
    s, r = c["s"], c["r"]
    if case.endswith("_rel"):  # as test_planes_relative_match_oracle
        assert r.extra["word_bits"] == 8 and r.extra["resolve_kernel"] == "k_plane_resolve_x2"
    if case.endswith("_w16"):
        assert r.extra["word_bits"] == 16
    nlev = int(s.plan.max_levels)
    rem_bins = min(nlev + 1, 65536)
    got = c["census"]
    assert got["by_remoteness"].shape == (rem_bins + 1, 4) and got["by_level"].shape == (nlev, 4)
    assert_census(got, expected(c, rem_bins))
    # consistency
    by_rem, by_lev, ext = got["by_remoteness"], got["by_level"], got["extremes"]
    assert int(by_rem.sum()) == int(by_lev.sum()) == r.positions == len(c["keys"])
    ck = s.checksum()
    cols = [ck["win"], ck["loss"], ck["tie"], ck["draw"]]
    assert [int(x) for x in by_rem.sum(0)] == cols and [int(x) for x in by_lev.sum(0)] == cols
    assert [e["count"] for e in ext] == cols
    assert int(by_rem[0].sum()) == r.primitives
    assert int(by_lev[0].sum()) == 1
    assert int(by_lev[0][r.root_value]) == 1 and int(by_rem[r.root_remoteness][r.root_value]) >= 1
    assert int(by_rem[rem_bins].sum()) == 0  # remoteness <= levels: nothing overflows the default
    for v in (0, 1):  # the WIN and LOSS witnesses are that many moves from the end
        if ext[v]["count"]:
            line = s.best_line(ext[v]["key"])
            assert len(line[0]) == ext[v]["max_remoteness"] + 1, v


def _heaps(case):
    return [int(h) for h in CASES[case][1].split("=")[1].split(":")]


def _ranks(case):
    return int(np.prod([h + 1 for h in _heaps(case)], dtype=np.int64))


@pytest.mark.parametrize("case", sorted(c for c in CASES if CASES[c][0] == SUM and _ranks(c) <= ORACLE_MAX))
def test_census_matches_oracle_words(case):
    """The small sum shapes against the oracle's own words; the level is the
    root digit sum - the rank's digit sum, computed here."""
    heaps, n = _heaps(case), _ranks(case)
    from oracle.oracle import Game
    sol = Game(SUM, CASES[case][1]).solve_rows()
    sol.refresh(True)
    assert sol.count == n
    w = np.array([sol.word(k) for k in range(n)], np.uint32)
    k, dsum = np.arange(n, dtype=np.int64), np.zeros(n, np.int64)
    for h in heaps:
        dsum += k % (h + 1)
        k //= h + 1
    c = solved(case)
    nlev = int(c["s"].plan.max_levels)
    rem_bins = min(nlev + 1, 65536)
    val, rem = (w & 3).astype(np.int64), (w >> 2).astype(np.int64)
    assert_census(c["census"], (_bin(np.minimum(rem, rem_bins), val, rem_bins + 1),
                                _bin(sum(heaps) - dsum, val, nlev), None))
    for v, e in enumerate(c["census"]["extremes"]):
        m = val == v
        assert e["count"] == int(m.sum())
        if e["count"]:
            top = int(rem[m].max())
            assert (e["max_remoteness"], e["key"]) == (top, int(np.nonzero(m & (rem == top))[0][0]))


@pytest.mark.parametrize("case", sorted(DIRECT))
def test_direct_equals_generic(case):
    c = solved(case)
    same_census(c["s"].census(generic=True), c["census"])


def test_plane_kernel_families_give_one_census():
    base = solved("planes_31_31_15_15")
    assert base["r"].extra["resolve_kernel"] == "k_plane_flow"
    for other in ("planes_31_31_15_15_x1", "planes_31_31_15_15_levels"):
        o = solved(other)
        assert o["r"].extra["resolve_kernel"] != "k_plane_flow"
        same_census(o["census"], base["census"])


@pytest.mark.parametrize("case", BIN_CASES)
def test_bins(case):
    c = solved(case)
    s = c["s"]
    top = int(c["rem"].max())
    full = s.census(rem_bins=top + 1)
    assert int(full["by_remoteness"][top + 1].sum()) == 0 and int(full["by_remoteness"][top].sum()) > 0
    assert_census(full, expected(c, top + 1))
    mid = top // 2
    assert 0 < mid < top
    cut = s.census(rem_bins=mid)
    assert_census(cut, expected(c, mid))
    np.testing.assert_array_equal(cut["by_remoteness"][mid], full["by_remoteness"][mid:].sum(0))
    assert cut["extremes"] == full["extremes"]  # the largest remoteness stays exact
    zero = s.census(rem_bins=0)
    assert zero["by_remoteness"].shape == (1, 4)
    assert_census(zero, expected(c, 0))
    # past the LDS threshold: the remoteness table is counted with global atomics
    wide = s.census(rem_bins=65536)
    assert wide["by_remoteness"].shape == (65537, 4)
    np.testing.assert_array_equal(wide["by_remoteness"][:top + 2], full["by_remoteness"])
    assert int(wide["by_remoteness"][top + 2:].sum()) == 0
    np.testing.assert_array_equal(wide["by_level"], full["by_level"])
    assert wide["extremes"] == full["extremes"]
    if case in DIRECT:
        for bins in (mid, 0, 65536):
            same_census(s.census(rem_bins=bins, generic=True), s.census(rem_bins=bins))
    # by_level NULL, extremes NULL
    nolev = s.census(levels=False)
    assert nolev["by_level"] is None
    np.testing.assert_array_equal(nolev["by_remoteness"], c["census"]["by_remoteness"])
    assert nolev["extremes"] == c["census"]["extremes"]
    noext = s.census(extremes=False)
    assert noext["extremes"] is None
    np.testing.assert_array_equal(noext["by_remoteness"], c["census"]["by_remoteness"])
    np.testing.assert_array_equal(noext["by_level"], c["census"]["by_level"])


@pytest.mark.parametrize("case", BIN_CASES)
def test_twice_on_one_solver(case):
    """The call zeroes its buffers and its scratch words: a second census, and
    one after a second solve, give the same arrays."""
    c = solved(case)
    s = c["s"]
    same_census(s.census(), c["census"])
    r2 = s.solve()
    assert r2.root_line == c["r"].root_line
    same_census(s.census(), c["census"])
    same_census(s.census(generic=True), c["census"])


def _raw_census(s, levels):
    import torch
    from gamesmanmpi_amd import _lib
    rd = torch.full((8 * 4,), -1, dtype=torch.int64, device=s.device)
    ld = torch.full((max(1, levels) * 4,), -1, dtype=torch.int64, device=s.device)
    rc = _lib.load().gm_solver_census(s.handle, 0, rd.data_ptr(), 7, ld.data_ptr(), levels, None)
    torch.cuda.synchronize()
    return rc, rd.cpu().numpy(), ld.cpu().numpy()


def test_refusals():
    from gamesmanmpi_amd import _lib
    from gamesmanmpi_amd.dist import group_solve
    from gamesmanmpi_amd.games import GameSpec
    from gamesmanmpi_amd.solver import Solver
    L = _lib.load()
    # fewer level rows than the game has levels: nothing is launched, nothing written
    s = solved("ttt_hashed")["s"]
    nlev = int(s.plan.max_levels)
    rc, rd, ld = _raw_census(s, nlev - 1)
    assert rc == _lib.GM_EINVAL and b"level" in L.gm_last_error()
    assert (rd == -1).all() and (ld == -1).all()
    rc, rd, ld = _raw_census(s, nlev)
    assert rc == 0 and int(rd.sum()) == int(ld.sum()) == 5478
    # never solved, stopped early, a shard
    fresh = Solver(GameSpec("tic_tac_toe_np"), layout="hashed")
    _, shards = group_solve(GameSpec(SUM, "heaps=7:7:7:15"), 2)
    for x in [fresh] + list(shards):
        with pytest.raises(_lib.GmError) as e:
            x.census()
        assert e.value.code == _lib.GM_EINVAL and "gm_solver_census" in str(e.value)
        rc, rd, ld = _raw_census(x, int(x.plan.max_levels))
        assert rc == _lib.GM_EINVAL and (rd == -1).all() and (ld == -1).all()
    assert fresh.solve_steps(0, 3) is None
    with pytest.raises(_lib.GmError) as e:
        fresh.census()
    assert e.value.code == _lib.GM_EINVAL
    fresh.solve()
    same_census(fresh.census(), solved("ttt_hashed")["census"])
