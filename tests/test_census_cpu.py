"""The census on the host (gamesmanmpi_amd/db.py census_of / format_census,
`python -m gamesmanmpi_amd.db DIR --game GAME --census`) against a bincount of
the oracle's words, and the host-only parts of gm_solver_census: the export,
the launcher's and the db tool's flags."""
import io
import json
import os
import subprocess
import sys
from contextlib import redirect_stdout

import numpy as np
import pytest

from conftest import ROOT

OWN_SUM = os.path.join(ROOT, "gamesmanmpi_amd", "games", "sum_four_to_one.py")
HEAPS = (4, 6, 3)


def _write_rank(root, rank, **arrays):
    d = os.path.join(root, "stats", str(rank))
    os.makedirs(d, exist_ok=True)
    np.savez_compressed(os.path.join(d, "solution.npz"), **arrays)
    with open(os.path.join(d, "meta.json"), "w") as f:
        json.dump({"owned_by_rank": rank}, f)


@pytest.fixture(scope="module")
def oracle_table():
    """(keys, value, remoteness, level) of heaps=4:6:3 from the oracle; the
    level is the root digit sum - the rank's digit sum, in numpy."""
    from oracle.oracle import Game
    sol = Game("sum_four_to_one", "heaps=4:6:3").solve()
    keys = np.arange(5 * 7 * 4, dtype=np.uint64)
    vr = np.array([sol.lookup(str(k).encode()) for k in keys.tolist()])
    k = keys.astype(np.int64)
    dsum = k % 5 + (k // 5) % 7 + k // 35
    return keys, vr[:, 0].astype(np.uint8), vr[:, 1].astype(np.uint32), sum(HEAPS) - dsum


def _solution_dir(tmp_path, table):
    keys, val, rem, _ = table
    game = tmp_path / "sum_four_to_one.py"
    game.write_text(open(OWN_SUM).read().replace(
        "HEAPS = (31, 31, 31, 31, 31, 31)", "HEAPS = (4, 6, 3)"))
    for r in range(2):  # two "ranks", interleaved ownership
        m = keys % 2 == r
        _write_rank(tmp_path / "sd", r, keys=keys[m], value=val[m], remoteness=rem[m])
    return str(tmp_path / "sd"), str(game)


def _parse(text):
    """{title: {row label: [win, lose, tie, draw, total]}} of format_census' text."""
    tables, cur = {}, None
    for line in text.splitlines():
        f = line.split()
        if not f:
            continue
        if f[1:] == ["Win", "Lose", "Tie", "Draw", "Total"]:
            cur = tables.setdefault(f[0], {})
        else:
            assert len(f) == 6, line
            cur[f[0]] = [int(x) for x in f[1:]]
    return tables


def _expect(index, value, rows):
    """{label: [w, l, t, d, total]} of the non-empty rows of a bincount."""
    want = {}
    for i in range(rows):
        row = [int(((index == i) & (value == v)).sum()) for v in range(4)]
        if sum(row):
            want[str(i)] = row + [sum(row)]
    return want


def test_db_census_matches_oracle_bincount(tmp_path, oracle_table):
    from gamesmanmpi_amd.db import main
    keys, val, rem, lev = oracle_table
    sd, game = _solution_dir(tmp_path, oracle_table)
    out = io.StringIO()
    with redirect_stdout(out):
        rc = main([sd, "--game", game, "--census"])
    assert rc == 0
    t = _parse(out.getvalue())
    assert sorted(t) == ["Level", "Remoteness"]
    total = [int((val == v).sum()) for v in range(4)] + [len(keys)]
    for title, index in (("Remoteness", rem.astype(np.int64)), ("Level", lev)):
        want = _expect(index, val, int(index.max()) + 1)
        want["Total"] = total
        assert t[title] == want, title
    assert t["Remoteness"]["Total"][4] == t["Level"]["Total"][4] == len(keys) == 140
    # level 0 is the root alone, remoteness 0 the primitive alone
    assert t["Level"]["0"][4] == 1 and t["Remoteness"]["0"] == [0, 1, 0, 0, 1]


def test_db_census_overflow_row(tmp_path, oracle_table):
    from gamesmanmpi_amd.db import census_of, format_census, main
    keys, val, rem, lev = oracle_table
    top = int(rem.max())
    full = census_of(val, rem, lev)
    assert full["by_remoteness"].shape == (top + 2, 4) and full["by_remoteness"][top + 1].sum() == 0
    assert full["by_level"].shape == (sum(HEAPS) + 1, 4)
    mid = top // 2
    cut = census_of(val, rem, lev, rem_bins=mid)
    assert cut["by_remoteness"].shape == (mid + 1, 4)
    np.testing.assert_array_equal(cut["by_remoteness"][:mid], full["by_remoteness"][:mid])
    np.testing.assert_array_equal(cut["by_remoteness"][mid], full["by_remoteness"][mid:].sum(0))
    np.testing.assert_array_equal(cut["by_level"], full["by_level"])
    zero = census_of(val, rem, rem_bins=0)
    assert zero["by_level"] is None
    np.testing.assert_array_equal(zero["by_remoteness"], full["by_remoteness"].sum(0)[None, :])
    assert int(zero["by_remoteness"].sum()) == len(keys)
    # the tool prints the overflow row as ">=N", and the totals do not change
    sd, game = _solution_dir(tmp_path, oracle_table)
    out = io.StringIO()
    with redirect_stdout(out):
        main([sd, "--game", game, "--census", "--rem-bins", str(mid)])
    t = _parse(out.getvalue())
    tail = [int(((rem >= mid) & (val == v)).sum()) for v in range(4)]
    assert t["Remoteness"][">=%d" % mid] == tail + [sum(tail)]
    assert str(mid) not in t["Remoteness"] and t["Remoteness"]["Total"][4] == len(keys)
    assert _parse(format_census(cut["by_remoteness"], cut["by_level"])) == t


def test_db_census_graph_table_has_no_levels(tmp_path):
    from gamesmanmpi_amd.db import main
    _write_rank(tmp_path / "sd", 0, names=np.array(["a", "b", "c"]),
                value=np.array([0, 1, 0], np.uint8), remoteness=np.array([3, 0, 1], np.uint32))
    game = tmp_path / "some_game.py"  # no descriptor: keyed by str(position)
    game.write_text("def initial_position():\n    return 'a'\n")
    out = io.StringIO()
    with redirect_stdout(out):
        rc = main([str(tmp_path / "sd"), "--game", str(game), "--census"])
    assert rc == 0
    t = _parse(out.getvalue())
    assert list(t) == ["Remoteness"]
    assert t["Remoteness"] == {"0": [0, 1, 0, 0, 1], "1": [1, 0, 0, 0, 1], "3": [1, 0, 0, 0, 1],
                               "Total": [2, 1, 0, 0, 3]}


def test_census_is_exported():
    from gamesmanmpi_amd import _lib
    assert "gm_solver_census" in _lib.EXPORTS
    assert getattr(_lib.load(), "gm_solver_census") is not None
    with open(os.path.join(ROOT, "include", "gamesman.h")) as f:
        assert "int gm_solver_census(" in f.read()
    assert _lib.GM_CENSUS_GENERIC == 1


def test_launcher_accepts_census():
    from gamesmanmpi_amd.solver_launcher import build_parser, check_analysis_args
    a = build_parser().parse_args(["g.py", "--census", "--json"])
    assert a.census and a.json
    assert not build_parser().parse_args(["g.py"]).census
    check_analysis_args(a, 1)
    check_analysis_args(a, 1, descriptor=False)  # graph solves are counted on the host
    with pytest.raises(SystemExit) as e:
        check_analysis_args(a, 2)
    assert "--census: one-GPU solves only" in str(e.value)


def test_launcher_census_report_of_a_graph_solve():
    from gamesmanmpi_amd.solver_launcher import host_census
    text, obj = host_census(np.array(["b", "a", "c"]), np.array([0, 0, 1], np.uint8),
                            np.array([3, 3, 0], np.uint32))
    assert "longest WIN: a in 3 moves" in text.splitlines()
    assert "longest LOSS: c in 0 moves" in text.splitlines()
    assert not any(line.startswith("longest TIE") for line in text.splitlines())
    assert obj["by_level"] is None and obj["by_remoteness"][3] == [2, 0, 0, 0]
    assert obj["witnesses"][0] == {"value": "WIN", "count": 2, "max_remoteness": 3, "position": "a"}
    assert obj["witnesses"][2]["count"] == 0 and obj["witnesses"][2]["position"] is None
    json.dumps(obj)


def test_db_help_lists_census():
    r = subprocess.run([sys.executable, "-m", "gamesmanmpi_amd.db", "--help"], cwd=ROOT,
                       capture_output=True, text=True, check=True)
    assert "--census" in r.stdout
