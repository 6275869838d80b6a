"""A saved tablebase opened on the GPU (gm_solver_open_table,
Solver.open_tablebase).  The yardstick is always the
solver that wrote the file, or the host reader of the same file -- never the
opened table against itself: every reader's answer on the image against the
solver's own, on keyed files (gmtk) and indexed files (gmtb) of every word
width; the audit finding a changed word where it is; broken directories,
key orders and bitmaps refused at open; the round trip between the two
formats byte for byte; the refusals; the db command line with --gpu."""
import io
import json
import os
import shutil
from contextlib import redirect_stdout

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

SUM, TOOT, TTT, OTH = "sum_four_to_one", "toot_and_otto_bitstring", "tic_tac_toe_np", "othello_bit_new"
NO_WORD = 0xFFFFFFFF
TTT_GAME = os.path.join(ROOT, "tests", "games", "descriptor_ttt", "tic_tac_toe_np.py")
GOLDEN_CLI = os.path.join(ROOT, "tests", "golden", "db_cli_ttt_gmtk.txt")

# id -> (game, params, layout, positions or None, word bytes, key bytes or None)
KEYED = {
    "ttt": (TTT, "", "auto", 5478, 1, 3),
    "othello_4x4": (OTH, "length=4,height=4", "auto", 54089, 1, 5),
    "connect_4x3_3": ("connect_four", "length=4,height=3,connect=3", "auto", 7157, 1, None),
    "ttt_board_symmetry": (TTT, "board_symmetry=1", "auto", None, 1, None),
}
INDEXED = {
    "four_to_one_20": ("four_to_one", "start=20", "auto", 21, 1, None),
    "sum_5_4_3_dense": (SUM, "heaps=5:4:3", "dense", 120, 1, None),
    "sum_31_31_3_planes": (SUM, "heaps=31:31:3", "planes", 4096, 1, None),
    "toot_3x3_ranked": (TOOT, "length=3,height=3", "ranked", None, 1, None),
    # 2-byte words need a remoteness above 63, i.e. (remoteness = 2/3 of the digit sum) a root digit sum of
    # 96 or more: 31:31:31 (sum 93, remoteness 62) still exports 1-byte words, 31:31:63 (125, 83) does not
    "sum_31_31_63_wide": (SUM, "heaps=31:31:63", "auto", 65536, 2, None),
    "four_to_one_24700_wide": ("four_to_one", "start=24700", "auto", 24701, 4, None),  # remoteness 16,467 > 16,383
}
CASES = dict(KEYED, **INDEXED)

_made = {}


def made(case, tmp_path_factory):
    """Once per case: the solve, the file the solver wrote and the file opened."""
    if case not in _made:
        from gamesmanmpi_amd.games import GameSpec
        from gamesmanmpi_amd.solver import Solver
        game, params, layout, npos, wb, kb = CASES[case]
        spec = GameSpec(game, params)
        s = Solver(spec, layout=layout)
        r = s.solve()
        if layout != "auto":
            assert r.extra["layout"] == layout
        if npos is not None:
            assert r.positions == npos
        d = tmp_path_factory.mktemp(case)
        if case in KEYED:
            path = str(d / "solution.gmtk")
            info = s.export_keyed_tablebase(path)
        else:
            path = str(d / "solution.gmtb")
            info = s.export_tablebase(path)
        assert info["word_bytes"] == wb, info
        if kb is not None:
            assert info["key_bytes"] == kb
        t = Solver.open_tablebase(spec, path)
        assert t.info["positions"] == r.positions and t.info["bytes"] == os.path.getsize(path)
        assert t.image.numel() == max(256, os.path.getsize(path))  # the image is the file: nothing expanded
        keys = np.sort(s.positions())
        _made[case] = dict(spec=spec, s=s, r=r, t=t, path=path, info=info, keys=keys, dir=d)
    return _made[case]


@pytest.fixture()
def get(tmp_path_factory):
    return lambda case: made(case, tmp_path_factory)


def _host_reader(c):
    from gamesmanmpi_amd import db
    if c["path"].endswith(".gmtk"):
        return db.KeyedTablebase(c["path"], c["spec"] if c["spec"].symmetric else None)
    return db.Tablebase(c["path"], c["spec"])


@pytest.mark.parametrize("case", sorted(CASES))
def test_query_positions_checksum(case, get):
    c = get(case)
    s, t, keys = c["s"], c["t"], c["keys"]
    np.testing.assert_array_equal(np.sort(t.positions()), keys)
    want = s.query(keys)
    assert (want != NO_WORD).all()
    np.testing.assert_array_equal(t.query(keys), want)
    np.testing.assert_array_equal(_host_reader(c).lookup_keys(keys), want)
    # 1,000 keys that are no positions: random 64-bit ones, and neighbours of real keys
    rnd = np.random.default_rng(5).integers(0, 1 << 64, 1000, dtype=np.uint64)
    near = keys[np.random.default_rng(6).integers(0, len(keys), 1000)] + np.uint64(1)
    for absent in (rnd[~np.isin(rnd, keys)], near[~np.isin(near, keys)]):
        got = t.query(absent)
        np.testing.assert_array_equal(got, s.query(absent))
        if not c["spec"].symmetric:  # (a symmetric table answers for a key's whole orbit)
            assert (got == NO_WORD).all()
    assert t.checksum() == s.checksum()


@pytest.mark.parametrize("case", sorted(CASES))
def test_moves_line_census_audit(case, get):
    c = get(case)
    s, t, r, keys = c["s"], c["t"], c["r"], c["keys"]
    for got, want in zip(t.moves(keys), s.moves(keys)):
        np.testing.assert_array_equal(got, want)
    for got, want in zip(t.best_line(), s.best_line()):
        np.testing.assert_array_equal(got, want)
    assert len(t.best_line()[0]) >= 1
    got, want = t.census(), s.census()
    np.testing.assert_array_equal(got["by_remoteness"], want["by_remoteness"])
    np.testing.assert_array_equal(got["by_level"], want["by_level"])
    assert got["extremes"] == want["extremes"]
    assert int(got["by_level"].sum()) == r.positions
    a = t.audit()
    assert (a["positions"], a["edges"], a["mismatches"]) == (r.positions, r.edges, 0) and len(a["bad_keys"]) == 0


def test_word_and_key_widths_all_occur(get):
    assert sorted({get(c)["info"]["word_bytes"] for c in INDEXED}) == [1, 2, 4]
    assert get("ttt")["info"]["key_bytes"] == 3 and get("othello_4x4")["info"]["key_bytes"] == 5
    assert get("ttt_board_symmetry")["r"].positions < get("ttt")["r"].positions


def _parents(c, key):
    children, _, nchild, _ = c["s"].moves(c["keys"])
    hit = np.zeros(len(c["keys"]), bool)
    for j in range(children.shape[1]):
        hit |= (children[:, j] == np.uint64(key)) & (nchild > j)
    return set(c["keys"][hit].tolist())


def _corrupt_word(c, out_dir, seed):
    """A copy of the case's file with the value bits of one stored word
    changed, at a position chosen with a seeded RNG; (path, that position's key)."""
    from gamesmanmpi_amd import db
    raw = bytearray(open(c["path"], "rb").read())
    i = int(np.random.default_rng(seed).integers(0, c["r"].positions))
    if c["path"].endswith(".gmtk"):
        tk = db.KeyedTablebase(c["path"])
        key = int(tk._key_at(np.array([i]))[0])
        words_off = db.tk_header(tk.word_bytes, tk.key_bytes, tk.bucket_bits, tk.positions)[3]
        del tk
    else:
        key = int(c["keys"][i])  # sum games: index order is key order
        words_off = db.tb_header(c["spec"].tb_index_space(), 1, c["r"].positions)[3]
    assert c["info"]["word_bytes"] == 1
    raw[words_off + i] ^= 1  # WIN <-> LOSS, TIE <-> DRAW: the remoteness stays
    os.makedirs(out_dir, exist_ok=True)
    path = os.path.join(out_dir, os.path.basename(c["path"]))
    with open(path, "wb") as f:
        f.write(raw)
    return path, key


@pytest.mark.parametrize("case", ["ttt", "sum_5_4_3_dense"])
def test_a_changed_word_is_found_by_the_audit(case, get, tmp_path):
    from gamesmanmpi_amd.solver import Solver
    c = get(case)
    path, key = _corrupt_word(c, str(tmp_path / "bad"), seed=17)
    t = Solver.open_tablebase(c["spec"], path)  # its structure is intact: it opens
    assert int(t.query(np.array([key], np.uint64))[0]) == int(c["s"].query(np.array([key], np.uint64))[0]) ^ 1
    a = t.audit()
    bad = set(a["bad_keys"].tolist())
    assert a["mismatches"] == len(bad) >= 1 and a["positions"] == c["r"].positions
    assert key in bad
    assert bad <= {key} | _parents(c, key), (key, bad)


def _open_refused(spec, path, what):
    from gamesmanmpi_amd import _lib
    from gamesmanmpi_amd.solver import Solver
    with pytest.raises(_lib.GmError) as e:
        Solver.open_tablebase(spec, path)
    assert e.value.code == _lib.GM_ECORRUPT and what in str(e.value), str(e.value)


def test_broken_structure_is_refused_at_open(get, tmp_path):
    from gamesmanmpi_amd import db
    c = get("ttt")
    raw = open(c["path"], "rb").read()
    tk = db.KeyedTablebase(c["path"])
    d = np.asarray(tk.dir).astype(np.uint64)
    kb, keys_off = tk.key_bytes, db.tk_header(1, tk.key_bytes, tk.bucket_bits, tk.positions)[2]
    del tk
    assert len(d) > 7 and d[6] + 1 <= d[-1]
    bad = str(tmp_path / "dir.gmtk")
    at = 64 + 8 * 5
    with open(bad, "wb") as f:  # directory entry 5 exceeds entry 6
        f.write(raw[:at] + np.array([d[6] + 1], "<u8").tobytes() + raw[at + 8:])
    _open_refused(c["spec"], bad, "bucket 5")
    h = int(np.flatnonzero(np.diff(d.astype(np.int64)) >= 2)[3])  # a bucket of two keys or more
    a = keys_off + int(d[h]) * kb
    bad = str(tmp_path / "keys.gmtk")
    with open(bad, "wb") as f:  # its first two keys swapped
        f.write(raw[:a] + raw[a + kb:a + 2 * kb] + raw[a:a + kb] + raw[a + 2 * kb:])
    _open_refused(c["spec"], bad, "bucket %d" % h)
    c = get("sum_31_31_3_planes")
    raw = bytearray(open(c["path"], "rb").read())
    idx = int(c["keys"][len(c["keys"]) * 2 // 3])  # a reached index (sum games: index = key)
    assert raw[64 + idx // 8] >> (idx % 8) & 1
    raw[64 + idx // 8] &= ~(1 << (idx % 8)) & 0xFF  # one bitmap bit cleared, the counts left alone
    bad = str(tmp_path / "bits.gmtb")
    with open(bad, "wb") as f:
        f.write(raw)
    _open_refused(c["spec"], bad, "block %d" % (idx // 512))


def test_round_trip_between_the_formats(get, tmp_path):
    from gamesmanmpi_amd.solver import Solver
    c = get("toot_3x3_ranked")
    s, spec = c["s"], c["spec"]
    gmtk = str(tmp_path / "solver.gmtk")
    info = s.export_keyed_tablebase(gmtk)
    from_tk = Solver.open_tablebase(spec, gmtk)
    out = str(tmp_path / "from_gmtk.gmtb")
    from_tk.export_tablebase(out)
    assert open(out, "rb").read() == open(c["path"], "rb").read()
    out = str(tmp_path / "from_gmtb.gmtk")
    got = c["t"].export_keyed_tablebase(out, bucket_bits=info["bucket_bits"])
    assert got["key_bytes"] == info["key_bytes"]
    assert open(out, "rb").read() == open(gmtk, "rb").read()
    assert from_tk.checksum() == s.checksum()
    assert from_tk.audit()["mismatches"] == 0


def test_an_opened_table_is_not_solved(get, tmp_path):
    from gamesmanmpi_amd import _lib, checkpoint
    t = get("ttt")["t"]
    for call in (t.solve, lambda: t.solve_steps(0, 1), lambda: t.set_kernel_timing(True),
                 lambda: checkpoint.save(t, str(tmp_path / "ck"), 1),
                 lambda: checkpoint.solve_checkpointed(t, str(tmp_path / "ck"), 1)):
        with pytest.raises(_lib.GmError) as e:
            call()
        assert e.value.code == _lib.GM_EINVAL
    assert not os.path.exists(str(tmp_path / "ck"))
    assert t.audit()["mismatches"] == 0  # (still serving)


def _run(argv):
    from gamesmanmpi_amd.db import main
    out = io.StringIO()
    with redirect_stdout(out):
        rc = main(argv)
    return rc, out.getvalue()


def test_db_command_line(get, tmp_path):
    from gamesmanmpi_amd.solver_launcher import device_census
    c = get("ttt")
    sd = tmp_path / "sd"
    d = sd / "stats" / "0"
    os.makedirs(d)
    shutil.copy(c["path"], d / "solution.gmtk")
    with open(d / "meta.json", "w") as f:
        json.dump({"game": c["spec"].name, "params": c["spec"].params, "format": "gmtk"}, f)
    base = [str(sd), "--game", TTT_GAME]
    # without --gpu: byte for byte what the parent commit printed
    host = [_run(base + q) for q in ([], ["--moves"], ["--census"])]
    assert [rc for rc, _ in host] == [0, 0, 0]
    assert "".join(text for _, text in host) == open(GOLDEN_CLI).read()
    assert "Level" not in host[2][1]
    # with --gpu: queries and moves as the host reader prints them, the census as the solver's --census
    assert _run(base + ["--gpu"]) == host[0]
    assert _run(base + ["--gpu", "--moves"]) == host[1]
    rc, text = _run(base + ["--gpu", "--census"])
    assert rc == 0 and text == device_census(c["spec"], c["s"])[0] + "\n" and "\n       Level" in text
    rc, text = _run(base + ["--gpu", "--audit"])
    assert rc == 0 and text == "audit: %d positions, %d edges, 0 mismatches\n" % (c["r"].positions, c["r"].edges)
    bad = tmp_path / "bad"
    path, key = _corrupt_word(c, str(bad / "stats" / "0"), seed=23)
    shutil.copy(d / "meta.json", bad / "stats" / "0" / "meta.json")
    rc, text = _run([str(bad), "--game", TTT_GAME, "--gpu", "--audit"])
    lines = text.splitlines()
    assert rc == 1 and 2 <= len(lines) <= 65 and lines[0].endswith("%d mismatches" % (len(lines) - 1))
    from gamesmanmpi_amd.db import plain_position
    assert all(x.startswith("  mismatch at ((") for x in lines[1:])
    assert "  mismatch at %s" % (plain_position(c["spec"].pos_of(key)),) in lines
