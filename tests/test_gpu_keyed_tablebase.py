"""The device export of the keyed tablebase (gm_solver_export_keyed,
Solver.export_keyed / export_keyed_tablebase) on every layout: the written
file against the pure-numpy writer fed with Solver.dump(), byte for byte, at
the default bucket_bits, at bucket counts on both sides of the LDS histogram's
limit (2^13 counters) that leave most buckets empty, and at bucket_bits 0
where one bucket holds the table; the file read back through
db.KeyedTablebase; the BUCKETED side-by-side path against the query path; the
refusals; the launcher's -sd DIR --tablebase on a game without an index."""
import ctypes
import io
import os
from contextlib import redirect_stdout

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

SUM, TOOT, TTT, OTH = "sum_four_to_one", "toot_and_otto_bitstring", "tic_tac_toe_np", "othello_bit_new"
NO_WORD = 0xFFFFFFFF
CAP = 1024  # positions of one bucket

# id -> (game, params, layout)
CASES = {
    "ttt_bucketed": (TTT, "", "bucketed"),
    "ttt_hashed": (TTT, "", "hashed"),
    "mttt_auto": ("mttt", "", "auto"),
    "othello_4x4_bucketed": (OTH, "length=4,height=4", "bucketed"),
    "othello_4x4_hashed": (OTH, "length=4,height=4", "hashed"),
    "othello_4x4_symmetric": (OTH, "length=4,height=4,symmetry=1", "auto"),
    "toot_3x4_bucketed": (TOOT, "length=3,height=4", "bucketed"),
    "toot_3x4_ranked": (TOOT, "length=3,height=4", "ranked"),
    "planes_31_31": (SUM, "heaps=31:31", "planes"),  # 1,024 positions: a bucket of exactly the capacity at b = 0
    "sum_6_6_6_6_dense": (SUM, "heaps=6:6:6:6", "dense"),
}
BUCKETED = sorted(c for c in CASES if CASES[c][2] == "bucketed")

_solved = {}


def solved(case):
    """One solve per case for the whole module, with its dump."""
    if case not in _solved:
        from gamesmanmpi_amd import db
        from gamesmanmpi_amd.games import GameSpec
        from gamesmanmpi_amd.solver import Solver
        game, params, layout = CASES[case]
        spec = GameSpec(game, params)
        s = Solver(spec, layout=layout)
        r = s.solve()
        if layout != "auto":
            assert r.extra["layout"] == layout
        keys, val, rem = s.dump()
        _solved[case] = dict(spec=spec, s=s, r=r, keys=keys, words=val.astype(np.uint32) | (rem << 2),
                             wb=db.tb_word_bytes(int(rem.max())))
    return _solved[case]


def _bits(case):
    """The bucket_bits a case is exported at: the default (None), about one
    position per bucket -- most buckets empty or of one key -- and, for
    tic-tac-toe, 2^13 and 2^14 buckets (the last LDS histogram, the first in
    global memory); 0 where one bucket can hold the table."""
    n = len(solved(case)["keys"])
    bits = [None, n.bit_length()]
    if case.startswith("ttt"):
        bits += [13, 14]
    if n <= CAP:
        bits.append(0)
    return bits


@pytest.mark.parametrize("case", sorted(CASES))
def test_file_is_the_numpy_writers(case, tmp_path):
    """1. byte-identical to db.write_keyed_tablebase fed with Solver.dump();
    exported twice, the same bytes.  2. every dumped key reads back its word,
    absent keys read NO_WORD."""
    from gamesmanmpi_amd import db
    c = solved(case)
    s, keys, words, wb = c["s"], c["keys"], c["words"], c["wb"]
    n = len(keys)
    assert n == int(c["r"].positions)
    have = set(keys.tolist())
    absent = np.array([k ^ 1 for k in keys[:4096].tolist() if k ^ 1 not in have], np.uint64)
    rnd = np.random.default_rng(3).integers(0, 1 << 64, 1024, dtype=np.uint64)
    rnd = rnd[~np.isin(rnd, keys)]
    for bits in _bits(case):
        got, want = str(tmp_path / "dev.gmtk"), str(tmp_path / "host.gmtk")
        info = s.export_keyed_tablebase(got, bucket_bits=bits)
        b = db.tk_default_bits(n) if bits is None else bits
        assert info["bucket_bits"] == b and info["positions"] == n and info["word_bytes"] == wb
        assert info["key_bytes"] == db.tk_key_bytes(keys)
        assert os.path.getsize(got) == info["bytes"] and not os.path.exists(got + ".tmp")
        assert db.write_keyed_tablebase(want, keys, words, wb, b) == b
        raw = open(got, "rb").read()
        assert raw == open(want, "rb").read(), (case, bits)
        if bits is None:
            s.export_keyed_tablebase(got)
            assert open(got, "rb").read() == raw
        tb = db.KeyedTablebase(got)
        np.testing.assert_array_equal(tb.lookup_keys(keys), words)
        assert (tb.lookup_keys(absent) == NO_WORD).all() and (tb.lookup_keys(rnd) == NO_WORD).all()
        if b >= 8:
            assert (np.diff(np.asarray(tb.dir).astype(np.int64)) == 0).any() == (bits is not None)
        del tb
    if case == "planes_31_31":
        assert n == CAP and 0 in _bits(case)


def test_keyed_agrees_with_the_indexed_tablebase(tmp_path):
    """2. toot 3x4 RANKED: the .gmtk and the .gmtb of one solver answer alike."""
    from gamesmanmpi_amd import db
    c = solved("toot_3x4_ranked")
    tk, tb = str(tmp_path / "solution.gmtk"), str(tmp_path / "solution.gmtb")
    c["s"].export_keyed_tablebase(tk)
    c["s"].export_tablebase(tb)
    a, b = db.KeyedTablebase(tk), db.Tablebase(tb, c["spec"])
    q = np.concatenate([c["keys"], c["keys"] ^ np.uint64(1), c["keys"][:512] | np.uint64(1 << 40)])
    np.testing.assert_array_equal(a.lookup_keys(q), b.lookup_keys(q))
    np.testing.assert_array_equal(a.by_remoteness(), b.by_remoteness())


@pytest.mark.parametrize("case", BUCKETED)
def test_direct_equals_generic(case):
    """3. BUCKETED: K[i] / W[i] side by side against the query path, section
    for section."""
    from gamesmanmpi_amd import db
    c = solved(case)
    n = len(c["keys"])
    for b in (db.tk_default_bits(n), n.bit_length()):
        direct = c["s"].export_keyed(b, c["wb"])
        generic = c["s"].export_keyed(b, c["wb"], generic=True)
        for x, y in zip(direct, generic):
            assert x.dtype == y.dtype and x.shape == y.shape
            np.testing.assert_array_equal(x.cpu().numpy(), y.cpu().numpy())
        assert direct[0].numel() == (1 << b) + 1 and int(direct[0][-1]) == n
        assert direct[1].numel() == n * db.tk_key_bytes(c["keys"]) and direct[2].numel() == n * c["wb"]


def _call(s, how, b, wb, cap):
    """The ABI call with room for `cap` positions: (rc, out, keys tensor)."""
    import torch
    from gamesmanmpi_amd import _lib
    dev = s.device
    stage = torch.zeros(max(2, cap * 3 // 2 + 1), dtype=torch.int64, device=dev)
    d = torch.zeros((1 << b) + 1, dtype=torch.int64, device=dev)
    keys = torch.full((max(16, cap * 8),), 0xAB, dtype=torch.uint8, device=dev)
    words = torch.full((max(16, cap * wb),), 0xAB, dtype=torch.uint8, device=dev)
    out = np.zeros(4, np.uint64)
    with torch.cuda.device(dev):
        rc = _lib.load().gm_solver_export_keyed(s.handle, how, b, wb, stage.data_ptr(), d.data_ptr(),
                                                keys.data_ptr(), words.data_ptr(), cap, out.ctypes.data)
    return rc, out, d, keys, words


def test_refusals():
    from gamesmanmpi_amd import _lib
    from gamesmanmpi_amd.games import GameSpec
    from gamesmanmpi_amd.solver import Solver
    err = lambda: _lib.load().gm_last_error().decode()  # noqa: E731
    # one bucket of 2,048 positions: over the capacity, nothing written past the directory
    s = Solver(GameSpec(SUM, "heaps=31:31:1"), layout="planes")
    assert s.solve().positions == 2048
    for how in (0, _lib.GM_EXPORT_GENERIC):
        rc, out, d, keys, words = _call(s, how, 0, 1, 2048)
        assert rc == _lib.GM_EFULL and int(out[2]) == 2048 and int(out[0]) == 2048
        assert "raise bucket_bits" in err()
        assert d.cpu().tolist() == [0, 2048]
        assert (keys.cpu().numpy() == 0xAB).all() and (words.cpu().numpy() == 0xAB).all()
    rc, out, _, _, _ = _call(s, 0, 1, 1, 2048)  # two buckets of about 1,024: whichever is larger is over
    assert (rc == _lib.GM_EFULL) == (int(out[2]) > CAP) and int(out[2]) >= 1024
    rc, out, d, _, _ = _call(s, 0, 2, 1, 2048)
    assert rc == 0 and int(out[0]) == 2048 and int(out[1]) == 2 and int(out[3]) == int(s.dump()[2].max())
    # a short cap: GM_EFULL with the count needed
    c = solved("ttt_bucketed")
    n = len(c["keys"])
    for how in (0, _lib.GM_EXPORT_GENERIC):
        rc, out, d, keys, _ = _call(c["s"], how, 5, 1, 64)
        assert rc == _lib.GM_EFULL and int(out[0]) == n and int(out[2]) <= CAP
        assert int(d[-1]) == n and (keys.cpu().numpy() == 0xAB).all()
    with pytest.raises(_lib.TableFull):
        c["s"].export_keyed(5, 1, cap=n - 1)
    # remoteness >= 131 in one byte
    big = Solver(GameSpec(SUM, "heaps=31:31:200"), layout="planes")
    big.solve()
    top = int(big.dump()[2].max())
    assert top >= 131
    for generic in (False, True):
        with pytest.raises(_lib.GmError) as ei:
            big.export_keyed(10, 1, generic=generic)
        assert ei.value.code == _lib.GM_EINVAL and "remoteness %d" % top in str(ei.value)
    # bad arguments: a word width that is none, more than 32 bucket bits, a flag that is none
    for how, b, wb in ((0, 5, 3), (0, 33, 1), (2, 5, 1)):
        rc = _lib.load().gm_solver_export_keyed(c["s"].handle, how, b, wb, None, None, None, None, 0,
                                                np.zeros(4, np.uint64).ctypes.data)
        assert rc == _lib.GM_EINVAL
    # an unsolved solver, a shard
    fresh = Solver(GameSpec(TTT, ""))
    with pytest.raises(_lib.GmError) as ei:
        fresh.export_keyed(5, 1, cap=6000)
    assert ei.value.code == _lib.GM_EINVAL
    from gamesmanmpi_amd.dist import group_solve
    _, shards = group_solve(GameSpec(SUM, "heaps=7:7:7:15"), 2)  # (solved shards: the refusal is the shard's)
    for shard in shards:
        with pytest.raises(_lib.GmError) as ei:
            shard.export_keyed(5, 1, cap=8192)
        assert ei.value.code == _lib.GM_EINVAL and "gm_solver_export_keyed" in str(ei.value)


def test_retry_on_a_full_bucket(tmp_path):
    """5. bucket_bits=1 on tic-tac-toe (2,739 positions per bucket) grows to a
    bucket_bits whose largest bucket fits."""
    from gamesmanmpi_amd import db
    c = solved("ttt_bucketed")
    path = str(tmp_path / "solution.gmtk")
    info = c["s"].export_keyed_tablebase(path, bucket_bits=1)
    assert 3 <= info["bucket_bits"] <= 4
    tb = db.KeyedTablebase(path)
    assert tb.bucket_bits == info["bucket_bits"]
    assert int(np.diff(np.asarray(tb.dir).astype(np.int64)).max()) <= CAP
    np.testing.assert_array_equal(tb.lookup_keys(c["keys"]), c["words"])
    want = str(tmp_path / "host.gmtk")
    db.write_keyed_tablebase(want, c["keys"], c["words"], c["wb"], info["bucket_bits"])
    assert open(path, "rb").read() == open(want, "rb").read()


def _run(main, argv):
    out = io.StringIO()
    with redirect_stdout(out):
        rc = main(argv)
    return rc, out.getvalue().splitlines()


def test_launcher_writes_a_keyed_tablebase(tmp_path):
    """6. -sd DIR --tablebase on tic-tac-toe, then the db command line on DIR."""
    from gamesmanmpi_amd import db, solver_launcher as sl
    game = os.path.join(ROOT, "tests", "games", "descriptor_ttt", "tic_tac_toe_np.py")
    sd = str(tmp_path / "sd")
    rc, lines = _run(sl.main, [game, "-sd", sd, "--tablebase", "--no-verify"])
    assert rc == 0
    root_line = lines[0]
    c = solved("ttt_bucketed")
    assert root_line == c["r"].root_line == "TIE in 9 moves"
    d = os.path.join(sd, "stats", "0")
    assert sorted(os.listdir(d)) == ["meta.json", "solution.gmtk"]
    rc, lines = _run(db.main, [sd, "--game", game])
    assert rc == 0 and len(lines) == 1 and lines[0].endswith(": " + root_line)
    rc, lines = _run(db.main, [sd, "--game", game, "--moves"])
    assert rc == 0 and len(lines) == 10 and sum(x.endswith(" *") for x in lines) == 1
    opened = db.SolutionDB(sd)
    assert opened.meta["format"] == "gmtk" and len(opened) == len(c["keys"])
    assert isinstance(opened.tablebase, db.KeyedTablebase)
    rc, lines = _run(db.main, [sd, "--game", game, "--census"])
    assert rc == 0 and lines[-1].split()[-1] == str(len(c["keys"]))
