"""The keyed tablebase on the host: gm_mix64 against its numpy restatement,
the file format through the pure-numpy writer and the mmap reader
(gamesmanmpi_amd/db.py: write_keyed_tablebase / KeyedTablebase) on the
oracle's solutions of tic-tac-toe and othello 4x4, damaged files, and the db
command line on a converted directory.  No GPU."""
import ctypes
import io
import json
import os
from contextlib import redirect_stdout

import numpy as np
import pytest

from conftest import ROOT

TTT_GAME = os.path.join(ROOT, "tests", "games", "descriptor_ttt", "tic_tac_toe_np.py")
NO_WORD = 0xFFFFFFFF
CASES = {"ttt": ("tic_tac_toe_np", "", 5478), "othello_4x4": ("othello_bit_new", "length=4,height=4", 54089)}

_solutions = {}


def _oracle(case):
    """(spec, keys u64, value, remoteness, solution) of the oracle's solve, once per case."""
    if case not in _solutions:
        from gamesmanmpi_amd.games import GameSpec
        from oracle.oracle import Game  # checker only
        name, params, count = CASES[case]
        spec = GameSpec(name, params)
        sol = Game(name, params).solve(1 << 22)
        canon, clen, val, rem = sol.dump(stride=32)
        assert sol.count == count
        _solutions[case] = (spec, spec.encode_batch(canon, clen), val, rem, sol)
    return _solutions[case]


def _words(val, rem):
    return val.astype(np.uint32) | (rem.astype(np.uint32) << 2)


def test_mix64_matches_the_library():
    from gamesmanmpi_amd import _lib, db
    rng = np.random.default_rng(7)
    keys = np.concatenate([np.array([0, 0xFFFFFFFFFFFFFFFF], np.uint64),
                           rng.integers(0, 1 << 64, 4096, dtype=np.uint64)])
    out = np.zeros(len(keys), np.uint64)
    assert _lib.load().gm_mix64(keys.ctypes.data, len(keys), out.ctypes.data) == 0
    np.testing.assert_array_equal(out, db.mix64(keys))
    assert int(out[0]) == 0 and len(np.unique(out)) == len(np.unique(keys))  # (a bijection fixes 0)
    # the bucket is the hash's top bits
    np.testing.assert_array_equal(db.tk_bucket(keys, 12), (out >> np.uint64(52)).astype(np.int64))
    assert (db.tk_bucket(keys, 0) == 0).all()


@pytest.mark.parametrize("case,bits", [("ttt", None), ("ttt", 0), ("ttt", 12), ("othello_4x4", None)])
def test_round_trip(tmp_path, case, bits):
    from gamesmanmpi_amd import db
    spec, keys, val, rem, sol = _oracle(case)
    words = _words(val, rem)
    wb = db.tb_word_bytes(int(rem.max()))
    path = str(tmp_path / "solution.gmtk")
    b = db.write_keyed_tablebase(path, keys, words, wb, bits)
    assert not os.path.exists(path + ".tmp")
    n = len(keys)
    if bits is None:  # the smallest b with n / 2^b <= 256
        assert n <= 256 << b and (b == 0 or n > 256 << (b - 1))
        assert b == {"ttt": 5, "othello_4x4": 8}[case]
    else:
        assert b == bits
    tb = db.KeyedTablebase(path)
    kb = tb.key_bytes
    assert kb == (int(np.bitwise_or.reduce(keys)).bit_length() + 7) // 8
    if case == "ttt":
        assert kb == 3
    assert (tb.positions, tb.word_bytes, tb.bucket_bits) == (n, wb, b) and len(tb) == n
    assert os.path.getsize(path) == 64 + 8 * ((1 << b) + 1) + n * kb + n * wb
    tb.check_directory()
    counts = np.diff(np.asarray(tb.dir).astype(np.int64))
    if bits == 12:
        assert (counts == 0).sum() > 500 and (counts == 1).sum() > 500  # many empty and one-key buckets
    # the keys section: by bucket, ascending inside a bucket
    stored = tb._key_at(np.arange(n))
    h = db.tk_bucket(stored, b)
    assert (np.diff(h) >= 0).all() and ((np.diff(stored.astype(np.int64)) > 0) | (np.diff(h) > 0)).all()
    # every key reads back its word, in shuffled order
    order = np.random.default_rng(1).permutation(n)
    np.testing.assert_array_equal(tb.lookup_keys(keys[order]), words[order])
    for i in order[:5].tolist():
        assert tb.lookup_key(int(keys[i])) == (int(val[i]), int(rem[i]))
    # absent keys
    have = set(keys.tolist())
    flipped = np.array([k ^ 1 for k in keys.tolist() if k ^ 1 not in have], np.uint64)
    assert len(flipped) > n // 4 and (tb.lookup_keys(flipped) == NO_WORD).all()
    rnd = np.random.default_rng(2).integers(0, 1 << 64, 4096, dtype=np.uint64)
    rnd = rnd[~np.isin(rnd, keys)]
    assert (tb.lookup_keys(rnd) == NO_WORD).all()
    above = keys[:64] | np.uint64(1 << (8 * kb))  # a bit above the stored bytes, the low bytes a stored key's
    assert (tb.lookup_keys(above) == NO_WORD).all() and tb.lookup_key(int(above[0])) is None
    mixed = np.concatenate([keys[:3], above[:2], flipped[:2], keys[-3:]])
    np.testing.assert_array_equal(tb.lookup_keys(mixed),
                                  np.concatenate([words[:3], [NO_WORD] * 4, words[-3:]]).astype(np.uint32))
    assert len(tb.lookup_keys(np.zeros(0, np.uint64))) == 0
    np.testing.assert_array_equal(tb.by_remoteness(), db.census_of(val, rem)["by_remoteness"])


def test_writer_refusals(tmp_path):
    from gamesmanmpi_amd import db
    p = str(tmp_path / "a.gmtk")
    with pytest.raises(ValueError):  # remoteness 64 in one byte
        db.write_keyed_tablebase(p, np.array([3, 9], np.uint64), np.array([1, 64 << 2], np.uint32), 1)
    with pytest.raises(ValueError):  # a key twice
        db.write_keyed_tablebase(p, np.array([3, 3], np.uint64), np.array([1, 1], np.uint32), 1)
    with pytest.raises(ValueError):
        db.write_keyed_tablebase(p, np.array([3, 4], np.uint64), np.array([1], np.uint32), 1)
    assert not os.path.exists(p)
    # an empty table and eight-byte keys
    db.write_keyed_tablebase(p, np.zeros(0, np.uint64), np.zeros(0, np.uint32), 1)
    tb = db.KeyedTablebase(p)
    assert len(tb) == 0 and tb.key_bytes == 1 and tb.lookup_key(5) is None
    big = np.array([1 << 63, 5, (1 << 64) - 2], np.uint64)
    db.write_keyed_tablebase(p, big, np.array([1, 2 | (300 << 2), 0], np.uint32), 2, 3)
    tb = db.KeyedTablebase(p)
    assert tb.key_bytes == 8 and tb.lookup_keys(big).tolist() == [1, 2 | (300 << 2), 0]
    assert tb.lookup_key(6) is None and tb.lookup_key(5) == (2, 300)


def test_damaged_files_are_refused(tmp_path):
    from gamesmanmpi_amd import db
    spec, keys, val, rem, _ = _oracle("ttt")
    path = str(tmp_path / "solution.gmtk")
    db.write_keyed_tablebase(path, keys, _words(val, rem), 1)
    raw = open(path, "rb").read()
    tb = db.KeyedTablebase(path)
    n, kb, nb = tb.positions, tb.key_bytes, 1 << tb.bucket_bits
    del tb
    bad = str(tmp_path / "bad.gmtk")

    def refused(data, lookups=False):
        with open(bad, "wb") as f:
            f.write(data)
        with pytest.raises(ValueError):
            t = db.KeyedTablebase(bad)
            if lookups:  # what opening does not read, a lookup that touches it refuses
                t.lookup_keys(keys)

    refused(b"XMTBKEY1" + raw[8:])                  # a bad magic
    refused(raw[:-1])                               # truncated words
    refused(raw[:-100])
    refused(raw[:len(raw) - n - 7])                 # truncated keys
    refused(raw[:64 + 8 * (nb + 1)])                # no keys at all
    refused(raw[:40])                               # a truncated header
    refused(raw[:64])
    refused(raw[:24] + np.array([n + 1], "<u8").tobytes() + raw[32:])  # positions off by one
    refused(raw[:24] + np.array([n - 1], "<u8").tobytes() + raw[32:])
    last = 64 + 8 * nb
    refused(raw[:last] + np.array([n - 1], "<u8").tobytes() + raw[last + 8:])  # dir[-1] != positions
    mid = 64 + 8 * (nb // 2)
    d = np.frombuffer(raw, "<u8", 2, mid)
    assert d[0] < d[1]
    swapped = raw[:mid] + np.array([d[1], d[0]], "<u8").tobytes() + raw[mid + 16:]  # a non-monotone directory
    refused(swapped, lookups=True)
    with open(bad, "wb") as f:
        f.write(swapped)
    with pytest.raises(ValueError):
        db.KeyedTablebase(bad).check_directory()
    assert kb == 3


def _run(argv):
    from gamesmanmpi_amd.db import main
    out = io.StringIO()
    with redirect_stdout(out):
        rc = main(argv)
    return rc, out.getvalue().splitlines()


def test_db_cli_on_a_converted_directory(tmp_path):
    """The positional queries and --moves print the same lines from the npz
    directory and from its --to-tablebase conversion, which writes .gmtk for a
    game without an index."""
    from gamesmanmpi_amd import db
    spec, keys, val, rem, sol = _oracle("ttt")
    d = tmp_path / "sd" / "stats" / "0"
    os.makedirs(d)
    np.savez_compressed(d / "solution.npz", keys=keys, value=val, remoteness=rem)
    with open(d / "meta.json", "w") as f:
        json.dump({"game": spec.name, "params": spec.params, "root": sol.root_line, "owned_by_rank": 0}, f)
    sd = str(tmp_path / "sd")
    from gamesmanmpi_amd.solver_launcher import ensure_src_utils, load_game
    utils = ensure_src_utils()
    mod = load_game(TTT_GAME)
    second = mod.do_move(mod.initial_position(), 4)
    last = second
    while mod.primitive(last) == utils.UNDECIDED:  # play first moves to a finished game
        last = mod.do_move(last, 0)
    mark = max(max(row) for row in second)
    full = ((mark,) * 3,) * 3  # nine marks of one player
    queries = [[], [str(second), str(last)], ["--moves"], ["--moves", str(second), str(last)], [str(full)],
               ["--census"]]
    before = [_run([sd, "--game", TTT_GAME] + q) for q in queries]
    assert before[0][0] == 0 and before[0][1][0].endswith(": " + sol.root_line)
    assert before[2][0] == 0 and len(before[2][1]) == 10 and sum(x.endswith(" *") for x in before[2][1]) == 1
    assert before[3][0] == 0 and len(before[3][1]) == 1 + 8 + 1
    assert before[4] == (1, ["%s: not reachable" % (full,)])
    rc, lines = _run([sd, "--game", TTT_GAME, "--to-tablebase"])
    assert rc == 0 and lines == [str(d / "solution.gmtk")]
    opened = db.SolutionDB(sd)
    assert isinstance(opened.tablebase, db.KeyedTablebase) and len(opened) == sol.count
    assert opened.meta["format"] == "gmtk" and opened.meta["root"] == sol.root_line
    assert opened.meta["bucket_bits"] == opened.tablebase.bucket_bits == 5
    after = [_run([sd, "--game", TTT_GAME] + q) for q in queries[:5]]
    assert after == before[:5]
    rc, lines = _run([sd, "--game", TTT_GAME, "--census"])  # the remoteness table only
    cut = before[5][1].index("")
    assert rc == 0 and lines == before[5][1][:cut]
    with pytest.raises(SystemExit):  # converting twice
        _run([sd, "--game", TTT_GAME, "--to-tablebase"])


def test_abi_symbols_and_kept_refusals():
    from gamesmanmpi_amd import _lib
    from gamesmanmpi_amd.games import GameSpec
    L = _lib.load()
    for name in ("gm_mix64", "gm_solver_export_keyed"):
        assert name in _lib.EXPORTS and getattr(L, name)
    header = open(os.path.join(ROOT, "include", "gamesman.h")).read()
    assert "int gm_mix64(" in header and "int gm_solver_export_keyed(" in header
    n = ctypes.c_uint64()
    for name, params in (("tic_tac_toe_np", ""), ("mttt", ""), ("othello_bit_new", "length=4,height=4")):
        assert L.gm_tb_info(GameSpec(name, params).id, ctypes.byref(n)) == _lib.GM_EINVAL
    assert L.gm_mix64(None, 1, None) == _lib.GM_EINVAL and L.gm_mix64(None, 0, None) == 0
    out = np.zeros(4, np.uint64)
    assert L.gm_solver_export_keyed(None, 0, 0, 1, None, None, None, None, 0, out.ctypes.data) == _lib.GM_EINVAL
