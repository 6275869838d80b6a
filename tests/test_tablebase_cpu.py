"""The indexed tablebase on the host: the index functions of the C-ABI
(gm_tb_info / gm_tb_index) against the oracle's reachable positions and a
Python restatement of the slot map, the file format through the pure-numpy
writer and the mmap reader (gamesmanmpi_amd/db.py), and the db command line
on a tablebase directory.  No GPU."""
import io
import json
import os
from contextlib import redirect_stdout

import numpy as np
import pytest

from conftest import ROOT

OWN_SUM = os.path.join(ROOT, "gamesmanmpi_amd", "games", "sum_four_to_one.py")
TOOT, SUM, FTO = "toot_and_otto_bitstring", "sum_four_to_one", "four_to_one"
NO_INDEX = 0xFFFFFFFFFFFFFFFF
NO_WORD = 0xFFFFFFFF
HAND = 6


def _oracle(name, params):
    """(spec, keys u64, value, remoteness, solution) of the oracle's solve."""
    from gamesmanmpi_amd.games import GameSpec
    from oracle.oracle import Game  # checker only
    spec = GameSpec(name, params)
    sol = Game(name, params).solve(1 << 22)
    canon, clen, val, rem = sol.dump(stride=24)
    return spec, spec.encode_batch(canon, clen), val, rem, sol


# -- gm_tb_index --------------------------------------------------------------
@pytest.mark.parametrize("name,params,total", [(SUM, "heaps=2:5:7", 3 * 6 * 8), (FTO, "start=20", 21)])
def test_sum_index_is_the_key(name, params, total):
    spec, keys, _, _, sol = _oracle(name, params)
    assert sol.count == total and sorted(keys.tolist()) == list(range(total))
    assert spec.tb_index_space() == (total + 511) // 512 * 512
    assert (spec.tb_index(keys) == keys).all()
    # a digit past its heap: only the top digit can be, and it lifts the key past the product
    past = np.array([total, total + 1, 511, 512, 1 << 40, NO_INDEX], np.uint64)
    assert (spec.tb_index(past) == np.uint64(NO_INDEX)).all()


def _shape(C, H):
    """rank_shape restated: per level the height vectors in code order, blocks
    of 8 x 2^L slots, levels padded to 512."""
    R = H + 1
    byl = {}
    for code in range(R ** C):
        hv = [(code // R ** x) % R for x in range(C)]
        byl.setdefault(sum(hv), []).append(code)
    base, at = {}, 0
    for L in range(C * H + 1):
        for j, code in enumerate(byl.get(L, [])):
            base[code] = at + j * (8 << L)
        at += (len(byl.get(L, [])) * (8 << L) + 511) // 512 * 512
    return base, at


def _slot(key, C, H, base):
    """rk_slot_of restated: key -> slot or None."""
    A = C * H
    full = (1 << A) - 1
    t, o = key & full, (key >> A) & full
    if t & o or key >> (2 * A + 13):
        return None
    occ = t | o
    code = pat = L = 0
    for x in range(C):
        h = 0
        while h < H and (occ >> (C * h + x)) & 1:
            h += 1
        if any((occ >> (C * y + x)) & 1 for y in range(h, H)):
            return None  # a floating piece
        for y in range(h):
            pat |= ((t >> (C * y + x)) & 1) << (L + y)
        code += h * (H + 1) ** x
        L += h
    nT = bin(pat).count("1")
    sT, sO = (key >> (2 * A)) & 7, (key >> (2 * A + 3)) & 7
    fT, fO = (key >> (2 * A + 6)) & 7, (key >> (2 * A + 9)) & 7
    turn = (key >> (2 * A + 12)) & 1
    a = HAND - fT
    used = (a, (L + 1) // 2 - a, nT - a, L // 2 - (nT - a))
    if not all(0 <= u <= HAND for u in used):
        return None
    if (HAND - used[1], HAND - used[2], HAND - used[3]) != (fO, sT, sO) or turn != (L & 1):
        return None
    return base[code] + (a << L) + pat


@pytest.mark.parametrize("C,H", [(3, 3), (4, 3), (2, 4)])
def test_toot_index_is_the_ranked_slot(C, H):
    spec, keys, _, _, sol = _oracle(TOOT, "length=%d,height=%d" % (C, H))
    base, nslots = _shape(C, H)
    space = spec.tb_index_space()
    assert space == nslots and space % 512 == 0
    idx = spec.tb_index(keys)
    assert (idx < np.uint64(space)).all()
    assert len(np.unique(idx)) == sol.count == len(keys)
    assert idx.tolist() == [_slot(k, C, H, base) for k in keys.tolist()]
    root = spec.encode(sol.game.root())
    assert root == spec.root_key and int(spec.tb_index(np.array([root], np.uint64))[0]) == 0
    # keys that are no position: a floating piece, bad hands, a wrong turn bit
    A = C * H
    k1 = next(k for k in keys.tolist() if bin(k & ((1 << 2 * A) - 1)).count("1") == 1)  # one piece on the board
    cell = (k1 | (k1 >> A)) & ((1 << A) - 1)
    piece_t = bool(k1 & cell)
    floating = (k1 & ~(cell | (cell << A))) | ((cell << C) << (0 if piece_t else A))  # lifted one row
    bad = [floating,
           k1 ^ (1 << (2 * A + 12)),          # the turn bit of the other player
           k1 ^ (1 << (2 * A)),               # a hand count off by one
           k1 | (7 << (2 * A + 6)),           # a hand of 7
           root | (1 << (2 * A + 13)),        # a bit above the key
           root | 1 | (1 << A)]               # T and O on one cell
    for k in bad:
        assert _slot(k, C, H, base) is None, hex(k)
    assert (spec.tb_index(np.array(bad, np.uint64)) == np.uint64(NO_INDEX)).all()


@pytest.mark.parametrize("name,params", [("tic_tac_toe_np", ""), ("mttt", ""),
                                         ("othello_bit_new", "length=4,height=4")])
def test_games_without_an_index(name, params):
    import ctypes
    from gamesmanmpi_amd import _lib
    from gamesmanmpi_amd.games import GameSpec
    spec = GameSpec(name, params)
    n = ctypes.c_uint64()
    assert _lib.load().gm_tb_info(spec.id, ctypes.byref(n)) == _lib.GM_EINVAL
    out = np.zeros(1, np.uint64)
    key = np.array([spec.root_key], np.uint64)
    assert _lib.load().gm_tb_index(spec.id, key.ctypes.data, 1, out.ctypes.data) == _lib.GM_EINVAL


# -- the file: write_tablebase -> Tablebase -------------------------------------
def _write(tmp_path, spec, keys, val, rem, name="solution.gmtb"):
    from gamesmanmpi_amd import db
    words = val.astype(np.uint32) | (rem.astype(np.uint32) << 2)
    wb = db.tb_word_bytes(int(rem.max()))
    path = str(tmp_path / name)
    db.write_tablebase(path, spec.tb_index_space(), spec.tb_index(keys), words, wb)
    assert not os.path.exists(path + ".tmp")
    return path, words, wb


@pytest.mark.parametrize("name,params", [(TOOT, "length=4,height=3"), (SUM, "heaps=6:6:6:6"), (SUM, "heaps=2:5:7")])
def test_round_trip(tmp_path, name, params):
    from gamesmanmpi_amd import db
    spec, keys, val, rem, sol = _oracle(name, params)
    path, words, wb = _write(tmp_path, spec, keys, val, rem)
    space = spec.tb_index_space()
    if params == "heaps=2:5:7":
        assert sol.count == 144 and space == 512  # an index space that is no multiple of 512 before padding
    tb = db.Tablebase(path, spec)
    assert (tb.index_space, tb.positions, tb.word_bytes) == (space, sol.count, wb) and len(tb) == sol.count
    assert os.path.getsize(path) == 64 + space // 8 + 8 * (space // 512 + 1) + sol.count * wb
    # every position reads back its golden (value, remoteness), in any order
    order = np.random.default_rng(1).permutation(len(keys))
    got = tb.lookup_keys(keys[order])
    assert (got == words[order]).all()
    for i in order[:5].tolist():
        assert tb.lookup_key(int(keys[i])) == (int(val[i]), int(rem[i]))
    # every other index of the space is unreached
    allw = tb.lookup_indexes(np.arange(space, dtype=np.uint64))
    idx = spec.tb_index(keys).astype(np.int64)
    mask = np.zeros(space, bool)
    mask[idx] = True
    assert (allw[mask] != NO_WORD).all() and (allw[~mask] == NO_WORD).all()
    assert (allw[idx] == words).all()
    # no index, and indexes outside the space
    assert (tb.lookup_indexes(np.array([NO_INDEX, space, space + 5], np.uint64)) == NO_WORD).all()
    # the remoteness table of the words section
    assert (tb.by_remoteness() == db.census_of(val, rem)["by_remoteness"]).all()


def test_word_bytes_and_refusals(tmp_path):
    from gamesmanmpi_amd import db
    assert [db.tb_word_bytes(r) for r in (0, 63, 64, 16383, 16384)] == [1, 1, 2, 2, 4]
    idx = np.array([3, 700], np.uint64)
    with pytest.raises(ValueError):  # remoteness 64 in one byte
        db.write_tablebase(str(tmp_path / "a.gmtb"), 1024, idx, np.array([1, 64 << 2], np.uint32), 1)
    with pytest.raises(ValueError):  # outside the space
        db.write_tablebase(str(tmp_path / "a.gmtb"), 512, idx, np.array([1, 1], np.uint32), 1)
    with pytest.raises(ValueError):  # twice
        db.write_tablebase(str(tmp_path / "a.gmtb"), 1024, np.array([3, 3], np.uint64), np.array([1, 1], np.uint32), 1)
    assert not os.path.exists(str(tmp_path / "a.gmtb"))
    # 2-byte words
    p = str(tmp_path / "b.gmtb")
    db.write_tablebase(p, 1024, idx, np.array([1 | (200 << 2), 0 | (16383 << 2)], np.uint32), 2)
    tb = db.Tablebase(p)
    assert tb.lookup_indexes(np.array([700, 3, 4], np.uint64)).tolist() == [16383 << 2, 1 | (200 << 2), NO_WORD]


def test_damaged_files_are_refused(tmp_path):
    from gamesmanmpi_amd import db
    spec, keys, val, rem, _ = _oracle(SUM, "heaps=2:5:7")
    path, _, _ = _write(tmp_path, spec, keys, val, rem)
    raw = open(path, "rb").read()
    bad = str(tmp_path / "bad.gmtb")
    with open(bad, "wb") as f:  # a bad magic
        f.write(b"XMTBASE1" + raw[8:])
    with pytest.raises(ValueError):
        db.Tablebase(bad, spec)
    for cut in (1, 100, len(raw) - 64):  # a truncated words section, down to none; then a truncated header
        with open(bad, "wb") as f:
            f.write(raw[:len(raw) - cut])
        with pytest.raises(ValueError):
            db.Tablebase(bad, spec)
    with open(bad, "wb") as f:
        f.write(raw[:40])
    with pytest.raises(ValueError):
        db.Tablebase(bad, spec)
    with open(bad, "wb") as f:  # a positions count larger than the words that follow
        f.write(raw[:24] + np.array([145], "<u8").tobytes() + raw[32:])
    with pytest.raises(ValueError):
        db.Tablebase(bad, spec)
    with open(bad, "wb") as f:  # another game's index space
        f.write(raw)
    from gamesmanmpi_amd.games import GameSpec
    with pytest.raises(ValueError):
        db.Tablebase(bad, GameSpec(SUM, "heaps=31:31"))


# -- the command line ---------------------------------------------------------------
def _run(argv):
    from gamesmanmpi_amd.db import main
    out = io.StringIO()
    with redirect_stdout(out):
        rc = main(argv)
    return rc, out.getvalue().splitlines()


def test_db_cli_on_a_tablebase(tmp_path):
    """The positional query, --moves and --census print the same lines from the
    npz directory and from its --to-tablebase conversion."""
    from gamesmanmpi_amd import db
    game = tmp_path / "sum_four_to_one.py"
    game.write_text(open(OWN_SUM).read().replace(
        "HEAPS = (31, 31, 31, 31, 31, 31)", "HEAPS = (4, 6, 3)"))
    spec, keys, val, rem, sol = _oracle(SUM, "heaps=4:6:3")
    d = tmp_path / "sd" / "stats" / "0"
    os.makedirs(d)
    np.savez_compressed(d / "solution.npz", keys=keys, value=val, remoteness=rem)
    with open(d / "meta.json", "w") as f:
        json.dump({"game": spec.name, "params": spec.params, "root": sol.root_line, "owned_by_rank": 0}, f)
    sd = str(tmp_path / "sd")
    queries = [[], ["139", "57", "0"], ["--moves", "139", "36", "1", "0"], ["--moves", "140"], ["--census"]]
    before = [_run([sd, "--game", str(game)] + q) for q in queries]
    assert before[0] == (0, ["139: " + sol.root_line]) and before[3] == (1, ["140: not reachable"])
    rc, lines = _run([sd, "--game", str(game), "--to-tablebase"])
    assert rc == 0 and lines == [str(d / "solution.gmtb")]
    opened = db.SolutionDB(sd)
    assert opened.tablebase is not None and len(opened) == sol.count
    assert opened.meta["format"] == "gmtb" and opened.meta["root"] == sol.root_line
    after = [_run([sd, "--game", str(game)] + q) for q in queries[:4]]
    assert after == before[:4]
    # --census on a tablebase: the remoteness table only
    rc, lines = _run([sd, "--game", str(game), "--census"])
    cut = before[4][1].index("")
    assert rc == 0 and lines == before[4][1][:cut]
    with pytest.raises(SystemExit):  # converting twice
        _run([sd, "--game", str(game), "--to-tablebase"])


def test_abi_symbols_exported():
    from gamesmanmpi_amd import _lib
    L = _lib.load()
    for name in ("gm_tb_info", "gm_tb_index", "gm_solver_export"):
        assert name in _lib.EXPORTS and getattr(L, name)
    assert (_lib.GM_NO_INDEX, _lib.GM_TB_BLOCK, _lib.GM_EXPORT_GENERIC) == (NO_INDEX, 512, 1)
