"""gm_table_check, the host-only header check of a tablebase file before it is
opened on the device (include/gamesman.h, gamesmanmpi_amd.table.check_header):
it accepts what db.write_tablebase / db.write_keyed_tablebase write and
refuses what db.Tablebase / db.KeyedTablebase refuse -- a bad magic, another
version, a file one byte short, a gmtb whose index space is not the game's, a
gmtk with key_bytes 0 or 9.  The files are a few dozen made-up (index, word)
pairs: the checks are structural, nothing is solved and no GPU is touched."""
import os

import numpy as np
import pytest

SUM = ("sum_four_to_one", "heaps=5:4:3")
TTT = ("tic_tac_toe_np", "")


def _spec(game):
    from gamesmanmpi_amd.games import GameSpec
    return GameSpec(*game)


@pytest.fixture()
def gmtb(tmp_path):
    """A gmtb of 40 made-up (index, word) pairs over heaps=5:4:3's index space."""
    from gamesmanmpi_amd import db
    spec = _spec(SUM)
    space = spec.tb_index_space()
    rng = np.random.default_rng(11)
    idx = np.sort(rng.choice(6 * 5 * 4, 40, replace=False)).astype(np.uint64)
    words = rng.integers(0, 4, 40).astype(np.uint32) | (rng.integers(0, 12, 40).astype(np.uint32) << 2)
    path = str(tmp_path / "solution.gmtb")
    db.write_tablebase(path, space, idx, words, 1)
    return spec, path, space


@pytest.fixture()
def gmtk(tmp_path):
    """A gmtk of 48 made-up (key, word) pairs, 3 key bytes, 4 buckets."""
    from gamesmanmpi_amd import db
    rng = np.random.default_rng(12)
    keys = np.unique(rng.integers(0, 1 << 18, 64).astype(np.uint64))[:48]
    keys[-1] |= np.uint64(1 << 17)  # (three key bytes for certain)
    keys = np.unique(keys)
    words = rng.integers(0, 4, len(keys)).astype(np.uint32) | (rng.integers(0, 9, len(keys)).astype(np.uint32) << 2)
    path = str(tmp_path / "solution.gmtk")
    assert db.write_keyed_tablebase(path, keys, words, 1, 2) == 2
    return _spec(TTT), path, len(keys)


def _patched(path, at, data, cut=0):
    """A copy of `path` with `data` written at byte `at` and `cut` bytes dropped from its end."""
    raw = bytearray(open(path, "rb").read())
    raw[at:at + len(data)] = data
    if cut:
        raw = raw[:-cut]
    out = path + ".bad"
    with open(out, "wb") as f:
        f.write(raw)
    return out


def _refused(spec, path, what):
    from gamesmanmpi_amd import _lib
    from gamesmanmpi_amd.table import check_header
    with pytest.raises(_lib.GmError) as e:
        check_header(spec, path)
    assert e.value.code == _lib.GM_EINVAL and what in str(e.value), str(e.value)


def test_untouched_files_are_accepted(gmtb, gmtk):
    from gamesmanmpi_amd import db
    from gamesmanmpi_amd.table import check_header
    spec, path, space = gmtb
    tb = db.Tablebase(path, spec)
    i = check_header(spec, path)
    assert (i["format"], i["positions"], i["word_bytes"], i["index_space"]) == ("gmtb", 40, 1, space)
    assert i["offsets"] == db.tb_header(space, 1, 40)[1:] and i["bytes"] == os.path.getsize(path)
    assert i["index_bytes"] == 0 and i["scratch_bytes"] % 256 == 0 and i["scratch_bytes"] > 0
    assert len(tb) == i["positions"]
    spec, path, n = gmtk
    tk = db.KeyedTablebase(path)
    i = check_header(spec, path)
    assert (i["format"], i["positions"], i["word_bytes"], i["key_bytes"], i["bucket_bits"]) == ("gmtk", n, 1, 3, 2)
    assert i["offsets"] == db.tk_header(1, 3, 2, n)[1:4] and i["bytes"] == db.tk_header(1, 3, 2, n)[4]
    assert (tk.key_bytes, tk.bucket_bits) == (3, 2)


def test_toot_gmtb_reports_its_index_tables(tmp_path):
    """A toot gmtb needs the RANKED index map on the device: first slots per
    height vector (u64), the two level tables, packed heights (u32)."""
    from gamesmanmpi_amd import db
    from gamesmanmpi_amd.table import check_header
    spec = _spec(("toot_and_otto_bitstring", "length=3,height=2"))
    space = spec.tb_index_space()
    key = np.array([spec.root_key], np.uint64)
    path = str(tmp_path / "solution.gmtb")
    db.write_tablebase(path, space, spec.tb_index(key), np.array([2 | (6 << 2)], np.uint32), 1)
    i = check_header(spec, path)
    nhv, levels = 3 ** 3, 3 * 2 + 1
    want = nhv * 8 + 2 * (levels + 1) * 8 + nhv * 4
    assert i["index_bytes"] == (want + 255) // 256 * 256
    state = i["scratch_bytes"] - i["index_bytes"]  # the solver's own state, before the tables
    assert state > 0 and state % 256 == 0


@pytest.mark.parametrize("which", ["gmtb", "gmtk"])
def test_bad_magic_version_and_a_short_file(which, gmtb, gmtk):
    spec, path, _ = gmtb if which == "gmtb" else gmtk
    _refused(spec, _patched(path, 0, b"GMTBOGUS"), "bad magic")
    _refused(spec, _patched(path, 8, np.array([2], "<u4").tobytes()), "version 2")
    _refused(spec, _patched(path, 0, b"", cut=1), "truncated")
    with open(path + ".tiny", "wb") as f:
        f.write(open(path, "rb").read()[:63])
    _refused(spec, path + ".tiny", "header bytes")


def test_gmtb_of_another_index_space(gmtb, tmp_path):
    """A well-formed gmtb of heaps=5:4:3 (index space 512) is no table of
    heaps=9:9:9 (1,024), and a game without an index opens no gmtb at all."""
    from gamesmanmpi_amd import db
    spec, path, space = gmtb
    other = _spec(("sum_four_to_one", "heaps=9:9:9"))
    assert other.tb_index_space() != space
    _refused(other, path, "index space")
    with pytest.raises(ValueError):
        db.Tablebase(path, other)
    _refused(_spec(TTT), path, "no tablebase index")
    # the header's own index space changed, sizes left alone: the offsets no longer fit
    _refused(spec, _patched(path, 16, np.array([space + 512], "<u8").tobytes()), "section offsets")


@pytest.mark.parametrize("kb", [0, 9])
def test_gmtk_key_bytes_out_of_range(kb, gmtk):
    from gamesmanmpi_amd import db
    spec, path, _ = gmtk
    bad = _patched(path, 16, np.array([kb], "<u4").tobytes())
    _refused(spec, bad, "key bytes %d" % kb)
    with pytest.raises(ValueError):
        db.KeyedTablebase(bad)


def test_other_header_fields(gmtb, gmtk):
    spec, path, _ = gmtb
    _refused(spec, _patched(path, 12, np.array([3], "<u4").tobytes()), "word bytes 3")
    _refused(spec, _patched(path, 24, np.array([41], "<u8").tobytes()), "section offsets")  # positions
    spec, path, _ = gmtk
    _refused(spec, _patched(path, 20, np.array([33], "<u4").tobytes()), "bucket bits 33")
    _refused(spec, _patched(path, 40, np.array([1], "<u8").tobytes()), "section offsets")  # keys offset


def test_exports_and_header_name_the_entry_points():
    from conftest import ROOT
    from gamesmanmpi_amd import _lib
    L = _lib.load()
    header = open(os.path.join(ROOT, "include", "gamesman.h")).read()
    for name in ("gm_table_check", "gm_solver_open_table"):
        assert name in _lib.EXPORTS and getattr(L, name) and name in header
    assert "#define GM_MODE_FILE 5u" in header and _lib.GM_MODE_FILE == 5
