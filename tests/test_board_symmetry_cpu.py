"""Board symmetry on the host (params "board_symmetry=1", csrc/gm_sym.h):
the key maps of gm_symmetry against a numpy restatement that permutes the
cells of the golden tables' unpacked canonical bytes (it never calls
gm_symmetry), the orbit counts, the symmetric descriptor's children, the
refusals, and SolutionDB over a keyed tablebase of representatives."""
import json
import os

import numpy as np
import pytest

from conftest import CASES, load_table

# golden table -> orbits of its reachable positions under the board maps
# that fix the start position
ORBITS = {
    "tic_tac_toe_np": 765,
    "mttt": 765,
    "toot_3x3": 5869,
    "toot_4x3": 100253,
    "toot_3x4": 64964,
    "othello_4x4": 13633,
}


def sym_case(name):
    stem, params = CASES[name]
    return stem, (params + ",board_symmetry=1").lstrip(",")


# -- the yardstick: cell permutations of the canonical bytes ------------------
def _ttt_maps():
    R = lambda a: a[:, ::-1, :]          # x -> 2 - x (cell 3x + y)
    C = lambda a: a[:, :, ::-1]          # y -> 2 - y
    T = lambda a: a.transpose(0, 2, 1)
    # the order include/gamesman.h documents: R C RC T RT CT RCT
    return [R, C, lambda a: R(C(a)), T, lambda a: R(T(a)), lambda a: C(T(a)),
            lambda a: R(C(T(a)))]


def _plane_maps(kind):
    if kind == "toot":
        return [lambda p: p[..., ::-1]]  # x -> L - 1 - x
    turn = lambda p: p[..., ::-1, ::-1]
    tr = lambda p: p.swapaxes(-1, -2)
    return [turn, tr, lambda p: turn(tr(p))]  # 180-degree turn, transpose, anti-transpose


def numpy_images(name, canon):
    """[canonical bytes of map i of every row] for golden table `name`."""
    stem, params = CASES[name]
    if stem in ("tic_tac_toe_np", "mttt"):
        a = canon.reshape(-1, 3, 3)
        return [np.ascontiguousarray(f(a)).reshape(-1, 9) for f in _ttt_maps()]
    kv = dict(p.split("=") for p in params.split(","))
    L, H = int(kv["length"]), int(kv["height"])
    A = L * H
    bits = np.unpackbits(canon, axis=1)  # MSB first: bit i is cell i, plane 1 at A + i
    out = []
    for f in _plane_maps("toot" if stem.startswith("toot") else "othello"):
        b = bits.copy()
        planes = bits[:, :2 * A].reshape(-1, 2, H, L)  # cell L*y + x
        b[:, :2 * A] = np.ascontiguousarray(f(planes)).reshape(-1, 2 * A)
        out.append(np.packbits(b, axis=1))
    return out


_cache = {}


def golden(name):
    """(plain spec, symmetric spec, table, golden keys, [numpy image keys])
    of a golden table, computed once."""
    if name not in _cache:
        from gamesmanmpi_amd.games import GameSpec
        plain, sym = GameSpec(*CASES[name]), GameSpec(*sym_case(name))
        t = load_table(name)
        keys = plain.encode_batch(t["canon"], t["clen"])
        imgs = [plain.encode_batch(c, t["clen"]) for c in numpy_images(name, t["canon"])]
        _cache[name] = (plain, sym, t, keys, imgs)
    return _cache[name]


def numpy_canon(name):
    """Orbit minima of the golden keys by the numpy maps."""
    _, _, _, gk, imgs = golden(name)
    return np.minimum.reduce([gk] + imgs)


# -- the maps -----------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(ORBITS))
def test_maps_match_numpy_and_keep_the_table(name):
    plain, sym, t, keys, imgs = golden(name)
    assert sym.board_symmetric and sym.symmetric and not plain.symmetric
    maps = {"tic_tac_toe_np": 7, "mttt": 7, "toot_and_otto_bitstring": 1, "othello_bit_new": 3}[plain.name]
    assert sym.symmetry_count() == len(imgs) == maps and plain.symmetry_count() == 0
    order = np.argsort(keys)
    skeys = keys[order]
    got = [sym.symmetry(keys, i) for i in range(len(imgs))]
    for i, (g, want) in enumerate(zip(got, imgs)):
        np.testing.assert_array_equal(g, want, err_msg="map %d" % i)
        np.testing.assert_array_equal(np.sort(g), skeys)  # a bijection of the reachable set
        at = order[np.searchsorted(skeys, g)]
        for col in ("value", "remoteness", "level", "nchild"):
            np.testing.assert_array_equal(t[col][at], t[col], err_msg="map %d, %s" % (i, col))
    # composing two maps gives the identity or a map of the group
    group = [keys] + got
    for i in range(len(got)):
        for j in range(len(got)):
            c = sym.symmetry(got[i], j)
            assert any((c == g).all() for g in group), (i, j)
    with pytest.raises(Exception):
        sym.symmetry(keys[:1], len(imgs))


@pytest.mark.parametrize("name", sorted(ORBITS))
def test_representatives_are_orbit_minima(name):
    plain, sym, t, keys, imgs = golden(name)
    rep = sym.symmetry(keys)
    np.testing.assert_array_equal(rep, numpy_canon(name))
    np.testing.assert_array_equal(sym.symmetry(rep), rep)  # idempotent
    assert len(np.unique(rep)) == ORBITS[name]
    assert sym.root_key == plain.root_key == int(sym.symmetry(np.array([plain.root_key], np.uint64))[0])
    np.testing.assert_array_equal(plain.symmetry(keys), keys)  # no parameter: identity


@pytest.mark.parametrize("name", sorted(ORBITS))
def test_symmetric_children_are_the_canonical_children(name):
    plain, sym, t, keys, _ = golden(name)
    canon = numpy_canon(name)  # the yardstick's representative of every golden key
    order = np.argsort(keys)
    skeys = keys[order]
    reps = np.unique(canon)
    pr, nc, ch = plain.host_expand(reps)
    spr, snc, sch = sym.host_expand(reps)
    np.testing.assert_array_equal(spr, pr)  # the primitive value is unchanged
    np.testing.assert_array_equal(snc, nc)  # duplicates stay: edges count occurrences
    n = ch.shape[1]
    live = np.arange(n)[None, :] < nc[:, None]
    # children of reachable positions are golden keys: their numpy representatives
    at = np.searchsorted(skeys, ch[live])
    np.testing.assert_array_equal(skeys[at], ch[live])
    none = np.uint64(0xFFFFFFFFFFFFFFFF)
    want = np.full(ch.shape, none)
    want[live] = canon[order[at]]
    got = np.where(live, sch, none)
    np.testing.assert_array_equal(np.sort(got, axis=1), np.sort(want, axis=1))
    assert (sch[live] != ch[live]).any()  # some child is not its own representative


def test_empty_board_emits_nine_children_of_three_orbits():
    _, sym, _, _, _ = golden("tic_tac_toe_np")
    _, nc, ch = sym.host_expand(np.array([sym.root_key], np.uint64))
    assert nc[0] == 9 and len(set(ch[0, :9].tolist())) == 3


def test_verify_replays_reference_modules_canonically():
    """GameSpec.verify on the recorded reference modules: the symmetric
    descriptor's children are the canonical images of the module's."""
    from test_launcher import _recorded
    from gamesmanmpi_amd.games import GameSpec
    for fname, kw, name in (("tic_tac_toe_np.py", {}, "tic_tac_toe_np"),
                            ("toot_and_otto_bitstring.py", dict(length=4, height=3), "toot_4x3"),
                            ("othello_bit_new.py", dict(length=4, height=4), "othello_4x4")):
        spec = GameSpec(*sym_case(name))
        assert spec.symmetry_count() > 0
        assert spec.verify(_recorded(fname, **kw), samples=100) == 100


def test_othello_sizes_other_than_four():
    """L = 2 runs the per-cell transpose: the three maps against numpy on
    every bit pattern of the key (turn bit and pass count included).  L = 3 and 5: the
    module's off-centre start is moved by the transpose, so the descriptor
    refuses them."""
    from gamesmanmpi_amd import _lib
    from gamesmanmpi_amd.games import GameSpec
    L = 2
    A = L * L
    sym = GameSpec("othello_bit_new", "length=2,height=2,board_symmetry=1")
    assert sym.symmetry_count() == 3
    keys = np.arange(1 << (2 * A + 3), dtype=np.uint64)  # every bit pattern of the key
    cells = ((keys[:, None] >> np.arange(2 * A, dtype=np.uint64)[None, :]) & np.uint64(1)).reshape(-1, 2, L, L)
    hi = keys & ~np.uint64((1 << (2 * A)) - 1)
    imgs = []
    for i, f in enumerate(_plane_maps("othello")):
        img = np.ascontiguousarray(f(cells)).reshape(-1, 2 * A)
        want = hi | (img << np.arange(2 * A, dtype=np.uint64)[None, :]).sum(axis=1, dtype=np.uint64)
        np.testing.assert_array_equal(sym.symmetry(keys, i), want, err_msg="map %d" % i)
        imgs.append(want)
    np.testing.assert_array_equal(sym.symmetry(keys), np.minimum.reduce([keys] + imgs))
    for n in (3, 5):
        with pytest.raises(_lib.GmError) as e:
            GameSpec("othello_bit_new", "length=%d,height=%d,board_symmetry=1" % (n, n))
        assert e.value.code == _lib.GM_EINVAL and "start position" in str(e.value)


# -- refusals -------------------------------------------------------------------
def test_refusals():
    from gamesmanmpi_amd import _lib
    from gamesmanmpi_amd.games import GameSpec
    for name, params in (("four_to_one", "start=4,board_symmetry=1"),
                         ("sum_four_to_one", "heaps=3:3,board_symmetry=1"),
                         ("othello_bit_new", "length=4,height=4,symmetry=1,board_symmetry=1"),
                         ("othello_bit_new", "length=4,height=4,board_symmetry=1,symmetry=1"),
                         ("tic_tac_toe_np", "symmetry=1")):  # still no symmetry_functions()
        with pytest.raises(_lib.GmError) as e:
            GameSpec(name, params)
        assert e.value.code == _lib.GM_EINVAL and str(e.value), (name, params)


def test_toot_plans_bucketed_and_refuses_ranked():
    from gamesmanmpi_amd import _lib
    from gamesmanmpi_amd.games import GameSpec
    L = _lib.load()
    plain, sym = GameSpec(*CASES["toot_4x3"]), GameSpec(*sym_case("toot_4x3"))
    plan = _lib.gm_plan_t()
    _lib.check(L.gm_plan(plain.id, 0, 0, 0, _lib.ctypes.byref(plan)))
    assert plan.mode == _lib.GM_MODE_RANKED
    _lib.check(L.gm_plan(sym.id, 0, 0, 0, _lib.ctypes.byref(plan)))
    assert plan.mode == _lib.GM_MODE_BUCKETED
    _lib.check(L.gm_plan(sym.id, 0, _lib.GM_F_HASH_TABLE, 0, _lib.ctypes.byref(plan)))
    assert plan.mode == _lib.GM_MODE_HASHED
    rc = L.gm_plan_keyed_shard(sym.id, 0, 2, 0, _lib.GM_F_RANKED_SHARD, 0, _lib.ctypes.byref(plan))
    assert rc == _lib.GM_EINVAL and b"ranked" in L.gm_last_error().lower()
    with pytest.raises(_lib.GmError):  # no RANKED index, so no indexed tablebase either
        sym.tb_index_space()


def test_launcher_refuses_a_game_without_a_board_group():
    from conftest import ROOT
    from gamesmanmpi_amd import solver_launcher as sl
    game = os.path.join(ROOT, "gamesmanmpi_amd", "games", "sum_four_to_one.py")
    with pytest.raises(SystemExit) as e:
        sl.main([game, "--board-symmetry", "--no-verify"])
    assert "no board group" in str(e.value)
    # a game file without a descriptor, and the graph path: refused, not ignored
    grid = os.path.join(ROOT, "tests", "games", "grid_tictactoe.py")
    ttt = os.path.join(ROOT, "tests", "games", "descriptor_ttt", "tic_tac_toe_np.py")
    for argv in ([grid, "--board-symmetry"], [ttt, "--board-symmetry", "--layout", "graph", "--no-verify"]):
        with pytest.raises(SystemExit) as e:
            sl.main(argv)
        assert "--board-symmetry" in str(e.value), argv


# -- SolutionDB over a keyed tablebase of representatives -------------------------
def test_solution_db_maps_every_key_to_its_representative(tmp_path):
    from gamesmanmpi_amd import db
    plain, sym, t, keys, _ = golden("tic_tac_toe_np")
    rep = sym.symmetry(keys)
    ukeys, first = np.unique(rep, return_index=True)
    assert len(ukeys) == 765
    # the golden rows OF the representatives themselves
    at = np.argsort(keys)[np.searchsorted(np.sort(keys), ukeys)]
    words = t["value"][at].astype(np.uint32) | (t["remoteness"][at].astype(np.uint32) << 2)
    d = tmp_path / "stats" / "0"
    d.mkdir(parents=True)
    bits = db.write_keyed_tablebase(str(d / db.TK_NAME), ukeys, words, 1)
    (d / "meta.json").write_text(json.dumps({"game": sym.name, "params": sym.params, "format": "gmtk",
                                             "bucket_bits": bits, "positions": len(ukeys), "word_bytes": 1}))
    sdb = db.SolutionDB(str(tmp_path))
    assert len(sdb) == 765
    canon, clen = t["canon"], t["clen"]
    for i in range(len(keys)):
        pos = plain.from_canon(canon[i, :clen[i]].tobytes())
        assert sdb.lookup(pos, plain) == (int(t["value"][i]), int(t["remoteness"][i])), i
    # the reader itself, in one batch
    w = sdb.tablebase.lookup_keys(keys)
    np.testing.assert_array_equal(w & 3, t["value"])
    np.testing.assert_array_equal(w >> 2, t["remoteness"])
    # a table without the parameter does not map: a non-representative is absent
    (d / "meta.json").write_text(json.dumps({"game": plain.name, "params": plain.params, "format": "gmtk"}))
    off = np.flatnonzero(rep != keys)[0]
    pos = plain.from_canon(canon[off, :clen[off]].tobytes())
    assert db.SolutionDB(str(tmp_path)).lookup(pos, plain) is None


def test_to_tablebase_of_a_symmetric_toot_table_stays_keyed(tmp_path):
    """A saved symmetric toot solve converted with the PLAIN game's spec (what
    `db DIR --game toot.py --to-tablebase` passes): the plain game has an
    index, the table of representatives has none, so the output is the keyed
    tablebase with the table's own params, and every golden key looks up."""
    from gamesmanmpi_amd import db
    name = "toot_3x3"
    plain, sym, t, keys, _ = golden(name)
    assert plain.tb_index_space() > 0
    canon = numpy_canon(name)
    reps = np.unique(canon)
    at = np.argsort(keys)[np.searchsorted(np.sort(keys), reps)]
    d = tmp_path / "stats" / "0"
    d.mkdir(parents=True)
    np.savez_compressed(str(d / "solution.npz"), keys=reps, value=t["value"][at], remoteness=t["remoteness"][at])
    (d / "meta.json").write_text(json.dumps({"game": sym.name, "params": sym.params, "positions": len(reps)}))
    path = db.convert_to_tablebase(str(tmp_path), plain)
    assert os.path.basename(path) == db.TK_NAME and not os.path.exists(str(d / db.TB_NAME))
    sdb = db.SolutionDB(str(tmp_path))
    assert isinstance(sdb.tablebase, db.KeyedTablebase) and len(sdb) == ORBITS[name]
    assert sdb.meta["params"] == sym.params and sdb.meta["format"] == "gmtk"
    for i in range(len(keys)):
        pos = plain.from_canon(t["canon"][i, :t["clen"][i]].tobytes())
        assert sdb.lookup(pos, plain) == (int(t["value"][i]), int(t["remoteness"][i])), i


def test_plain_keyed_tablebase_opens_without_a_spec(tmp_path):
    """A plain .gmtk needs no descriptor to open: an unregistered game name in its meta is fine."""
    from gamesmanmpi_amd import db
    d = tmp_path / "stats" / "0"
    d.mkdir(parents=True)
    db.write_keyed_tablebase(str(d / db.TK_NAME), np.array([3, 9], np.uint64), np.array([1, 6], np.uint32), 1)
    (d / "meta.json").write_text(json.dumps({"game": "no_such_game", "params": "", "format": "gmtk"}))
    sdb = db.SolutionDB(str(tmp_path))
    assert sdb.tablebase.spec is None and sdb.lookup_key(9) == (2, 1)
