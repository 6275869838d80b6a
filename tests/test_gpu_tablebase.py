"""The device export of the indexed tablebase (gm_solver_export,
Solver.export_range / export_tablebase) on every layout that serves an indexed
game: the whole index space in one call against the same space in chunks of
1,024 indexes, the counts against the solve's, the written file read back
through db.Tablebase against Solver.dump(), and the direct PLANES / RANKED
kernels against the generic path, byte for byte.

Chunks: an index space of fewer than three 1,024-index chunks (heaps=31:31
holds 1,024 indexes, four_to_one start=20 one block of 512) is cut into
512-index blocks instead -- it has no three chunks to give."""
import ctypes
import io
import os
from contextlib import redirect_stdout

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

PLANE_LEVELS = 65536  # GM_F_PLANE_LEVELS
SUM, TOOT, FTO = "sum_four_to_one", "toot_and_otto_bitstring", "four_to_one"
NO_WORD = 0xFFFFFFFF

# id -> (game, params, layout, flags)
PLANES = {
    "planes_31_31": (SUM, "heaps=31:31", "planes", 0),                      # no outer digit, 1-byte words
    "planes_31_31_2_5": (SUM, "heaps=31:31:2:5", "planes", 0),              # mixed bases
    "planes_31_31_4_0_2": (SUM, "heaps=31:31:4:0:2", "planes", 0),          # a zero-height heap
    "planes_31_31_200_rel": (SUM, "heaps=31:31:200", "planes", 0),          # 8-bit relative forms, 2-byte words
    "planes_31_31_444_w16": (SUM, "heaps=31:31:444", "planes", 0),          # 16-bit forms
    "planes_31_31_15_15": (SUM, "heaps=31:31:15:15", "planes", 0),          # the one-launch writer
    "planes_31_31_15_15_levels": (SUM, "heaps=31:31:15:15", "planes", PLANE_LEVELS),  # the per-level writer
}
RANKED = {
    "toot_3x3_ranked": (TOOT, "length=3,height=3", "ranked", 0),
    "toot_3x4_ranked": (TOOT, "length=3,height=4", "ranked", 0),
    "toot_4x3_ranked": (TOOT, "length=4,height=3", "ranked", 0),
    "toot_4x4_ranked": (TOOT, "length=4,height=4", "ranked", 0),  # ~1 slot in 6 reached: the compaction matters
}
GENERIC = {
    "sum_6_6_6_6_dense": (SUM, "heaps=6:6:6:6", "dense", 0),
    "sum_6_6_6_6_hashed": (SUM, "heaps=6:6:6:6", "hashed", 0),
    "four_to_one_20_dense": (FTO, "start=20", "dense", 0),
    "four_to_one_20_hashed": (FTO, "start=20", "hashed", 0),
    "toot_3x4_bucketed": (TOOT, "length=3,height=4", "bucketed", 0),
}
CASES = {**PLANES, **RANKED, **GENERIC}
DIRECT = {**PLANES, **RANKED}

_solved = {}


def solved(case):
    """One solve per case for the whole module, with the dump, the word width
    the exporter picks and the whole index space exported in one call."""
    if case not in _solved:
        from gamesmanmpi_amd import db
        from gamesmanmpi_amd.games import GameSpec
        from gamesmanmpi_amd.solver import Solver
        game, params, layout, flags = CASES[case]
        spec = GameSpec(game, params)
        s = Solver(spec, layout=layout, flags=flags)
        r = s.solve()
        assert r.extra["layout"] == layout
        keys, val, rem = s.dump()
        wb = db.tb_word_bytes(int(rem.max()))
        space = spec.tb_index_space()
        _solved[case] = dict(spec=spec, s=s, r=r, keys=keys, words=val.astype(np.uint32) | (rem << 2), wb=wb,
                             space=space, whole=_host(s.export_range(0, space, wb)))
    return _solved[case]


def _host(t):
    bits, counts, words = t
    return (bits.cpu().numpy().view(np.uint64), counts.cpu().numpy().view(np.uint32), words.cpu().numpy())


def _same(a, b):
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and x.shape == y.shape
        np.testing.assert_array_equal(x, y)


@pytest.mark.parametrize("case", sorted(CASES))
def test_chunks_concatenate_to_the_whole(case):
    """1. one call over the whole space == chunks of 1,024 indexes, byte for
    byte; 2. the set bits == the solve's positions == the block counts' sum."""
    import torch
    from gamesmanmpi_amd import _lib
    c = solved(case)
    s, space, wb = c["s"], c["space"], c["wb"]
    bits, counts, words = c["whole"]
    assert bits.shape == (space // 64,) and counts.shape == (space // 512,)
    npos = int(c["r"].positions)
    assert sum(bin(int(x)).count("1") for x in bits.tolist()) == npos == int(counts.sum(dtype=np.uint64))
    assert len(words) == npos * wb and npos == len(c["keys"])
    per_block = np.array([sum(bin(int(x)).count("1") for x in bits[8 * b:8 * b + 8].tolist())
                          for b in range(0, space // 512, max(1, space // 512 // 64))])
    np.testing.assert_array_equal(per_block, counts[::max(1, space // 512 // 64)])
    chunk = 1024 if space >= 3 * 1024 - 512 else 512
    firsts = list(range(0, space, chunk))
    assert len(firsts) >= (3 if space >= 1536 else space // 512)
    dev = s.device
    gb = torch.zeros(space // 64, dtype=torch.int64, device=dev)
    gc = torch.zeros(space // 512, dtype=torch.int32, device=dev)
    gw = torch.zeros(max(1, npos * wb), dtype=torch.uint8, device=dev)
    tmp = torch.zeros(chunk * wb, dtype=torch.uint8, device=dev)
    L, n, at = _lib.load(), ctypes.c_uint64(), 0
    with torch.cuda.device(dev):
        for first in firsts:
            count = min(chunk, space - first)  # (the tail, where the space is no multiple of the chunk)
            _lib.check(L.gm_solver_export(s.handle, 0, first, count, wb, gb[first // 64:].data_ptr(),
                                          gc[first // 512:].data_ptr(), tmp.data_ptr(), chunk, ctypes.byref(n)))
            gw[at * wb:(at + n.value) * wb] = tmp[:n.value * wb]
            at += n.value
    assert at == npos
    _same(_host((gb, gc, gw[:npos * wb])), c["whole"])


@pytest.mark.parametrize("case", sorted(CASES))
def test_file_answers_every_position(case, tmp_path):
    """3. every (key, value, remoteness) of Solver.dump() is found through
    Tablebase.lookup_keys on the written file; unreached indexes read as such."""
    from gamesmanmpi_amd import db
    c = solved(case)
    path = str(tmp_path / "solution.gmtb")
    info = c["s"].export_tablebase(path, chunk=1 << 20)  # (toot 4x4: eight chunks, the last a partial one)
    assert info["positions"] == len(c["keys"]) and info["word_bytes"] == c["wb"]
    assert os.path.getsize(path) == info["bytes"] and not os.path.exists(path + ".tmp")
    tb = db.Tablebase(path, c["spec"])
    assert (tb.index_space, tb.positions, tb.word_bytes) == (c["space"], len(c["keys"]), c["wb"])
    np.testing.assert_array_equal(tb.lookup_keys(c["keys"]), c["words"])
    # the sections are the one-call export's
    bits, counts, words = c["whole"]
    np.testing.assert_array_equal(np.asarray(tb.bits), bits)
    np.testing.assert_array_equal(np.diff(np.asarray(tb.counts)), counts)
    np.testing.assert_array_equal(np.asarray(tb.words).view(np.uint8), words)
    reached = np.zeros(c["space"], bool)
    reached[c["spec"].tb_index(c["keys"]).astype(np.int64)] = True
    free = np.flatnonzero(~reached)
    if len(free):
        pick = free[np.random.default_rng(2).integers(0, len(free), 4096)]
        pick = np.concatenate([pick, free[:8], free[-8:]]).astype(np.uint64)
        assert (tb.lookup_indexes(pick) == NO_WORD).all()


@pytest.mark.parametrize("case", sorted(DIRECT))
def test_direct_equals_generic(case):
    """4. the storage-order kernels against index -> key -> the query path."""
    c = solved(case)
    _same(_host(c["s"].export_range(0, c["space"], c["wb"], generic=True)), c["whole"])


def test_wider_words_hold_the_same_values():
    c = solved("toot_3x3_ranked")
    for wb in (2, 4):
        for generic in (False, True):
            bits, counts, words = _host(c["s"].export_range(0, c["space"], wb, generic=generic))
            np.testing.assert_array_equal(bits, c["whole"][0])
            np.testing.assert_array_equal(words.view({2: np.uint16, 4: np.uint32}[wb]), c["whole"][2])


def test_refusals():
    from gamesmanmpi_amd import _lib
    from gamesmanmpi_amd.games import GameSpec
    from gamesmanmpi_amd.solver import Solver
    # remoteness >= 131 in one byte
    c = solved("planes_31_31_200_rel")
    assert c["wb"] == 2 and int((c["words"] >> 2).max()) >= 131
    for generic in (False, True):
        with pytest.raises(_lib.GmError) as ei:
            c["s"].export_range(0, c["space"], 1, generic=generic)
        assert ei.value.code == _lib.GM_EINVAL and "remoteness %d" % int((c["words"] >> 2).max()) in str(ei.value)
    # a short words_cap: GM_EFULL with the count needed
    c = solved("toot_3x4_ranked")
    import torch
    L, n = _lib.load(), ctypes.c_uint64()
    s, space = c["s"], c["space"]
    bits = torch.zeros(space // 64, dtype=torch.int64, device=s.device)
    counts = torch.zeros(space // 512, dtype=torch.int32, device=s.device)
    words = torch.zeros(64, dtype=torch.uint8, device=s.device)
    for how in (0, _lib.GM_EXPORT_GENERIC):
        with torch.cuda.device(s.device):
            rc = L.gm_solver_export(s.handle, how, 0, space, 1, bits.data_ptr(), counts.data_ptr(),
                                    words.data_ptr(), 64, ctypes.byref(n))
        assert rc == _lib.GM_EFULL and n.value == len(c["keys"])
        with pytest.raises(_lib.TableFull):
            s.export_range(0, space, 1, generic=bool(how), words_cap=len(c["keys"]) - 1)
    # ranges that are no whole blocks inside the space
    for first, count in ((0, 100), (64, 512), (0, space + 512), (space, 512)):
        with torch.cuda.device(s.device):
            rc = L.gm_solver_export(s.handle, 0, first, count, 1, bits.data_ptr(), counts.data_ptr(),
                                    words.data_ptr(), 64, ctypes.byref(n))
        assert rc == _lib.GM_EINVAL, (first, count)
    # an unsolved solver, a shard, a game without an index
    fresh = Solver(GameSpec(SUM, "heaps=31:31"), layout="planes")
    with pytest.raises(_lib.GmError) as ei:
        fresh.export_range(0, 1024, 1)
    assert ei.value.code == _lib.GM_EINVAL
    from gamesmanmpi_amd.dist import group_solve
    _, shards = group_solve(GameSpec(SUM, "heaps=7:7:7:15"), 2)  # (solved shards: the refusal is the shard's)
    for shard in shards:
        with pytest.raises(_lib.GmError) as ei:
            shard.export_range(0, 512, 1)
        assert ei.value.code == _lib.GM_EINVAL and "gm_solver_export" in str(ei.value)
    ttt = Solver(GameSpec("tic_tac_toe_np", ""))
    ttt.solve()
    with pytest.raises(_lib.GmError) as ei:
        ttt.export_range(0, 512, 1)
    assert ei.value.code == _lib.GM_EINVAL


def _run(main, argv):
    out = io.StringIO()
    with redirect_stdout(out):
        rc = main(argv)
    return rc, out.getvalue().splitlines()


def test_launcher_writes_a_tablebase(tmp_path):
    """-sd DIR --tablebase on toot 3x3, then the db command line on DIR."""
    from gamesmanmpi_amd import db, solver_launcher as sl
    game = os.path.join(ROOT, "tests", "games", "descriptor_toot", "toot_and_otto_bitstring.py")
    sd = str(tmp_path / "sd")
    rc, lines = _run(sl.main, [game, "-sd", sd, "--tablebase", "--no-verify"])
    assert rc == 0
    root_line = lines[0]
    c = solved("toot_3x3_ranked")
    assert root_line == c["r"].root_line
    d = os.path.join(sd, "stats", "0")
    assert sorted(os.listdir(d)) == ["meta.json", "solution.gmtb"]
    rc, lines = _run(db.main, [sd, "--game", game])
    assert rc == 0 and len(lines) == 1 and lines[0].endswith(": " + root_line)
    rc, lines = _run(db.main, [sd, "--game", game, "--moves"])
    assert rc == 0 and len(lines) > 1 and sum(x.endswith(" *") for x in lines) == 1
    opened = db.SolutionDB(sd)
    assert opened.meta["format"] == "gmtb" and len(opened) == len(c["keys"])
    # refused with a one-line message: no -sd, a game without an index
    with pytest.raises(SystemExit):
        sl.main([game, "--tablebase", "--no-verify"])
    with pytest.raises(SystemExit):
        sl.main([os.path.join(ROOT, "tests", "games", "grid_tictactoe.py"), "-sd", sd, "--tablebase"])
