"""Connect Four (K_CONNECT, csrc/gm_games.h) on the GPU.  The oracle knows
nothing of the game, so the yardsticks are the game file itself, solved
through the host-enumerated graph path (GenericSolver runs the module's own
functions), and the fixtures tests/golden/make_connect_four.py generated
from the module."""
import functools
import io
import json
from contextlib import redirect_stdout

import numpy as np
import pytest

from test_connect_four_cpu import GAME_FILE, c4_graph, c4_params, c4_summary, c4_table, np_mirror, py_key

pytestmark = pytest.mark.gpu

WORD_BOARDS = [(4, 3, 3), (4, 4, 3), (4, 4, 4)]


def name_of(board):
    return "%dx%d_%d" % board


def spec_of(board, sym=False):
    from gamesmanmpi_amd.games import GameSpec
    return GameSpec("connect_four", c4_params(*board) + (",board_symmetry=1" if sym else ""))


@functools.lru_cache(maxsize=None)
def graph_words(board):
    """(keys sorted, words) of the graph solve of the module, computed once."""
    from gamesmanmpi_amd.generic import GenericSolver
    g = c4_graph(*board)
    s = GenericSolver(g)
    r = s.solve()
    names, val, rem = s.dump()
    keys = np.array([py_key(n) for n in names], np.uint64)
    order = np.argsort(keys)
    words = val.astype(np.uint32) | (rem.astype(np.uint32) << 2)
    return keys[order], words[order], r


@functools.lru_cache(maxsize=None)
def solved(board, layout, sym=False):
    from gamesmanmpi_amd.solver import Solver
    s = Solver(spec_of(board, sym), layout=layout)
    r = s.solve()
    assert r.extra["layout"] == layout
    return s, r


def sorted_dump(dumps):
    k = np.concatenate([d[0] for d in dumps])
    w = np.concatenate([d[1].astype(np.uint32) | (d[2].astype(np.uint32) << 2) for d in dumps])
    order = np.argsort(k)
    return k[order], w[order]


@pytest.mark.parametrize("layout", ["bucketed", "hashed"])
@pytest.mark.parametrize("board", WORD_BOARDS)
def test_single_table_word_for_word(board, layout):
    keys, words, gr = graph_words(board)
    s, r = solved(board, layout)
    assert (r.positions, r.edges, r.primitives, r.root_line) == (gr.positions, gr.edges, gr.primitives, gr.root_line)
    info = c4_summary()[name_of(board)]
    assert (r.positions, r.edges, r.root_line) == (info["positions"], info["edges"], info["root_line"])
    k, w = sorted_dump([s.dump()])
    np.testing.assert_array_equal(k, keys)
    np.testing.assert_array_equal(w, words)


def test_auto_layout_is_bucketed():
    from gamesmanmpi_amd.solver import Solver
    assert Solver(spec_of((4, 3, 3))).solve().extra["layout"] == "bucketed"


@pytest.mark.parametrize("local", [False, True])
@pytest.mark.parametrize("world", [3, 8])
@pytest.mark.parametrize("board", WORD_BOARDS)
def test_md5_shards_word_for_word(board, world, local):
    from gamesmanmpi_amd import _lib
    from gamesmanmpi_amd.keyed import group_keyed_solve
    keys, words, gr = graph_words(board)
    spec = spec_of(board)
    r, shards = group_keyed_solve(spec, world, flags=_lib.GM_F_BKS_LOCAL if local else 0)
    assert (r.positions, r.edges, r.root_line) == (gr.positions, gr.edges, gr.root_line)
    dumps = [sh.dump() for sh in shards]
    for rank, d in enumerate(dumps):
        if len(d[0]):
            assert (spec.owners_host(d[0], world) == rank).all()
    k, w = sorted_dump(dumps)
    np.testing.assert_array_equal(k, keys)
    np.testing.assert_array_equal(w, words)


def test_md5_hash_table_shards():
    from gamesmanmpi_amd.keyed import group_keyed_solve
    board = (4, 3, 3)
    keys, words, gr = graph_words(board)
    r, shards = group_keyed_solve(spec_of(board), 3, layout="hashed")
    assert (r.positions, r.edges, r.root_line) == (gr.positions, gr.edges, gr.root_line)
    k, w = sorted_dump([sh.dump() for sh in shards])
    np.testing.assert_array_equal(k, keys)
    np.testing.assert_array_equal(w, words)


def test_owner_kernel_against_md5():
    """gm_owner on the device (the register-resident form of the connect
    kinds) against hashlib on str(pos)."""
    import hashlib
    import torch
    from gamesmanmpi_amd import _lib
    g = c4_graph(4, 3, 3)
    spec = spec_of((4, 3, 3))
    keys = np.array([py_key(n) for n in g.names], np.uint64)
    kd = torch.from_numpy(keys.view(np.int64)).cuda()
    for P in (2, 3, 7, 8):
        od = torch.zeros(len(keys), dtype=torch.int32, device="cuda")
        _lib.check(_lib.load().gm_owner(spec.id, kd.data_ptr(), len(keys), P, od.data_ptr(),
                                        torch.cuda.current_stream().cuda_stream))
        want = [int(hashlib.md5(n.encode("utf-8")).hexdigest(), 16) % P for n in g.names]
        assert od.cpu().numpy().tolist() == want


@pytest.mark.parametrize("board", [(5, 4, 4), (1, 4, 4), (4, 1, 4), (2, 2, 2), (3, 2, 3)])
def test_counts_primitives_and_root_line(board):
    info = c4_summary()[name_of(board)]
    s, r = solved(board, "bucketed")
    assert (r.positions, r.edges, r.primitives, r.root_line) == (
        info["positions"], info["edges"], info["primitives"], info["root_line"])
    c = s.census()
    np.testing.assert_array_equal(c["by_level"].sum(axis=1)[:len(info["level_hist"])], info["level_hist"])
    np.testing.assert_array_equal(c["by_level"].sum(axis=0), info["value_hist_WLTD"])
    if board != (5, 4, 4):
        t = c4_table(name_of(board))
        k, w = sorted_dump([s.dump()])
        np.testing.assert_array_equal(k, t["keys"])
        np.testing.assert_array_equal(w, t["value"].astype(np.uint32) | (t["remoteness"].astype(np.uint32) << 2))


def test_5x4_is_the_tie_in_20():
    _, r = solved((5, 4, 4), "bucketed")
    assert (r.positions, r.root_line) == (3945711, "TIE in 20 moves")


def test_fixed_and_generic_kernels_agree_on_5x4():
    """connect=4 on 5x4 runs ConnectFixed<5,4,4>; the HASHED layout runs the
    generic K_CONNECT kernels: the same checksum over every position."""
    b, _ = solved((5, 4, 4), "bucketed")
    h, _ = solved((5, 4, 4), "hashed")
    assert b.checksum() == h.checksum()


@pytest.mark.parametrize("board", [(4, 4, 4), (5, 4, 4)])
def test_board_symmetry(board):
    L, H, K = board
    info = c4_summary()[name_of(board)]
    p, rp = solved(board, "bucketed")
    if board == (4, 4, 4):
        t = c4_table(name_of(board))
        keys = t["keys"]
        words = t["value"].astype(np.uint32) | (t["remoteness"].astype(np.uint32) << 2)
    else:  # no committed table of 3.9 M rows: the plain solve, pinned to the fixture's counts above
        keys, words = sorted_dump([p.dump()])
    reps = np.unique(np.minimum(keys, np_mirror(keys, L, H)))
    assert len(reps) == info["mirror_orbits"]
    s, r = solved(board, "bucketed", True)
    assert r.positions == len(reps) < rp.positions
    assert r.root_line == info["root_line"]
    w = s.query(keys)  # every key, representative or not
    np.testing.assert_array_equal(w, words)
    sk, sw = sorted_dump([s.dump()])
    np.testing.assert_array_equal(sk, reps)
    np.testing.assert_array_equal(sw, words[np.searchsorted(keys, reps)])
    a = s.audit()
    assert (a["mismatches"], a["positions"]) == (0, len(reps))
    # the census of the representatives, from the plain words
    want = np.bincount(words[np.searchsorted(keys, reps)] & 3, minlength=4)
    c = s.census()
    np.testing.assert_array_equal(c["by_remoteness"].sum(axis=0), want)
    np.testing.assert_array_equal(c["by_level"].sum(axis=0), want)
    # the plain solve's census totals, through the orbit sizes (1 for a self-mirror position, else 2)
    size = 1 + (np_mirror(reps, L, H) != reps)
    plain = np.bincount(words[np.searchsorted(keys, reps)] & 3, weights=size, minlength=4).astype(np.uint64)
    np.testing.assert_array_equal(p.census()["by_level"].sum(axis=0), plain)


def test_board_symmetry_hashed_and_shards():
    from gamesmanmpi_amd.keyed import group_keyed_solve
    board = (4, 4, 4)
    s, r = solved(board, "bucketed", True)
    ref = sorted_dump([s.dump()])
    h, rh = solved(board, "hashed", True)
    assert rh.positions == r.positions
    for a, b in zip(sorted_dump([h.dump()]), ref):
        np.testing.assert_array_equal(a, b)
    rg, shards = group_keyed_solve(spec_of(board, True), 3)
    assert (rg.positions, rg.edges, rg.root_line) == (r.positions, r.edges, r.root_line)
    for a, b in zip(sorted_dump([sh.dump() for sh in shards]), ref):
        np.testing.assert_array_equal(a, b)


def test_audit_census_moves_and_best_line():
    board = (4, 4, 4)
    t = c4_table(name_of(board))
    info = c4_summary()[name_of(board)]
    s, r = solved(board, "bucketed")
    a = s.audit()
    assert (a["mismatches"], a["positions"], a["edges"]) == (0, info["positions"], info["edges"])
    c = s.census()
    np.testing.assert_array_equal(c["by_level"].sum(axis=0), info["value_hist_WLTD"])
    np.testing.assert_array_equal(c["by_level"].sum(axis=1)[:len(info["level_hist"])], info["level_hist"])
    np.testing.assert_array_equal(c["by_remoteness"].sum(axis=0), np.bincount(t["value"], minlength=4))
    np.testing.assert_array_equal(c["by_remoteness"][:, 2][:int(t["remoteness"].max()) + 1],
                                  np.bincount(t["remoteness"][t["value"] == 2]))
    # moves: the children in gen_moves order with the fixture's words
    at = np.arange(0, len(t["keys"]), 101)
    keys = t["keys"][at]
    ch, wd, nc, best = s.moves(keys)
    np.testing.assert_array_equal(nc, t["nchild"][at])
    pr, hn, hc = s.spec.host_expand(keys)
    words = t["value"].astype(np.uint32) | (t["remoteness"].astype(np.uint32) << 2)
    for i in range(len(keys)):
        n = int(nc[i])
        assert ch[i, :n].tolist() == hc[i, :n].tolist()
        assert wd[i, :n].tolist() == words[np.searchsorted(t["keys"], ch[i, :n])].tolist()
        assert (best[i] == -1) == (n == 0)
    # the line from the root: one position per move, as long as the root's remoteness
    lk, lv, lr = s.best_line()
    assert int(lk[0]) == 0 and len(lk) == r.root_remoteness + 1 == 17
    assert lr.tolist() == list(range(r.root_remoteness, -1, -1))
    assert set(lv.tolist()) == {2}
    for a_, b_ in zip(lk[:-1], lk[1:]):
        _, n1, c1 = s.spec.host_expand(np.array([a_], np.uint64))
        assert int(b_) in c1[0, :n1[0]].tolist()


def test_keyed_tablebase_round_trip(tmp_path):
    from gamesmanmpi_amd import _lib, db
    board = (4, 4, 4)
    t = c4_table(name_of(board))
    s, _ = solved(board, "bucketed")
    with pytest.raises(_lib.GmError):
        s.spec.tb_index_space()  # no indexed tablebase for this game
    d = tmp_path / "stats" / "0"
    d.mkdir(parents=True)
    info = s.export_keyed_tablebase(str(d / db.TK_NAME))
    assert info["positions"] == len(t["keys"])
    (d / "meta.json").write_text(json.dumps({"game": s.spec.name, "params": s.spec.params, "format": "gmtk"}))
    sdb = db.SolutionDB(str(tmp_path))
    w = sdb.tablebase.lookup_keys(t["keys"])
    np.testing.assert_array_equal(w, t["value"].astype(np.uint32) | (t["remoteness"].astype(np.uint32) << 2))
    assert sdb.lookup("-" * 16, s.spec) == (2, 16)
    assert sdb.tablebase.lookup_key(py_key("O" + "-" * 15)) is None  # O never moves first


def test_checkpoint_mid_forward_and_mid_backward(tmp_path):
    from gamesmanmpi_amd import checkpoint
    from gamesmanmpi_amd.solver import Solver
    board = (4, 3, 3)
    keys, words, gr = graph_words(board)
    T = spec_of(board).max_levels
    for cut in (T // 2, T + T // 2):  # forward steps are [0, T - 1), backward the rest
        s = Solver(spec_of(board), layout="bucketed")
        assert T - 1 < s.steps and 0 < cut < s.steps
        assert s.solve_steps(0, cut) is None
        ck = str(tmp_path / ("ck%d" % cut))
        checkpoint.save(s, ck, cut)
        del s
        s2, step = checkpoint.restore(ck)
        assert step == cut
        r = s2.solve_steps(step, 0)
        assert (r.positions, r.root_line) == (gr.positions, gr.root_line)
        k, w = sorted_dump([s2.dump()])
        np.testing.assert_array_equal(k, keys)
        np.testing.assert_array_equal(w, words)


def test_staging_capacity_mixed_forms():
    """Solver(staging_records=N) with N the widest level's out-edges: by the
    fixture's per-level counts some levels overflow their count-free regions
    and are redone counted, others are not; a redone level costs 5 more
    forward launches."""
    from gamesmanmpi_amd.solver import Solver
    from test_gpu_bucketed_capacity import KBKC, _cap, _mix64
    board = (4, 4, 4)
    t = c4_table(name_of(board))
    spec = spec_of(board)
    T = spec.max_levels
    pr, nc, ch = spec.host_expand(t["keys"])
    np.testing.assert_array_equal(nc, t["nchild"])  # the fixture's own child counts
    valid = np.arange(ch.shape[1])[None, :] < nc[:, None]
    plev = np.repeat(t["level"].astype(np.int64), nc)
    part = (_mix64(ch[valid]) >> np.uint64(56)).astype(np.int64)
    width = np.bincount(t["level"], minlength=T)
    edges = np.bincount(plev, minlength=T)
    fullest = np.bincount(plev * KBKC + part, minlength=T * KBKC).reshape(T, KBKC).max(1)
    n = int(edges.max())
    want = [lv for lv in range(T) if fullest[lv] > _cap(n)]
    with_children = int((edges > 0).sum())
    assert 0 < len(want) < with_children, (n, _cap(n), fullest.tolist())
    base = 2 * int((width[:T - 1] > 0).sum()) + 4 * with_children
    s = Solver(spec, layout="bucketed", positions=len(t["keys"]), staging_records=n, kernel_timing=True)
    table = s.buffers[0]
    table[s.claimed_table_bytes:].fill_(0xA5)
    r = s.solve()
    s.torch.cuda.synchronize(s.device)
    assert bool((table[s.claimed_table_bytes:] == 0xA5).all().item())
    extra = r.n_expand_launches - base
    print("connect four 4x4: N=%d cap=%d launches=%d base=%d" % (n, _cap(n), r.n_expand_launches, base))
    assert extra == 5 * len(want)
    k, w = sorted_dump([s.dump()])
    np.testing.assert_array_equal(k, t["keys"])
    np.testing.assert_array_equal(w, t["value"].astype(np.uint32) | (t["remoteness"].astype(np.uint32) << 2))


@pytest.mark.parametrize("sym", [False, True])
def test_launcher(sym):
    from gamesmanmpi_amd import solver_launcher as sl
    info = c4_summary()["5x4_4"]  # the game file's default board
    out = io.StringIO()
    with redirect_stdout(out):
        rc = sl.main([GAME_FILE] + (["--board-symmetry"] if sym else []))
    lines = out.getvalue().splitlines()
    assert rc == 0 and lines[0] == info["root_line"] == "TIE in 20 moves"
    if sym:
        assert lines[1] == "%d representatives" % info["mirror_orbits"]
