"""Host side of the move analysis: `python -m gamesmanmpi_amd.db --moves` on
keyed and graph (name-keyed) tables written from a CPU oracle solve, the
launcher's --audit / --line flags, and the new ABI symbols.  No GPU."""
import io
import json
import os
from contextlib import redirect_stdout

import numpy as np
import pytest

from conftest import ROOT

OWN_SUM = os.path.join(ROOT, "gamesmanmpi_amd", "games", "sum_four_to_one.py")
GRID = os.path.join(ROOT, "tests", "games", "grid_tictactoe.py")
NAMES = ("WIN", "LOSS", "TIE", "DRAW")


def _write_rank(root, rank, **arrays):
    d = os.path.join(root, "stats", str(rank))
    os.makedirs(d, exist_ok=True)
    np.savez_compressed(os.path.join(d, "solution.npz"), **arrays)
    with open(os.path.join(d, "meta.json"), "w") as f:
        json.dump({"owned_by_rank": rank}, f)


def _best(children):
    """The rule of include/gamesman.h, restated: children = [(value, rem)]."""
    vals = [v for v, _ in children]
    if 1 in vals:  # a LOSS child: the parent wins, as fast as it can
        m = min(r for v, r in children if v == 1)
        return next(i for i, c in enumerate(children) if c == (1, m))
    for pv in (2, 3):  # TIE, then DRAW
        if pv in vals:
            m = max(r for v, r in children if v == pv)
            return next(i for i, (v, r) in enumerate(children) if v == pv and (pv == 3 or r == m))
    m = max(r for _, r in children)  # every child wins: lose as slowly as possible
    return next(i for i, (_, r) in enumerate(children) if r == m)


def _run(argv):
    from gamesmanmpi_amd.db import main
    out = io.StringIO()
    with redirect_stdout(out):
        rc = main(argv)
    return rc, out.getvalue().splitlines()


def test_db_moves_keyed(tmp_path):
    from oracle.oracle import Game
    heaps = (4, 6, 3)
    game = tmp_path / "sum_four_to_one.py"
    game.write_text(open(OWN_SUM).read().replace(
        "HEAPS = (31, 31, 31, 31, 31, 31)", "HEAPS = %r" % (heaps,)))
    sol = Game("sum_four_to_one", "heaps=4:6:3").solve()
    keys = np.arange(5 * 7 * 4, dtype=np.uint64)
    vr = np.array([sol.lookup(str(k).encode()) for k in keys.tolist()])
    _write_rank(tmp_path / "sd", 0, keys=keys, value=vr[:, 0].astype(np.uint8),
                remoteness=vr[:, 1].astype(np.uint32))
    stride = (1, 5, 35)
    for k in (139, 57, 0, 1, 36):
        rc, lines = _run([str(tmp_path / "sd"), "--game", str(game), "--moves", str(k)])
        assert rc == 0
        v, m = sol.lookup(str(k).encode())
        assert lines[0] == "%d: %s in %d moves" % (k, NAMES[v], m)
        digits = [(k // stride[i]) % (heaps[i] + 1) for i in range(3)]
        kids = [k - t * stride[i] for i in range(3) for t in (1, 2) if digits[i] >= t]
        assert len(lines) == 1 + len(kids)
        if not kids:
            continue
        cvr = [tuple(int(x) for x in sol.lookup(str(c).encode())) for c in kids]
        best = _best(cvr)
        for j, (c, (cv, cm)) in enumerate(zip(kids, cvr)):
            assert lines[1 + j].endswith("-> %d: %s in %d moves%s" % (c, NAMES[cv], cm, " *" if j == best else ""))
        assert sum(line.endswith(" *") for line in lines) == 1
    # past the heaps: not in the table
    rc, lines = _run([str(tmp_path / "sd"), "--game", str(game), "--moves", "140"])
    assert rc == 1 and lines == ["140: not reachable"]


def _solve_module(mod):
    """Every position of a game module reachable from its initial position,
    solved with the reference-canonical retrograde: {str(pos): (v, r)}."""
    seen, order, stack = {}, [], [mod.initial_position()]
    while stack:
        p = stack.pop()
        if str(p) in seen:
            continue
        kids = [] if mod.primitive(p) != 4 else [mod.do_move(p, m) for m in mod.gen_moves(p)]
        seen[str(p)] = (p, kids)
        order.append(str(p))
        stack.extend(kids)
    sol = {}

    def solve(name):
        if name in sol:
            return sol[name]
        p, kids = seen[name]
        if not kids:
            sol[name] = (int(mod.primitive(p)), 0)
            return sol[name]
        c = [solve(str(k)) for k in kids]
        loss = [r for v, r in c if v == 1]
        if loss:
            sol[name] = (0, min(loss) + 1)
        else:
            v = 2 if any(v == 2 for v, _ in c) else 3 if any(v == 3 for v, _ in c) else 1
            sol[name] = (v, max(r for _, r in c) + 1)
        return sol[name]

    for name in order:
        solve(name)
    return sol, seen


def test_db_moves_graph_rows(tmp_path):
    """position_moves / best_index on a name-keyed table, positions as the
    module's own objects (what --moves prints for the initial position)."""
    from gamesmanmpi_amd.db import SolutionDB, best_index, position_moves
    from gamesmanmpi_amd.solver_launcher import ensure_src_utils, load_game
    ensure_src_utils()
    mod = load_game(GRID)
    sol, seen = _solve_module(mod)
    names = sorted(sol)
    _write_rank(tmp_path / "sd", 0, names=np.array(names),
                value=np.array([sol[n][0] for n in names], np.uint8),
                remoteness=np.array([sol[n][1] for n in names], np.uint32))
    db = SolutionDB(str(tmp_path / "sd"))
    start = mod.initial_position()
    mid = mod.do_move(mod.do_move(start, (1, (1, 1))), (2, (0, 1)))
    won = next(p for p, kids in seen.values() if not kids)
    for pos in (start, mid, won):
        rows = position_moves(db, mod, pos)
        kids = seen[str(pos)][1]
        assert [str(c) for _, c, _ in rows] == [str(k) for k in kids]
        assert [c for _, _, c in rows] == [sol[str(k)] for k in kids]
        if kids:
            assert best_index([c for _, _, c in rows]) == _best([sol[str(k)] for k in kids])
        else:
            assert rows == [] and best_index([]) is None
    assert sol[str(mid)][0] == 0  # the mover wins: the best move is a LOSS child of the least remoteness
    rows = position_moves(db, mod, mid)
    b = best_index([c for _, _, c in rows])
    assert rows[b][2] == (1, sol[str(mid)][1] - 1)
    # the CLI on the initial position (no literal needed)
    rc, lines = _run([str(tmp_path / "sd"), "--game", GRID, "--moves"])
    assert rc == 0
    body = "\n".join(lines)
    assert body.count(" -> ") == 9 and body.count(" *") == 1
    assert "TIE in 9 moves" in body
    # a position the table does not hold
    rc, lines = _run([str(tmp_path / "sd"), "--game", GRID, "--moves", "[[1, 1, 1], [1, 1, 1], [1, 1, 1]]"])
    assert rc == 1 and len(lines) == 1 and lines[0].endswith(": not reachable")


def test_best_index_rule():
    from gamesmanmpi_amd.db import best_index
    W, L, T, D = range(4)
    assert best_index([(W, 3), (L, 4), (L, 2), (L, 2), (T, 9)]) == 2   # WIN: first LOSS of the least remoteness
    assert best_index([(W, 9), (T, 2), (T, 5), (T, 5), (D, 7)]) == 2   # TIE: first TIE of the largest TIE remoteness
    assert best_index([(W, 9), (D, 0), (D, 3)]) == 1                   # DRAW: the first DRAW child
    assert best_index([(W, 1), (W, 5), (W, 5), (W, 3)]) == 1           # LOSS: first child of the largest remoteness
    assert best_index([]) is None and best_index([(W, 1), None]) is None


def test_launcher_flags():
    from gamesmanmpi_amd.solver_launcher import build_parser, check_analysis_args
    a = build_parser().parse_args(["game.py", "--audit", "--line"])
    assert a.audit and a.line
    check_analysis_args(a, 1)  # one GPU: accepted
    for flags in (["--audit"], ["--line"], ["--audit", "--line"]):
        a = build_parser().parse_args(["game.py"] + flags)
        with pytest.raises(SystemExit):
            check_analysis_args(a, 2)
        with pytest.raises(SystemExit):
            check_analysis_args(a, 1, descriptor=False)
    a = build_parser().parse_args(["game.py", "--audit", "--layout", "graph"])
    with pytest.raises(SystemExit):
        check_analysis_args(a, 1)
    plain = build_parser().parse_args(["game.py"])
    assert not plain.audit and not plain.line
    check_analysis_args(plain, 8)  # nothing asked: nothing refused


def test_launcher_rejects_audit_under_torchrun(monkeypatch):
    """main() refuses at argument validation, before the game file loads."""
    from gamesmanmpi_amd import solver_launcher
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setenv("RANK", "0")
    with pytest.raises(SystemExit) as e:
        solver_launcher.main(["/nonexistent/game.py", "--audit"])
    assert "one-GPU" in str(e.value)


def test_new_symbols_exported_with_signatures():
    import ctypes
    from gamesmanmpi_amd import _lib
    lib = _lib.load()
    want = {
        "gm_solver_moves": [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p,
                            ctypes.c_void_p, ctypes.c_void_p],
        "gm_solver_line": [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64,
                           ctypes.POINTER(ctypes.c_uint64)],
        "gm_solver_audit": [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p],
    }
    for name, args in want.items():
        assert name in _lib.EXPORTS
        f = getattr(lib, name)
        assert list(f.argtypes) == args and f.restype is ctypes.c_int
    # null handles are refused, not dereferenced
    n = ctypes.c_uint64()
    out = (ctypes.c_uint64 * 4)()
    assert lib.gm_solver_moves(None, None, 1, None, None, None, None) == _lib.GM_EINVAL
    assert lib.gm_solver_line(None, 0, None, None, 0, ctypes.byref(n)) == _lib.GM_EINVAL
    assert lib.gm_solver_audit(None, None, 0, out) == _lib.GM_EINVAL
