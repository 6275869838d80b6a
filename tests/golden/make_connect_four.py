#!/usr/bin/env python3
"""Generate tests/golden/connect_four/ from gamesmanmpi_amd/games/connect_four.py
through the module's own API (initial_position / gen_moves / do_move /
primitive).  Nothing of the device library is imported: the fixtures are an
independent yardstick for its descriptor.

Every move adds one piece, so the positions are enumerated level by level
(level = pieces on the board) and solved from the last level down with the
reference-canonical retrograde (make_golden.py): value = WIN if any child is
a LOSS, else TIE if any TIE, else LOSS; remoteness = 1 + min over the LOSS
children for a WIN, otherwise 1 + max over all children; primitives have
remoteness 0.

Writes
  summary.json     per board: positions, edges, primitives, level_hist,
                   max_level_width, value_hist_WLTD, root_line, mirror_orbits
                   (orbits of the positions under the left-right mirror)
  <board>.npz      for the boards in TABLES, every reachable position:
                   keys (uint64, sorted), value, remoteness, nchild, level.
                   A key packs the string: bit i set for pos[i] == 'X', bit
                   length*height + i set for pos[i] == 'O'.

Usage:  python tests/golden/make_connect_four.py [BOARD ...]
"""
import importlib.util
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "connect_four")

WIN, LOSS, TIE, DRAW, UNDECIDED = 0, 1, 2, 3, 4
NAMES = ("WIN", "LOSS", "TIE", "DRAW")

# name -> (length, height, connect)
BOARDS = {
    "2x2_2": (2, 2, 2), "3x2_3": (3, 2, 3), "1x4_4": (1, 4, 4), "4x1_4": (4, 1, 4),
    "3x3_3": (3, 3, 3), "4x3_3": (4, 3, 3), "4x4_3": (4, 4, 3), "4x4_4": (4, 4, 4),
    "5x4_4": (5, 4, 4),
}
TABLES = ("2x2_2", "3x2_3", "1x4_4", "4x1_4", "3x3_3", "4x4_4")


def load_module(length, height, connect):
    sys.path.insert(0, os.path.join(REPO, "gamesmanmpi_amd", "compat"))  # src.utils
    path = os.path.join(REPO, "gamesmanmpi_amd", "games", "connect_four.py")
    spec = importlib.util.spec_from_file_location("gm_connect_four", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.length, mod.height, mod.connect = length, height, connect
    return mod


def key_of(pos):
    A, k = len(pos), 0
    for i, c in enumerate(pos):
        if c == "X":
            k |= 1 << i
        elif c == "O":
            k |= 1 << (A + i)
    return k


def solve(mod):
    """(levels, info): levels[L] = {pos: (value, remoteness, nchild)}"""
    levels = [[mod.initial_position()]]
    kids = []  # per level: pos -> children (None for primitives)
    while levels[-1]:
        nxt, seen, ch = [], set(), {}
        for pos in levels[-1]:
            if mod.primitive(pos) != UNDECIDED:
                ch[pos] = None
                continue
            cs = [mod.do_move(pos, m) for m in mod.gen_moves(pos)]
            if not cs:
                raise RuntimeError("non-primitive position without moves: %r" % pos)
            ch[pos] = cs
            for c in cs:
                if c not in seen:
                    seen.add(c)
                    nxt.append(c)
        kids.append(ch)
        levels.append(nxt)
    levels.pop()
    solved = [None] * len(levels)
    for L in range(len(levels) - 1, -1, -1):
        below = solved[L + 1] if L + 1 < len(levels) else {}
        out = {}
        for pos in levels[L]:
            cs = kids[L][pos]
            if cs is None:
                out[pos] = (int(mod.primitive(pos)), 0, 0)
                continue
            cv = [below[c] for c in cs]
            losses = [r for v, r, _ in cv if v == LOSS]
            if losses:
                out[pos] = (WIN, 1 + min(losses), len(cs))
            else:
                v = TIE if any(x[0] == TIE for x in cv) else DRAW if any(x[0] == DRAW for x in cv) else LOSS
                out[pos] = (v, 1 + max(r for _, r, _ in cv), len(cs))
        solved[L] = out
        kids[L] = None
    return solved


def main():
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, "summary.json")
    summary = json.load(open(path)) if os.path.exists(path) else {}
    for name in sys.argv[1:] or BOARDS:
        length, height, connect = BOARDS[name]
        t0 = time.time()
        mod = load_module(length, height, connect)
        solved = solve(mod)
        hist = [0, 0, 0, 0]
        prims = edges = 0
        for lv in solved:
            for v, r, n in lv.values():
                hist[v] += 1
                edges += n
                prims += n == 0
        # orbits under the left-right mirror x -> length - 1 - x, on the strings
        orbits = 0
        for lv in solved:
            for pos in lv:
                img = "".join(pos[length * y:length * (y + 1)][::-1] for y in range(height))
                orbits += key_of(pos) <= key_of(img)
        rv, rr, _ = solved[0][mod.initial_position()]
        widths = [len(lv) for lv in solved]
        summary[name] = {
            "length": length, "height": height, "connect": connect,
            "positions": sum(widths), "edges": edges, "primitives": prims,
            "level_hist": widths, "max_level_width": max(widths),
            "value_hist_WLTD": hist, "mirror_orbits": orbits, "root_line": "%s in %d moves" % (NAMES[rv], rr),
            "source": "gamesmanmpi_amd/games/connect_four.py through tests/golden/make_connect_four.py",
        }
        if name in TABLES:
            rows = sorted((key_of(p), v, r, n, L) for L, lv in enumerate(solved) for p, (v, r, n) in lv.items())
            cols = list(zip(*rows))
            np.savez_compressed(os.path.join(OUT, name + ".npz"),
                                keys=np.array(cols[0], np.uint64), value=np.array(cols[1], np.uint8),
                                remoteness=np.array(cols[2], np.uint8), nchild=np.array(cols[3], np.uint8),
                                level=np.array(cols[4], np.uint8))
        print(name, summary[name]["positions"], summary[name]["edges"], summary[name]["root_line"],
              "%.1f s" % (time.time() - t0), flush=True)
        with open(path, "w") as f:
            json.dump(summary, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
