"""Solution database written by the launcher's -sd option, and queries on it.

The reference keeps a rank's results in shelve files
`<DIR>/stats/<rank>/{resolved,remote}` (src/cache_dict.py:19-42): value and
remoteness per position key.  The launcher writes the binary counterpart,
`<DIR>/stats/<rank>/solution.npz` + `meta.json` per rank (solver_launcher.py
write_stats), and this module reads any number of rank directories back as
one table:

    python -m gamesmanmpi_amd.db DIR --game GAME_FILE [POSITION ...]

prints `<position>: <VALUE> in <r> moves` for each position (a Python
literal evaluated against nothing but literals, e.g. 4 or '...'), or for the
game's initial position when none is given.  Descriptor-solved tables are
keyed by the packed u64 key (GameSpec.key_of); graph-solved tables (game
files without a descriptor) by str(position).

    python -m gamesmanmpi_amd.db DIR --game GAME_FILE --moves [POSITION ...]

adds, under each position, one row per legal move (the module's gen_moves /
do_move) with the child's value and remoteness from the table, the best move
marked with `*` (best_index below; the rule of gm_solver_moves,
include/gamesman.h).

    python -m gamesmanmpi_amd.db DIR --game GAME_FILE --census

prints the analysis table of the whole solution instead: positions by
remoteness x (Win Lose Tie Draw Total), then by level x the same
(census_of / format_census below; the launcher's --census prints the same
tables from the device's gm_solver_census).  Graph tables have no level
function and print the remoteness table only.  Host only: no GPU is touched.
"""
import argparse
import ast
import glob
import json
import os
import sys

import numpy as np

NAMES = ("WIN", "LOSS", "TIE", "DRAW")


class SolutionDB:
    def __init__(self, root):
        ranks = sorted(glob.glob(os.path.join(root, "stats", "*", "solution.npz")))
        if not ranks:
            raise FileNotFoundError("no stats/<rank>/solution.npz under %r" % root)
        keys, names, val, rem, metas = [], [], [], [], []
        for path in ranks:
            with np.load(path) as z:  # allow_pickle stays False
                if "keys" in z.files:
                    keys.append(z["keys"].astype(np.uint64))
                else:
                    names.append(z["names"])
                val.append(z["value"].astype(np.uint8))
                rem.append(z["remoteness"].astype(np.uint32))
            with open(os.path.join(os.path.dirname(path), "meta.json")) as f:
                metas.append(json.load(f))
        if keys and names:
            raise ValueError("mixed keyed and graph tables under %r" % root)
        self.meta = metas[0]
        self.ranks = len(ranks)
        self.value = np.concatenate(val)
        self.remoteness = np.concatenate(rem)
        if keys:
            self.by = "key"
            k = np.concatenate(keys)
            order = np.argsort(k, kind="stable")
            self.keys = k[order]
            if len(self.keys) > 1 and (np.diff(self.keys) == 0).any():
                raise ValueError("a position appears in two rank files")
            self.value, self.remoteness = self.value[order], self.remoteness[order]
        else:
            self.by = "name"
            self.index = {str(n): i for i, n in enumerate(np.concatenate(names))}

    def __len__(self):
        return len(self.value)

    def lookup_key(self, key):
        i = int(np.searchsorted(self.keys, np.uint64(key)))
        if i == len(self.keys) or int(self.keys[i]) != int(key):
            return None
        return int(self.value[i]), int(self.remoteness[i])

    def lookup_name(self, name):
        i = self.index.get(name)
        return None if i is None else (int(self.value[i]), int(self.remoteness[i]))

    def lookup(self, pos, spec=None):
        """(value, remoteness) of a game position, or None if unreachable."""
        if self.by == "name":
            return self.lookup_name(str(pos))
        if spec is None:
            raise ValueError("a keyed table needs the game's GameSpec")
        key = spec.key_of(pos)
        if "symmetry=1" in self.meta.get("params", "").split(","):
            # a symmetric solve stored orbit representatives (gm_symmetry)
            from .games import GameSpec
            key = int(GameSpec(spec.name, self.meta["params"]).symmetry(
                np.array([key], np.uint64))[0])
        return self.lookup_key(key)


def best_index(children):
    """Index of the best move among `children`, a list of (value,
    remoteness) in gen_moves order -- the rule of gm_solver_moves: a WIN
    parent (some child is a LOSS) takes the first LOSS child of the smallest
    remoteness; a TIE parent the first TIE child of the largest remoteness
    among TIE children; a DRAW parent the first DRAW child; a LOSS parent
    the first child of the largest remoteness.  None without children or
    with a child the table does not hold."""
    if not children or any(c is None for c in children):
        return None
    WIN, LOSS, TIE, DRAW = range(4)
    vals = [v for v, _ in children]
    if LOSS in vals:
        cand = [(r, i) for i, (v, r) in enumerate(children) if v == LOSS]
        return min(cand)[1]
    for pv in (TIE, DRAW):
        if pv in vals:
            cand = [(-r if pv == TIE else 0, i) for i, (v, r) in enumerate(children) if v == pv]
            return min(cand)[1]
    return min((-r, i) for i, (v, r) in enumerate(children))[1]


def census_of(value, remoteness, levels=None, rem_bins=None):
    """The census of a table held on the host, in gm_solver_census' layout:
    dict with by_remoteness (uint64 [rem_bins + 1, 4]: positions of remoteness
    r and value WIN / LOSS / TIE / DRAW, the last row every remoteness >=
    rem_bins) and by_level (uint64 [max level + 1, 4], or None without
    `levels`, the level of each position).  rem_bins defaults to the largest
    remoteness + 1, which leaves the overflow row empty."""
    value = np.asarray(value).astype(np.int64)
    remoteness = np.asarray(remoteness).astype(np.int64)
    if rem_bins is None:
        rem_bins = int(remoteness.max()) + 1 if len(remoteness) else 0
    by_rem = np.zeros((int(rem_bins) + 1, 4), np.uint64)
    np.add.at(by_rem, (np.minimum(remoteness, int(rem_bins)), value), 1)
    by_lev = None
    if levels is not None:
        levels = np.asarray(levels).astype(np.int64)
        by_lev = np.zeros((int(levels.max()) + 1 if len(levels) else 0, 4), np.uint64)
        np.add.at(by_lev, (levels, value), 1)
    return {"by_remoteness": by_rem, "by_level": by_lev}


def _census_table(title, rows, overflow=None):
    """One table: non-empty rows of `rows` ([n, 4]), then the totals.
    overflow: the index of a last row that collects everything from there on."""
    rows = np.asarray(rows).astype(np.uint64)
    fmt = "%12s" + " %14s" * 5
    out = [fmt % (title, "Win", "Lose", "Tie", "Draw", "Total")]
    for i, row in enumerate(rows.tolist()):
        if sum(row):
            label = ">=%d" % i if i == overflow else "%d" % i
            out.append(fmt % ((label,) + tuple(row) + (sum(row),)))
    tot = [int(x) for x in rows.sum(axis=0, dtype=np.uint64)] if len(rows) else [0] * 4
    out.append(fmt % (("Total",) + tuple(tot) + (sum(tot),)))
    return out


def format_census(by_remoteness, by_level=None):
    """The analysis table as text: remoteness x (Win Lose Tie Draw Total),
    non-empty rows only, with a totals line; then, with by_level, level x the
    same.  The last row of by_remoteness is the overflow row (census_of)."""
    lines = _census_table("Remoteness", by_remoteness, overflow=len(by_remoteness) - 1)
    if by_level is not None:
        lines.append("")
        lines.extend(_census_table("Level", by_level))
    return "\n".join(lines)


def db_census(db, spec=None, rem_bins=None):
    """census_of a SolutionDB: keyed tables get their levels from
    GameSpec.host_level, graph tables (by name) have none."""
    levels = None
    if db.by == "key":
        if spec is None:
            raise ValueError("a keyed table needs the game's GameSpec")
        levels = spec.host_level(db.keys)
    return census_of(db.value, db.remoteness, levels, rem_bins)


def position_moves(db, mod, pos, spec=None):
    """[(move, child position, (value, remoteness) or None)] for every legal
    move of a non-primitive position, in gen_moves order."""
    from .solver_launcher import ensure_src_utils
    utils = ensure_src_utils()  # the constants the module itself imports
    if mod.primitive(pos) != utils.UNDECIDED:
        return []
    out = []
    for mv in mod.gen_moves(pos):
        child = mod.do_move(pos, mv)
        out.append((mv, child, db.lookup(child, spec)))
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(prog="gamesmanmpi_amd.db")
    ap.add_argument("statsdir")
    ap.add_argument("--game", required=True, help="the game file that was solved")
    ap.add_argument("--moves", action="store_true",
                    help="list every legal move of each position with the child's "
                         "value and remoteness; `*` marks the best move")
    ap.add_argument("--census", action="store_true",
                    help="print the whole solution's positions by remoteness and by level "
                         "(Win Lose Tie Draw Total per row) instead of looking positions up")
    ap.add_argument("--rem-bins", type=int, default=None, metavar="N",
                    help="--census: remoteness rows 0..N-1, then one row for the rest "
                         "(default: every remoteness its own row)")
    ap.add_argument("positions", nargs="*")
    args = ap.parse_intermixed_args(argv)
    from . import _lib
    from .solver_launcher import ensure_src_utils, load_game
    ensure_src_utils()
    mod = load_game(args.game)
    db = SolutionDB(args.statsdir)
    spec = None
    if db.by == "key":
        from .games import spec_for_module
        spec = spec_for_module(mod, os.path.splitext(os.path.basename(args.game))[0])
    if args.census:
        c = db_census(db, spec, args.rem_bins)
        print(format_census(c["by_remoteness"], c["by_level"]))
        return 0
    todo = [ast.literal_eval(p) for p in args.positions] or [mod.initial_position()]
    rc = 0
    for pos in todo:
        try:
            r = db.lookup(pos, spec)
        except _lib.GmError:  # no key: outside the game's state space
            r = None
        if r is None:
            print("%s: not reachable" % (pos,))
            rc = 1
        else:
            print("%s: %s in %d moves" % (pos, NAMES[r[0]], r[1]))
            if args.moves:
                rows = position_moves(db, mod, pos, spec)
                best = best_index([c for _, _, c in rows])
                for i, (mv, child, c) in enumerate(rows):
                    what = "not reachable" if c is None else "%s in %d moves" % (NAMES[c[0]], c[1])
                    print("  %s -> %s: %s%s" % (mv, child, what, " *" if i == best else ""))
                    if c is None:
                        rc = 1
    return rc


if __name__ == "__main__":
    sys.exit(main())
