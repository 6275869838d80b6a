#!/usr/bin/env python3
"""Connect four 5x4 and 6x5 (connect 4) on BUCKETED, plain and with
board_symmetry=1, with toot-and-otto 5x4 and 6x4 beside them, in one process
on one GPU: solve ms (gm_result's device time, median of argv[1] = 3 solves
after one warm-up solve), positions, edges and the plan's table, level and
scratch bytes.  A record, not a gate: one JSON line per row on stdout and the
table in profiles/connect_four_bench.txt (argv[2]).

Connect four 6x5 has no enumerated position count; its bound (the gravity
fillings, wins ignored) asks for a level of more than 2^32 edges, which the
plan refuses.  The row is then attempted with argv[3] positions (default
1.3e9) as the caller's estimate, and a refusal is recorded with its message.

--layout ranked (anywhere on the command line) writes another record instead,
profiles/connect_four_ranked_bench.txt: the RANKED layout of connect four
(csrc/gm_ranked_connect.h) beside BUCKETED on the plain boards both solve,
5x4 and 6x4, and alone on 7x4 and 6x5, which have no BUCKETED plan; forward,
backward and total ms, positions, edges, primitives and the table's bytes.
The file is rewritten after every row, so that a run cut short keeps the
rows it finished."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = [
    ("connect 5x4", "connect_four", "length=5,height=4,connect=4", 0),
    ("connect 6x5", "connect_four", "length=6,height=5,connect=4", None),
    ("toot 5x4", "toot_and_otto_bitstring", "length=5,height=4", 0),
    ("toot 6x4", "toot_and_otto_bitstring", "length=6,height=4", 0),
]


RANKED_CASES = [
    ("connect 5x4", "length=5,height=4,connect=4", ("ranked", "bucketed")),
    ("connect 6x4", "length=6,height=4,connect=4", ("ranked", "bucketed")),
    ("connect 7x4", "length=7,height=4,connect=4", ("ranked",)),
    ("connect 6x5", "length=6,height=5,connect=4", ("ranked",)),
]


def ranked_record(reps, out):
    import torch
    from gamesmanmpi_amd import _lib
    from gamesmanmpi_amd.games import GameSpec
    from gamesmanmpi_amd.solver import Solver
    fmt = "%-12s %-9s %10s %10s %10s %14s %14s %14s %15s  %s"
    head = fmt % ("board", "layout", "fwd ms", "bwd ms", "solve ms", "positions", "edges", "primitives",
                  "table bytes", "root")
    rows, notes = [], []

    def write():
        lines = [head] + rows + notes
        lines.append("(%s; median of %d solves after a warm-up, one process; plain boards, no board_symmetry)"
                     % (torch.cuda.get_device_name(0), reps))
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")
        return lines

    for board, params, layouts in RANKED_CASES:
        for layout in layouts:
            torch.cuda.empty_cache()
            try:
                s = Solver(GameSpec("connect_four", params), layout=layout)
                s.solve()  # warm-up
                rs = sorted((s.solve() for _ in range(reps)), key=lambda r: r.ms_total)
            except (_lib.GmError, RuntimeError, ValueError) as e:
                notes.append("%s %s: %s" % (board, layout, str(e)[:300]))
                print(json.dumps({"board": board, "layout": layout, "refused": str(e)[:300]}), flush=True)
                write()
                continue
            r = rs[len(rs) // 2]
            row = {"board": board, "layout": layout, "root": r.root_line, "ms_forward": round(r.ms_forward, 3),
                   "ms_backward": round(r.ms_backward, 3), "solve_ms": round(r.ms_total, 3),
                   "solve_ms_all": [round(x.ms_total, 3) for x in rs], "positions": int(r.positions),
                   "edges": int(r.edges), "primitives": int(r.primitives), "table_bytes": int(s.plan.table_bytes)}
            print(json.dumps(row), flush=True)
            rows.append(fmt % (board, layout, "%.3f" % r.ms_forward, "%.3f" % r.ms_backward, "%.3f" % r.ms_total,
                               r.positions, r.edges, r.primitives, s.plan.table_bytes, r.root_line))
            write()
            del s
    print("\n".join(write()), flush=True)
    return 0


def main():
    if "--layout" in sys.argv:
        at = sys.argv.index("--layout")
        layout = sys.argv[at + 1] if at + 1 < len(sys.argv) else ""
        del sys.argv[at:at + 2]
        if layout not in ("bucketed", "ranked"):
            raise SystemExit("--layout: bucketed (the default record) or ranked")
        if layout == "ranked":
            return ranked_record(int(sys.argv[1]) if len(sys.argv) > 1 else 3,
                                 sys.argv[2] if len(sys.argv) > 2
                                 else os.path.join(ROOT, "profiles", "connect_four_ranked_bench.txt"))
    import torch
    from gamesmanmpi_amd import _lib
    from gamesmanmpi_amd.games import GameSpec
    from gamesmanmpi_amd.solver import Solver
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 3
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "connect_four_bench.txt")
    estimate = int(float(sys.argv[3])) if len(sys.argv) > 3 else 1300000000
    rows, notes = [], []
    for board, stem, params, positions in CASES:
        for extra in ("", ",board_symmetry=1"):
            torch.cuda.empty_cache()
            spec = GameSpec(stem, params + extra)
            try:
                if positions is None:  # no known count: show what the bound plans, then try the estimate
                    try:
                        Solver(spec, layout="bucketed")
                    except (_lib.GmError, RuntimeError) as e:
                        notes.append("%s sym=%d, bound %d positions: %s" % (board, bool(extra), spec.positions_bound, e))
                s = Solver(spec, layout="bucketed", positions=estimate if positions is None else positions)
                r = s.solve()  # warm-up
                ms = sorted(s.solve().ms_total for _ in range(reps))
            except (_lib.GmError, RuntimeError) as e:
                notes.append("%s sym=%d with %d positions planned: %s" % (board, bool(extra), estimate, str(e)[:300]))
                print(json.dumps({"board": board, "board_symmetry": int(bool(extra)), "refused": str(e)[:300]}), flush=True)
                continue
            row = {"board": board, "board_symmetry": int(bool(extra)), "root": r.root_line,
                   "solve_ms": round(ms[len(ms) // 2], 3), "solve_ms_all": [round(m, 3) for m in ms],
                   "positions": int(r.positions), "edges": int(r.edges),
                   "table_bytes": int(s.plan.table_bytes), "level_bytes": 8 * int(s.plan.level_capacity),
                   "scratch_bytes": int(s.plan.scratch_bytes)}
            print(json.dumps(row), flush=True)
            rows.append(row)
            del s
    fmt = "%-12s %-4s %10s %14s %14s %15s %14s %10s  %s"
    lines = [fmt % ("board", "sym", "solve ms", "positions", "edges", "table bytes", "level bytes", "scratch", "root")]
    for r in rows:
        lines.append(fmt % (r["board"], r["board_symmetry"], "%.3f" % r["solve_ms"], r["positions"], r["edges"],
                            r["table_bytes"], r["level_bytes"], r["scratch_bytes"], r["root"]))
    lines += notes
    lines.append("(BUCKETED, %s; median of %d solves after a warm-up, one process; the plan's bounds are the plain "
                 "board's, not shrunk for the symmetric solve)" % (torch.cuda.get_device_name(0), reps))
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
