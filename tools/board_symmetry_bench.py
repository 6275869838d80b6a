#!/usr/bin/env python3
"""Toot-and-otto 5x4 and 6x4 on BUCKETED, plain and with board_symmetry=1
(the left-right mirror, csrc/gm_sym.h), in one process on one GPU: solve ms
(gm_result's device time, median of argv[1] = 3 solves after one warm-up
solve), positions, edges and the plan's table, level and scratch bytes.  The
symmetric row carries its ratios to the plain row of the same run.  A record,
not a gate: one JSON line per row on stdout, and the table in
profiles/board_symmetry_bench.txt (argv[2]; DESIGN.md section 7b quotes it).
argv[3]: the boards' columns, comma separated (default 5,6)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import torch
    from gamesmanmpi_amd.games import GameSpec
    from gamesmanmpi_amd.solver import Solver
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 3
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "board_symmetry_bench.txt")
    cols = [int(c) for c in (sys.argv[3] if len(sys.argv) > 3 else "5,6").split(",")]
    rows = []
    for L in cols:
        plain = None
        for extra in ("", ",board_symmetry=1"):
            torch.cuda.empty_cache()
            s = Solver(GameSpec("toot_and_otto_bitstring", "length=%d,height=4%s" % (L, extra)), layout="bucketed")
            r = s.solve()  # warm-up
            ms = sorted(s.solve().ms_total for _ in range(reps))
            row = {"board": "%dx4" % L, "board_symmetry": int(bool(extra)), "root": r.root_line,
                   "solve_ms": round(ms[len(ms) // 2], 3), "solve_ms_all": [round(m, 3) for m in ms],
                   "positions": int(r.positions), "edges": int(r.edges),
                   "table_bytes": int(s.plan.table_bytes), "level_bytes": 8 * int(s.plan.level_capacity),
                   "scratch_bytes": int(s.plan.scratch_bytes)}
            if plain is None:
                plain = row
            else:
                assert row["root"] == plain["root"]
                for k in ("solve_ms", "positions", "edges"):
                    row[k + "_ratio"] = round(row[k] / plain[k], 4)
            print(json.dumps(row), flush=True)
            rows.append(row)
            del s
    fmt = "%-5s %-4s %10s %7s %14s %7s %14s %7s %15s %14s %10s"
    lines = [fmt % ("board", "sym", "solve ms", "ratio", "positions", "ratio", "edges", "ratio",
                    "table bytes", "level bytes", "scratch")]
    for r in rows:
        lines.append(fmt % (r["board"], r["board_symmetry"], "%.3f" % r["solve_ms"], r.get("solve_ms_ratio", ""),
                            r["positions"], r.get("positions_ratio", ""), r["edges"], r.get("edges_ratio", ""),
                            r["table_bytes"], r["level_bytes"], r["scratch_bytes"]))
    lines.append("(BUCKETED, %s; median of %d solves after a warm-up; ratios against the plain solve of the "
                 "same run; the plan's bounds are the plain board's, not shrunk for the symmetric solve)"
                 % (torch.cuda.get_device_name(0), reps))
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
