#!/usr/bin/env python3
"""Times Solver.census() on the bench table (sum_four_to_one,
heaps=31:31:31:31:31:31, PLANES) and on toot-and-otto 6x4 (RANKED): the
direct kernel and the generic path (enumerator + query path), each with and
without the witness pass, next to gm_solver_checksum on the same solver, all in
one run.  Device time between two events on the solver's stream, median of 3
(after one warm-up call each).  Prints one JSON line per table (DESIGN.md
section 7d records them)."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

TABLES = (
    ("sum_four_to_one", "heaps=31:31:31:31:31:31", "planes"),
    ("toot_and_otto_bitstring", "length=6,height=4", "ranked"),
)
HBM_TBPS = 6.29  # measured HBM bandwidth of the MI355X (a float4 copy; 8.0 TB/s is the spec)


def device_ms(torch, fn, reps):
    fn()  # warm-up
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return round(ts[len(ts) // 2], 3)


def main():
    import numpy as np
    import torch
    from gamesmanmpi_amd.games import GameSpec
    from gamesmanmpi_amd.solver import Solver
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 3
    for game, params, layout in TABLES:
        s = Solver(GameSpec(game, params), layout=layout)
        r = s.solve()
        direct, generic = s.census(), s.census(generic=True)
        same = (np.array_equal(direct["by_remoteness"], generic["by_remoteness"])
                and np.array_equal(direct["by_level"], generic["by_level"])
                and direct["extremes"] == generic["extremes"])
        row = {"game": game, "params": params, "layout": layout, "positions": r.positions,
               "solve_ms": round(r.ms_total, 3), "direct_equals_generic": same,
               "census_positions": int(direct["by_remoteness"].sum()),
               "extremes": direct["extremes"],
               "direct_ms": device_ms(torch, lambda: s.census(), reps),
               "direct_no_extremes_ms": device_ms(torch, lambda: s.census(extremes=False), reps),
               "generic_ms": device_ms(torch, lambda: s.census(generic=True), reps),
               "generic_no_extremes_ms": device_ms(torch, lambda: s.census(generic=True, extremes=False), reps),
               "checksum_ms": device_ms(torch, lambda: s.checksum(), reps)}
        if layout == "planes":  # the words alone, read once at the achieved HBM rate
            words = r.positions * r.extra["word_bits"] // 8
            row["table_word_bytes"] = words
            row["plain_read_ms"] = round(words / (HBM_TBPS * 1e12) * 1e3, 3)
            row["direct_no_extremes_over_plain_read"] = round(row["direct_no_extremes_ms"] / row["plain_read_ms"], 2)
        print(json.dumps(row), flush=True)
        del s
        torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
