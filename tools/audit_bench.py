#!/usr/bin/env python3
"""Times Solver.audit() -- every stored word re-derived from its children's
words through the query path -- on the bench table (sum_four_to_one,
heaps=31:31:31:31:31:31, PLANES) and on toot-and-otto 6x4 (RANKED), next to
the solve itself.  Prints one JSON line per table (DESIGN.md records them)."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

TABLES = (
    ("sum_four_to_one", "heaps=31:31:31:31:31:31", "planes"),
    ("toot_and_otto_bitstring", "length=6,height=4", "ranked"),
)


def main():
    import torch
    from gamesmanmpi_amd.games import GameSpec
    from gamesmanmpi_amd.solver import Solver
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    for game, params, layout in TABLES:
        s = Solver(GameSpec(game, params), layout=layout)
        r = s.solve()
        a = s.audit()  # warm-up, and the result that is reported
        ts = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            s.audit()
            ts.append((time.perf_counter() - t0) * 1e3)
        ts.sort()
        med = ts[len(ts) // 2]
        print(json.dumps({"game": game, "params": params, "layout": layout,
                          "positions": a["positions"], "edges": a["edges"],
                          "mismatches": a["mismatches"],
                          "solve_ms": round(r.ms_total, 3),
                          "audit_ms_min": round(ts[0], 3), "audit_ms_median": round(med, 3),
                          "audit_ms_max": round(ts[-1], 3),
                          "positions_per_s": round(a["positions"] / (med * 1e-3)),
                          "child_words_per_s": round(a["edges"] / (med * 1e-3))}), flush=True)
        del s
        torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
