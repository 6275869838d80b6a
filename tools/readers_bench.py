#!/usr/bin/env python3
"""Times the three table readers -- gm_solver_checksum, gm_solver_positions
and gm_solver_query of every position -- on one solved table per layout: at
the benchmark's own sizes where the layout has one (PLANES: sum_four_to_one
heaps=31:31:31:31:31:31; RANKED and BUCKETED: toot-and-otto 6x4), HASHED and
DENSE on smaller tables.  The C calls themselves, on buffers allocated once:
wall time of a call (each one ends with a stream synchronisation), median of
`reps` calls after one warm-up call.  Prints one JSON line per table.

  python tools/readers_bench.py [reps]

GM_LIBPATH selects another in-tree build of the library (gamesmanmpi_amd/_lib.py):
run it on two builds in one session to compare them, and twice on one build
for the run-to-run spread (profiles/readers_refactor.txt)."""
import ctypes
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

TABLES = (
    ("sum_four_to_one", "heaps=31:31:31:31:31:31", "planes"),
    ("toot_and_otto_bitstring", "length=6,height=4", "ranked"),
    ("toot_and_otto_bitstring", "length=6,height=4", "bucketed"),
    ("toot_and_otto_bitstring", "length=4,height=4", "hashed"),
    ("sum_four_to_one", "heaps=31:31:31:31:31", "dense"),
)


def wall_ms(torch, fn, reps):
    fn()  # warm-up
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    ts.sort()
    return round(ts[len(ts) // 2], 3), round(ts[0], 3), round(ts[-1], 3)


def main():
    import numpy as np
    import torch
    from gamesmanmpi_amd import _lib
    from gamesmanmpi_amd.games import GameSpec
    from gamesmanmpi_amd.solver import Solver
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    L = _lib.load()
    for game, params, layout in TABLES:
        s = Solver(GameSpec(game, params), layout=layout)
        r = s.solve()
        n = r.positions
        keys = torch.empty(n, dtype=torch.int64, device=s.device)
        words = torch.empty(n, dtype=torch.int32, device=s.device)
        ck = np.zeros(6, np.uint64)
        got = ctypes.c_uint64()
        with torch.cuda.device(s.device):
            row = {"game": game, "params": params, "layout": r.extra["layout"], "positions": n,
                   "library": os.path.relpath(_lib.LIBPATH), "reps": reps, "ms": "median, min, max",
                   "checksum_ms": wall_ms(torch, lambda: _lib.check(L.gm_solver_checksum(s._h, ck.ctypes.data)), reps),
                   "positions_ms": wall_ms(torch, lambda: _lib.check(L.gm_solver_positions(
                       s._h, keys.data_ptr(), n, ctypes.byref(got))), reps),
                   "query_ms": wall_ms(torch, lambda: _lib.check(L.gm_solver_query(
                       s._h, keys.data_ptr(), n, words.data_ptr())), reps)}
        # what was timed read the table: every position listed, found, and counted
        row["ok"] = bool(got.value == n == int(ck[1]) and int((words == -1).sum()) == 0)
        row["checksum"] = "%016x" % int(ck[0])
        print(json.dumps(row), flush=True)
        del s, keys, words
        torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
