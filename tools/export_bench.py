#!/usr/bin/env python3
"""Times gm_solver_export on the bench table (sum_four_to_one,
heaps=31:31:31:31:31:31, PLANES) and on toot-and-otto 6x4 (RANKED): the whole
index space in one call -- bitmap, counts, scan and compaction, no copy to the
host and no file -- through the direct kernels and through the generic path,
in one run.  Device time between two events on the solver's stream, median of
3 after one warm-up call.  Then, on toot-and-otto 4x4, the bytes and the
end-to-end time of solution.gmtb (Solver.export_tablebase) against
solution.npz (solver_launcher.write_stats).  Prints one JSON line per table
(DESIGN.md section 7e records them)."""
import ctypes
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

TABLES = (
    ("sum_four_to_one", "heaps=31:31:31:31:31:31", "planes"),
    ("toot_and_otto_bitstring", "length=6,height=4", "ranked"),
)
HBM_TBPS = 6.29  # measured HBM bandwidth of the MI355X (a float4 copy; 8.0 TB/s is the spec)


def main():
    import numpy as np
    import torch
    from gamesmanmpi_amd import _lib, db, solver_launcher
    from gamesmanmpi_amd.games import GameSpec
    from gamesmanmpi_amd.solver import Solver
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 3
    L = _lib.load()
    for game, params, layout in TABLES:
        spec = GameSpec(game, params)
        s = Solver(spec, layout=layout)
        r = s.solve()
        space = spec.tb_index_space()
        wb = db.tb_word_bytes(max(e["max_remoteness"] for e in s.census(rem_bins=0, levels=False)["extremes"]))
        bits = torch.empty(space // 64, dtype=torch.int64, device=s.device)
        counts = torch.empty(space // 512, dtype=torch.int32, device=s.device)
        words = torch.empty(r.positions * wb, dtype=torch.uint8, device=s.device)
        n = ctypes.c_uint64()

        def run(how):
            _lib.check(L.gm_solver_export(s.handle, how, 0, space, wb, bits.data_ptr(), counts.data_ptr(),
                                          words.data_ptr(), r.positions, ctypes.byref(n)))
            assert n.value == r.positions

        def device_ms(how):
            run(how)  # warm-up
            ts = []
            for _ in range(reps):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                run(how)
                b.record()
                b.synchronize()
                ts.append(a.elapsed_time(b))
            ts.sort()
            return round(ts[len(ts) // 2], 3)

        run(0)
        direct = [t.clone() for t in (bits, counts, words)]
        run(_lib.GM_EXPORT_GENERIC)
        same = all(bool(torch.equal(a, b)) for a, b in zip(direct, (bits, counts, words)))
        del direct
        # the table's own bytes, read once at the achieved HBM rate: PLANES the words,
        # RANKED a byte per slot plus the reach bits
        table = r.positions * r.extra["word_bits"] // 8 if layout == "planes" else space + space // 8
        row = {"game": game, "params": params, "layout": layout, "positions": r.positions, "index_space": space,
               "word_bytes": wb, "solve_ms": round(r.ms_total, 3), "direct_equals_generic": same,
               "direct_ms": device_ms(0), "generic_ms": device_ms(_lib.GM_EXPORT_GENERIC),
               "table_bytes_read": table, "plain_read_ms": round(table / (HBM_TBPS * 1e12) * 1e3, 3),
               "tablebase_bytes": 64 + space // 8 + 8 * (space // 512 + 1) + r.positions * wb}
        row["direct_over_plain_read"] = round(row["direct_ms"] / row["plain_read_ms"], 2)
        row["generic_over_plain_read"] = round(row["generic_ms"] / row["plain_read_ms"], 2)
        row["bytes_per_position"] = round(row["tablebase_bytes"] / r.positions, 3)
        print(json.dumps(row), flush=True)
        del s, bits, counts, words
        torch.cuda.empty_cache()
    # the files, end to end, on toot 4x4
    spec = GameSpec("toot_and_otto_bitstring", "length=4,height=4")
    s = Solver(spec, layout="ranked")
    r = s.solve()
    with tempfile.TemporaryDirectory() as d:
        t0 = time.time()
        info = s.export_tablebase(os.path.join(d, "solution.gmtb"))
        t1 = time.time()
        solver_launcher.write_stats(d, 0, spec, s, r)
        t2 = time.time()
        npz = os.path.getsize(os.path.join(d, "stats", "0", "solution.npz"))
    print(json.dumps({"game": spec.name, "params": spec.params, "positions": r.positions,
                      "gmtb_bytes": info["bytes"], "gmtb_write_s": round(t1 - t0, 3),
                      "npz_bytes": npz, "npz_write_s": round(t2 - t1, 3),
                      "gmtb_bytes_per_position": round(info["bytes"] / r.positions, 3),
                      "npz_bytes_per_position": round(npz / r.positions, 3)}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
