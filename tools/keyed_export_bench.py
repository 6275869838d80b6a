#!/usr/bin/env python3
"""Times gm_solver_export_keyed: othello 4x4 on BUCKETED and on HASHED, and
the largest toot-and-otto board asked for on BUCKETED (argv[2]: 4, 5 or 6
columns of height 4; default 5) -- the whole call, count, scan, scatter, sort
and pack, no copy to the host and no file.  On BUCKETED the side-by-side path
and the query path (GM_EXPORT_GENERIC) run in the same process.  Device time
between two events on the solver's stream, median of 3 after one warm-up
call.  Each row also gives the time a plain read of 12 B per position plus a
plain write of the file's bytes would take at the measured HBM rate, and the
call's ratio to it.  Then, on the last solver (toot 4x4 when that one holds
more than 8M positions), the bytes and the end-to-end time of solution.gmtk
(Solver.export_keyed_tablebase) against solution.npz
(solver_launcher.write_stats).  Prints one JSON line per table (DESIGN.md
section 7f records them)."""
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_TBPS = 6.29  # measured HBM bandwidth of the MI355X (a float4 copy; 8.0 TB/s is the spec)


def main():
    import numpy as np
    import torch
    from gamesmanmpi_amd import _lib, db, solver_launcher
    from gamesmanmpi_amd.games import GameSpec
    from gamesmanmpi_amd.solver import Solver
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 3
    cols = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    tables = (
        ("othello_bit_new", "length=4,height=4", "bucketed"),
        ("othello_bit_new", "length=4,height=4", "hashed"),
        ("toot_and_otto_bitstring", "length=%d,height=4" % cols, "bucketed"),
    )
    L = _lib.load()
    s = spec = r = None
    for game, params, layout in tables:
        del s
        torch.cuda.empty_cache()
        spec = GameSpec(game, params)
        s = Solver(spec, layout=layout)
        r = s.solve()
        ext = s.census(rem_bins=0, levels=False)["extremes"]
        npos = sum(e["count"] for e in ext)
        wb = db.tb_word_bytes(max(e["max_remoteness"] for e in ext))
        b = db.tk_default_bits(npos)
        stage = torch.empty(npos * 3 // 2 + 1, dtype=torch.int64, device=s.device)
        d = torch.empty((1 << b) + 1, dtype=torch.int64, device=s.device)
        keys = torch.empty(npos * 8, dtype=torch.uint8, device=s.device)
        words = torch.empty(max(16, npos * wb), dtype=torch.uint8, device=s.device)
        out = np.zeros(4, np.uint64)

        def run(how):
            _lib.check(L.gm_solver_export_keyed(s.handle, how, b, wb, stage.data_ptr(), d.data_ptr(),
                                                keys.data_ptr(), words.data_ptr(), npos, out.ctypes.data))
            assert int(out[0]) == npos

        def device_ms(how):
            run(how)  # warm-up
            ts = []
            for _ in range(reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                run(how)
                e1.record()
                e1.synchronize()
                ts.append(e0.elapsed_time(e1))
            ts.sort()
            return round(ts[len(ts) // 2], 3)

        run(_lib.GM_EXPORT_GENERIC)
        kb = int(out[1])
        file_bytes = db.tk_header(wb, kb, b, npos)[4]
        plain = (12 * npos + file_bytes) / (HBM_TBPS * 1e12) * 1e3
        row = {"game": game, "params": params, "layout": layout, "positions": npos, "bucket_bits": b,
               "largest_bucket": int(out[2]), "word_bytes": wb, "key_bytes": kb, "solve_ms": round(r.ms_total, 3),
               "file_bytes": file_bytes, "bytes_per_position": round(file_bytes / npos, 3),
               "plain_read_write_ms": round(plain, 4)}
        if layout == "bucketed":
            generic = [t.clone() for t in (d, keys[:npos * kb], words[:npos * wb])]
            run(0)
            row["direct_equals_generic"] = all(
                bool(torch.equal(x, y)) for x, y in zip(generic, (d, keys[:npos * kb], words[:npos * wb])))
            del generic
            row["direct_ms"] = device_ms(0)
            row["generic_ms"] = device_ms(_lib.GM_EXPORT_GENERIC)
            row["direct_ms_again"] = device_ms(0)  # (the order of the two is not what decides)
            row["direct_over_plain"] = round(row["direct_ms"] / plain, 1)
        else:
            row["generic_ms"] = device_ms(_lib.GM_EXPORT_GENERIC)
        row["generic_over_plain"] = round(row["generic_ms"] / plain, 1)
        print(json.dumps(row), flush=True)
        del stage, d, keys, words
    # the files, end to end, on one solver: the last one, or toot 4x4 when that
    # table's solution.npz would take minutes to write
    if r.positions > 8_000_000:
        del s
        torch.cuda.empty_cache()
        spec = GameSpec("toot_and_otto_bitstring", "length=4,height=4")
        s = Solver(spec, layout="bucketed")
        r = s.solve()
    with tempfile.TemporaryDirectory() as tmp:
        t0 = time.time()
        info = s.export_keyed_tablebase(os.path.join(tmp, "solution.gmtk"))
        t1 = time.time()
        solver_launcher.write_stats(tmp, 0, spec, s, r)
        t2 = time.time()
        npz = os.path.getsize(os.path.join(tmp, "stats", "0", "solution.npz"))
    print(json.dumps({"game": spec.name, "params": spec.params, "positions": info["positions"],
                      "gmtk_bytes": info["bytes"], "gmtk_write_s": round(t1 - t0, 3),
                      "npz_bytes": npz, "npz_write_s": round(t2 - t1, 3),
                      "gmtk_bytes_per_position": round(info["bytes"] / info["positions"], 3),
                      "npz_bytes_per_position": round(npz / info["positions"], 3)}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
