#!/usr/bin/env python3
"""Times a saved tablebase opened on the GPU (Solver.open_tablebase, DESIGN.md
section 7j) against the solver that wrote it, in one process: toot-and-otto
5x4 as solution.gmtk and as solution.gmtb, and the bench's PLANES table
(sum_four_to_one heaps=31:31:31:31:31:31) as solution.gmtb.  Per file:

  open_s       Solver.open_tablebase end to end (file -> pinned chunk -> device,
               header check, the validation kernel), wall clock
  query        2^24 random reached keys, already on the device, through
               gm_solver_query: the opened image against the solver's own
               table, device ms between two events and keys per second
  audit        gm_solver_audit on both, device ms

Median of 3 after one warm-up call (argv[1]: the repetitions; argv[2]: a
smaller toot width, 3 or 4, for a quick run).  A record, not a gate: one JSON
line per file."""
import ctypes
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

NKEYS = 1 << 24


def main():
    import numpy as np
    import torch
    from gamesmanmpi_amd import _lib
    from gamesmanmpi_amd.games import GameSpec
    from gamesmanmpi_amd.solver import Solver
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 3
    cols = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    toot = ("toot_and_otto_bitstring", "length=%d,height=4" % cols)
    tables = ((toot, "auto", "gmtk"), (toot, "auto", "gmtb"),
              (("sum_four_to_one", "heaps=31:31:31:31:31:31"), "planes", "gmtb"))
    L = _lib.load()

    def device_ms(call):
        call()  # warm-up
        ts = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call()
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1))
        ts.sort()
        return ts[len(ts) // 2]

    s = last = None
    for (game, params), layout, fmt in tables:
        if (game, params, layout) != last:
            del s
            torch.cuda.empty_cache()
            spec = GameSpec(game, params)
            s = Solver(spec, layout=layout)
            r = s.solve()
            last = (game, params, layout)
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "solution." + fmt)
            t0 = time.time()
            info = s.export_tablebase(path) if fmt == "gmtb" else s.export_keyed_tablebase(path)
            write_s = time.time() - t0
            opens = []
            t = None
            for _ in range(reps + 1):  # (the first: warm-up, the page cache included)
                del t
                torch.cuda.empty_cache()
                t0 = time.time()
                t = Solver.open_tablebase(spec, path)
                opens.append(time.time() - t0)
            opens = sorted(opens[1:])
        # 2^24 random reached keys, on the device
        n = ctypes.c_uint64()
        pos = torch.empty(r.positions, dtype=torch.int64, device=s.device)
        _lib.check(L.gm_solver_positions(s.handle, pos.data_ptr(), r.positions, ctypes.byref(n)))
        assert n.value == r.positions
        g = torch.Generator(device=s.device)
        g.manual_seed(1)
        keys = pos[torch.randint(0, pos.numel(), (NKEYS,), generator=g, device=s.device)].contiguous()
        del pos
        out = {}
        for name, x in (("solver", s), ("file", t)):
            wd = torch.empty(NKEYS, dtype=torch.int32, device=s.device)
            bad = torch.empty(64, dtype=torch.int64, device=s.device)
            acc = np.zeros(4, np.uint64)
            q = device_ms(lambda: _lib.check(L.gm_solver_query(x.handle, keys.data_ptr(), NKEYS, wd.data_ptr())))
            a = device_ms(lambda: _lib.check(L.gm_solver_audit(x.handle, bad.data_ptr(), 64, acc.ctypes.data)))
            assert int(acc[0]) == r.positions and int(acc[2]) == 0, acc
            out[name] = (q, a, wd)
        assert bool(torch.equal(out["solver"][2], out["file"][2]))
        row = {"game": game, "params": params, "layout": r.extra["layout"], "format": fmt,
               "positions": r.positions, "file_bytes": info["bytes"], "word_bytes": info["word_bytes"],
               "key_bytes": info.get("key_bytes"), "write_s": round(write_s, 3),
               "open_s": round(opens[len(opens) // 2], 3),
               "open_gb_per_s": round(info["bytes"] / opens[len(opens) // 2] / 1e9, 3)}
        for name in ("solver", "file"):
            q, a, _ = out[name]
            row["query_ms_" + name] = round(q, 3)
            row["query_mkeys_per_s_" + name] = round(NKEYS / q / 1e3, 1)
            row["audit_ms_" + name] = round(a, 3)
        row["query_file_over_solver"] = round(out["file"][0] / out["solver"][0], 2)
        row["audit_file_over_solver"] = round(out["file"][1] / out["solver"][1], 2)
        print(json.dumps(row), flush=True)
        del t, keys, out
    return 0


if __name__ == "__main__":
    sys.exit(main())
