#!/usr/bin/env python3
"""What gm_graph_solve_loopy costs, on one GPU.

(a) The 600,000-position graph without cycles of tests/test_gpu_graph_fuzz.py
    through gm_graph_solve and gm_graph_solve_loopy, alternating in one
    process; with --parent-lib PATH (a libgamesman_hip.so built from the
    parent commit) that library's gm_graph_solve takes turns with them.
(b) A random graph of 2^20 positions with cycles everywhere (out-degree
    1 .. 4, children uniform over all positions, each primitive code at
    0.05): time, rounds and the positions by rule.

Times are the library's own ms_total (host clock from the first memset to
the last synchronise).  Output: profiles/graph_loopy_bench.txt.
"""
import argparse
import ctypes
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


class Graph:
    """A CSR graph on the device and the buffers of a solve."""

    def __init__(self, prim, offsets, children):
        import numpy as np
        import torch
        from gamesmanmpi_amd.generic import loopy_scratch_bytes
        dev = torch.device("cuda")
        self.n = len(prim)
        self.prim = torch.from_numpy(prim).to(dev)
        self.offsets = torch.from_numpy(offsets).to(dev)
        self.children = torch.from_numpy(np.ascontiguousarray(children).view(np.int32)).to(dev)
        self.words = torch.empty(self.n, dtype=torch.int32, device=dev)
        self.scratch = torch.zeros(loopy_scratch_bytes(self.n), dtype=torch.uint8, device=dev)
        self.stream = torch.cuda.current_stream(dev).cuda_stream

    def solve(self, fn, loopy):
        """(gm_result, counts or None, words copy) of one call of fn."""
        from gamesmanmpi_amd import _lib
        r = _lib.gm_result()
        args = [self.prim.data_ptr(), self.offsets.data_ptr(), self.children.data_ptr(), self.n, 0,
                self.words.data_ptr(), self.scratch.data_ptr(), self.stream, ctypes.byref(r)]
        counts = (ctypes.c_uint64 * 4)() if loopy else None
        rc = fn(*(args + [counts] if loopy else args))
        if rc:
            raise RuntimeError("solve failed: %d" % rc)
        return r, None if counts is None else [int(c) for c in counts], self.words.clone()


def parent_entry(path):
    from gamesmanmpi_amd import _lib
    c = ctypes
    fn = c.CDLL(path).gm_graph_solve
    fn.argtypes = [c.c_void_p, c.c_void_p, c.c_void_p, c.c_uint64, c.c_uint64, c.c_void_p, c.c_void_p, c.c_void_p,
                   c.POINTER(_lib.gm_result)]
    fn.restype = c.c_int
    return fn


def line(name, ms, rounds):
    ms = sorted(ms)
    return "%-34s min %8.3f  median %8.3f  max %8.3f ms   rounds %s" % (
        name, ms[0], statistics.median(ms), ms[-1], rounds)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", help="libgamesman_hip.so of the parent commit")
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "graph_loopy_bench.txt"))
    a = ap.parse_args()
    import numpy as np
    import torch
    from gamesmanmpi_amd import _lib
    from test_gpu_graph_fuzz import random_dag
    lib = _lib.load()
    out = ["graph_loopy_bench: %s, %d timed calls per entry, alternating, after one warm-up each"
           % (torch.cuda.get_device_name(0), a.rounds)]

    rng = np.random.default_rng(20)
    g = random_dag(rng, 600_000, mean_degree=4, leaves=0.25, window=1 << 13).graph(rng)
    dag = Graph(g.prim, g.offsets, g.children)
    entries = [("gm_graph_solve", lib.gm_graph_solve, False), ("gm_graph_solve_loopy", lib.gm_graph_solve_loopy, True)]
    if a.parent_lib:
        entries.append(("gm_graph_solve (parent commit)", parent_entry(a.parent_lib), False))
    ms = {name: [] for name, _, _ in entries}
    rounds, ref = {}, None
    for it in range(a.rounds + 1):
        for name, fn, loopy in entries:
            r, counts, words = dag.solve(fn, loopy)
            if ref is None:
                ref = words
            assert torch.equal(words, ref), name
            assert counts is None or counts == [dag.n, 0, 0, 0]
            if it:
                ms[name].append(r.ms_total)
                rounds.setdefault(name, set()).add(int(r.levels))
    out.append("(a) graph without cycles: %d positions, %d edges" % (dag.n, len(g.children)))
    out += ["    " + line(name, ms[name], sorted(rounds[name])) for name, _, _ in entries]

    n = 1 << 20
    rng = np.random.default_rng(7)
    u = rng.random(n)
    prim = np.full(n, 4, np.uint8)
    for code in range(4):
        prim[(u >= code * 0.05) & (u < (code + 1) * 0.05)] = code
    deg = np.where(prim == 4, rng.integers(1, 5, n), 0)
    offsets = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    children = rng.integers(0, n, int(offsets[-1])).astype(np.uint32)
    loop = Graph(prim, offsets, children)
    t, lv = [], set()
    for it in range(a.rounds + 1):
        r, counts, words = loop.solve(lib.gm_graph_solve_loopy, True)
        if it:
            t.append(r.ms_total)
            lv.add(int(r.levels))
    val = words.cpu().numpy().view(np.uint32)
    out.append("(b) random graph with cycles: %d positions, %d edges" % (n, len(children)))
    out.append("    " + line("gm_graph_solve_loopy", t, sorted(lv)))
    out.append("    founded %d  attractor %d  tie %d  draw %d;  WIN %d LOSS %d TIE %d DRAW %d;  largest remoteness %d"
               % (tuple(counts) + tuple(int(((val & 3) == v).sum()) for v in range(4)) + (int((val >> 2).max()),)))
    # rounds per phase: phase A alone is what gm_graph_solve runs before it gives up
    r0 = _lib.gm_result()
    lib.gm_graph_solve(loop.prim.data_ptr(), loop.offsets.data_ptr(), loop.children.data_ptr(), n, 0,
                       loop.words.data_ptr(), loop.scratch.data_ptr(), loop.stream, ctypes.byref(r0))
    # the same graph with its TIE primitives turned into DRAW primitives has the same WIN and LOSS
    # words, so the same rounds of A and B, and one round of C (nothing to ignore, nothing resolves)
    prim2 = prim.copy()
    prim2[prim == 2] = 3
    r2, _, _ = Graph(prim2, offsets, children).solve(lib.gm_graph_solve_loopy, True)
    b = int(r2.levels) - int(r0.levels) - 1
    out.append("    rounds: phase A %d (gm_graph_solve stops there: %d positions never resolve), phase B %d, phase C %d"
               % (r0.levels, n - r0.positions, b, max(lv) - r0.levels - b))
    text = "\n".join(out)
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
