"""Single-GPU solve driver: allocates HBM buffers with PyTorch-ROCm, hands
their addresses to libgamesman_hip.so and reads results back.

Stands in for one rank of the reference's Process (src/process.py:10-267):
``Solver.solve()`` is Process.run until the root is resolved, and
``Solver.query()`` reads the table that replaces the resolved/remote
CacheDicts (src/cache_dict.py).  No CPU fallback exists: without a gfx950
device the library returns GM_ENOGPU and this raises.
"""
import ctypes
from dataclasses import dataclass, field

import numpy as np

from . import _lib
from .games import GameSpec

NAMES = ("WIN", "LOSS", "TIE", "DRAW")


@dataclass
class SolveResult:
    root_value: int
    root_remoteness: int
    positions: int
    edges: int
    primitives: int
    levels: int
    max_level_width: int
    ms_total: float
    ms_forward: float
    ms_backward: float
    ms_expand_kernels: float = 0.0
    ms_resolve_kernels: float = 0.0
    n_expand_launches: int = 0
    n_resolve_launches: int = 0
    extra: dict = field(default_factory=dict)

    @property
    def root_line(self):
        """Exactly what src/process.py:47-52 prints."""
        return "%s in %d moves" % (NAMES[self.root_value],
                                   self.root_remoteness)


class Solver:
    """Owns the device buffers of one game's solve on one GPU."""

    def __init__(self, spec, positions=0, device=None, kernel_timing=False,
                 layout="auto", max_table_bytes=0, rank=0, world=1,
                 stream=None, flags=0, staging_records=0):
        """layout: "auto" (planes, else the level-major dense table, when
        the descriptor supports it and the table fits max_table_bytes; the
        ranked table for toot-and-otto; else bucketed levels when every move
        advances one level; else the keyed hash table), "planes" (sum games
        whose first two heaps hold 32 values: natural rank order,
        gm_plane.h), "dense" (the level-major dense table), "ranked"
        (positions at computed indices: toot-and-otto, gm_ranked.h, which
        "auto" picks too, and connect four, gm_ranked_connect.h, on request
        only -- boards up to 8 columns, 7 rows and 2^36 slots, 6x5 included,
        one GPU),
        "bucketed" or "hashed" (the open-addressing hash table).
        flags: kernel-family flags (_lib.GM_F_WORDS32 / GM_F_RESOLVE_SCALAR /
        GM_F_SHARD_INORDER, A/B runs), fixed for this solver's lifetime.
        rank/world > 1: this object is one shard of a dense / planes multi-
        GPU solve (gamesmanmpi_amd.dist), or with layout="bucketed" /
        "hashed" one md5 shard of a keyed solve (gamesmanmpi_amd.keyed;
        `positions` is then this shard's bound); stream: a torch stream to
        run on.  staging_records=N (bucketed layouts, one GPU or md5 shard):
        the buffers keep the plan's sizes, but the library is told a table
        that ends where N staging records per level end (claimed_table_bytes),
        so the solve runs with that staging capacity and never regrows; the
        bytes past the claimed end are the caller's (capacity tests keep a
        canary there)."""
        import torch
        if not torch.cuda.is_available():
            raise RuntimeError("gamesmanmpi_amd needs a ROCm GPU (gfx950); "
                               "no device is visible")
        self.torch = torch
        self.spec = spec if isinstance(spec, GameSpec) else GameSpec(*spec)
        self.device = torch.device(device if device is not None else "cuda")
        self.kernel_timing = kernel_timing
        if layout not in ("auto", "planes", "dense", "hashed", "bucketed", "ranked"):
            raise ValueError("layout must be auto, planes, dense, ranked, bucketed or hashed")
        self.layout = layout
        if layout == "ranked" and self.spec.board_symmetric:
            raise _lib.GmError(_lib.GM_EINVAL, "board_symmetry=1 has no ranked layout: the RANKED index "
                                               "has no representative form (use bucketed or hashed)")
        self.max_table_bytes = int(max_table_bytes)
        self.rank, self.world = int(rank), int(world)
        self.stream = stream
        if flags & ~_lib.KERNEL_FLAGS:
            raise ValueError("flags: kernel-family flags only (%#x)" % _lib.KERNEL_FLAGS)
        self.flags = int(flags)
        self.staging_records = int(staging_records)
        self.claimed_table_bytes = None
        self.positions_hint = int(positions or self.spec.positions_bound)
        # the layout planned: `layout`, except that "auto" falls back to the
        # hashed table when a bucketed plan hits a layout limit (solve())
        self._planned_layout = layout
        self._h = None
        self._bufs = None
        self._alloc(self.positions_hint)

    def _alloc(self, positions):
        torch = self.torch
        L = _lib.load()
        self._free()
        plan = _lib.gm_plan_t()
        flags = self.flags | {"hashed": _lib.GM_F_FORCE_HASHED | _lib.GM_F_HASH_TABLE,
                              "bucketed": _lib.GM_F_FORCE_HASHED,
                              "dense": _lib.GM_F_LEVEL_MAJOR,
                              "ranked": _lib.GM_F_RANKED}.get(self._planned_layout, 0)
        if self.world > 1 and self.layout in ("bucketed", "ranked"):
            # an md5 shard of bucketed levels (`positions` bounds this
            # shard), or of the RANKED index space (toot-and-otto)
            if self.layout == "ranked":
                flags |= _lib.GM_F_RANKED_SHARD
            _lib.check(L.gm_plan_keyed_shard(self.spec.id, self.rank,
                                             self.world, int(positions), flags,
                                             self.max_table_bytes,
                                             ctypes.byref(plan)))
        elif self.world > 1 and self.layout != "hashed":
            _lib.check(L.gm_plan_shard(self.spec.id, self.rank, self.world,
                                       flags, self.max_table_bytes,
                                       ctypes.byref(plan)))
        else:
            _lib.check(L.gm_plan(self.spec.id, int(positions), flags,
                                 self.max_table_bytes, ctypes.byref(plan)))
        if self.layout == "dense" and plan.mode != _lib.GM_MODE_DENSE:
            raise ValueError("%r has no dense layout (or it does not fit)"
                             % (self.spec,))
        if self.layout == "planes" and plan.mode != _lib.GM_MODE_PLANES:
            raise ValueError("%r has no planes layout (heaps 0 and 1 of 32 "
                             "values), or it does not fit" % (self.spec,))
        if self.layout == "ranked" and plan.mode != _lib.GM_MODE_RANKED:
            raise ValueError("%r has no ranked layout (toot-and-otto and connect four "
                             "boards), or it does not fit" % (self.spec,))
        if self.layout == "bucketed" and plan.mode != _lib.GM_MODE_BUCKETED:
            raise ValueError("%r: bucketed levels need every move to advance "
                             "one level" % (self.spec,))
        with torch.cuda.device(self.device):
            table = torch.empty(plan.table_bytes, dtype=torch.uint8,
                                device=self.device)
            levels = torch.empty(max(1, plan.level_capacity),
                                 dtype=torch.int64, device=self.device)
            scratch = torch.empty(plan.scratch_bytes, dtype=torch.uint8,
                                  device=self.device)
            stream = self.stream or torch.cuda.current_stream(self.device)
        self._tensors = (table, levels, scratch)
        b = _lib.gm_buffers()
        b.table = table.data_ptr()
        b.table_slots = plan.table_slots
        b.levels = levels.data_ptr()
        b.level_capacity = plan.level_capacity
        b.scratch = scratch.data_ptr()
        b.scratch_bytes = plan.scratch_bytes
        b.stream = stream.cuda_stream
        b.flags = flags | (_lib.GM_F_KERNEL_TIMING if self.kernel_timing else 0)
        b.mode = plan.mode
        b.table_bytes = plan.table_bytes
        if self.staging_records:
            if plan.mode != _lib.GM_MODE_BUCKETED:
                raise ValueError("staging_records applies to bucketed layouts only")
            # words, in-edges (a second set on md5 shards) and 24 B (48 B with
            # the exchange buffers) per staging record: 4 level_capacity +
            # K table_slots + R N with K, R = 6, 24 (12, 48), each array
            # padded to 8 bytes as bk_setup carves them, so its Emax == N
            sets, r = (1, 24) if self.world == 1 else (2, 48)
            slots = int(plan.table_slots)
            b.table_bytes = ((4 * int(plan.level_capacity) + 7 & ~7)
                             + sets * (4 * slots + (2 * slots + 7 & ~7))
                             + r * self.staging_records)
            if b.table_bytes > plan.table_bytes:
                raise ValueError("staging_records=%d exceeds the plan's table"
                                 % self.staging_records)
        self.claimed_table_bytes = int(b.table_bytes)
        self._bufs = b
        self._cflags = flags  # the flags the solver was created with (layout bits included)
        self.plan = plan
        h = ctypes.c_void_p()
        _lib.check(L.gm_solver_create_shard(self.spec.id, self.rank,
                                            self.world, ctypes.byref(b),
                                            ctypes.byref(h)))
        self._h = h

    def _free(self):
        if self._h is not None:
            _lib.load().gm_solver_destroy(self._h)
            self._h = None
        self._tensors = None

    def __del__(self):
        try:
            self._free()
        except Exception:  # noqa: BLE001 -- interpreter teardown
            pass

    @property
    def handle(self):
        return self._h

    def shard_stats(self):
        """md5 shards of the RANKED layout: (slots this shard resolved in its
        last solve, reached positions its md5 owner rule gives it)."""
        out = (ctypes.c_uint64 * 2)()
        _lib.check(_lib.load().gm_rk_shard_stats(self._h, out))
        return int(out[0]), int(out[1])

    def set_kernel_timing(self, on):
        """Time every kernel launch with HIP events (on the solve stream)."""
        self.kernel_timing = bool(on)
        _lib.check(_lib.load().gm_solver_set_flags(
            self._h, self._cflags | (_lib.GM_F_KERNEL_TIMING if on else 0)))

    def solve(self, max_retries=4):
        """Full solve from the root; grows the buffers on GM_EFULL."""
        L = _lib.load()
        r = _lib.gm_result()
        if self.world > 1 or getattr(self, "staging_records", 0):
            max_retries = 0  # shard tables are sized exactly; a chosen capacity stays
        attempt = 0
        while True:
            try:
                with self.torch.cuda.device(self.device):
                    _lib.check(L.gm_solver_solve(self._h, ctypes.byref(r)))
                break
            except _lib.TableFull:
                if attempt == max_retries:
                    raise
                attempt += 1
                self.positions_hint *= 2
                self._alloc(self.positions_hint)
            except _lib.LayoutLimit:
                # a bucketed level past 2^29 positions or a fine bucket past
                # its LDS capacity: "auto" may use the hashed table instead
                # (once); an explicit layout keeps the error
                if (self.layout != "auto" or self._planned_layout != "auto" or self.world > 1
                        or int(self.plan.mode) != _lib.GM_MODE_BUCKETED):
                    raise
                self._planned_layout = "hashed"
                self._alloc(self.positions_hint)
        return self._result(r)

    # -- queued solves (one-table PLANES) ------------------------------------
    def solve_async(self):
        """Enqueue a full solve on the solver's stream and return its ticket
        without waiting (gm_solver_solve_async; one-table PLANES solvers).
        Solves queued back to back run back to back on the GPU; collect()
        each one, in ticket order (at most 8 outstanding)."""
        L = _lib.load()
        t = ctypes.c_uint64()
        with self.torch.cuda.device(self.device):
            _lib.check(L.gm_solver_solve_async(self._h, ctypes.byref(t)))
        return int(t.value)

    def collect(self, ticket):
        """Wait for queued solve `ticket`; its SolveResult (ms_total is the
        solve's device span)."""
        L = _lib.load()
        r = _lib.gm_result()
        with self.torch.cuda.device(self.device):
            _lib.check(L.gm_solver_collect(self._h, int(ticket), ctypes.byref(r)))
        return self._result(r)

    # -- stop / resume (checkpoints: gamesmanmpi_amd.checkpoint) ------------
    @property
    def steps(self):
        """Steps of a full solve (gm_solver_set_steps): forward levels
        0..T-1, then backward levels T-1..0."""
        return 2 * int(self.plan.max_levels)

    def solve_steps(self, first=0, stop=0):
        """Run steps [first, stop) of the solve (stop 0 = to the end).
        Returns the SolveResult when the solve completed, None when it
        stopped early -- the state then stays in this solver's buffers
        (save it with checkpoint.save, or continue with first=stop).  No
        buffer regrowth: a table that fills raises TableFull."""
        L = _lib.load()
        _lib.check(L.gm_solver_set_steps(self._h, int(first), int(stop)))
        r = _lib.gm_result()
        with self.torch.cuda.device(self.device):
            rc = L.gm_solver_solve(self._h, ctypes.byref(r))
        if rc == _lib.GM_PARTIAL:
            return None
        _lib.check(rc)
        return self._result(r)

    @property
    def buffers(self):
        """(table, level store, scratch) device tensors (uint8 / int64 /
        uint8): everything a stopped solve leaves behind."""
        return self._tensors

    def _result(self, r):
        return SolveResult(
            root_value=r.root_value, root_remoteness=r.root_remoteness,
            positions=r.positions, edges=r.edges, primitives=r.primitives,
            levels=r.levels, max_level_width=r.max_level_width,
            ms_total=r.ms_total, ms_forward=r.ms_forward,
            ms_backward=r.ms_backward,
            ms_expand_kernels=r.ms_expand_kernels,
            ms_resolve_kernels=r.ms_resolve_kernels,
            n_expand_launches=r.n_expand_launches,
            n_resolve_launches=r.n_resolve_launches,
            extra={"layout": _lib.MODE_NAMES[self.plan.mode],
                   "word_bits": r.word_bits,
                   "resolve_kernel": _lib.RESOLVE_KERNELS.get(r.kernels & 0xFFFF),
                   "pull_kernel": _lib.PULL_KERNELS.get(r.kernels >> 16),
                   "table_bytes": self.plan.table_bytes})

    # -- reading the table -------------------------------------------------
    def query(self, keys):
        """Words (value | remoteness << 2; GM_NO_WORD if unreachable) of
        `keys` (numpy uint64 array)."""
        torch = self.torch
        keys = np.ascontiguousarray(keys, dtype=np.uint64)
        if len(keys) == 0:
            return np.zeros(0, np.uint32)
        kd = torch.from_numpy(keys.view(np.int64)).to(self.device)
        wd = torch.empty(len(keys), dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(_lib.load().gm_solver_query(
                self._h, kd.data_ptr(), len(keys), wd.data_ptr()))
        return wd.cpu().numpy().view(np.uint32)

    def positions(self):
        """Every reachable key (numpy uint64, level order)."""
        torch = self.torch
        n = ctypes.c_uint64()
        L = _lib.load()
        rc = L.gm_solver_positions(self._h, None, 0, ctypes.byref(n))
        if rc not in (0, _lib.GM_EFULL):
            _lib.check(rc)
        out = torch.empty(max(1, n.value), dtype=torch.int64,
                          device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(L.gm_solver_positions(self._h, out.data_ptr(),
                                             n.value, ctypes.byref(n)))
        return out[:n.value].cpu().numpy().view(np.uint64)

    def checksum(self):
        """Whole-solve fingerprint (gm_solver_checksum): dict with the
        order-independent checksum of every reachable position's
        (canonical bytes, value, remoteness), the position count and the
        W/L/T/D histogram."""
        out = np.zeros(6, np.uint64)
        with self.torch.cuda.device(self.device):
            _lib.check(_lib.load().gm_solver_checksum(self._h,
                                                      out.ctypes.data))
        v = [int(x) for x in out]
        return {"checksum": "%016x" % v[0], "positions": v[1], "win": v[2],
                "loss": v[3], "tie": v[4], "draw": v[5]}

    # -- move analysis and the whole-table audit ----------------------------
    def moves(self, keys):
        """(children u64[n, GM_MAXCHILD], words u32[n, GM_MAXCHILD],
        nchild u8[n], best i8[n]) of `keys` (gm_solver_moves): each key's
        children in gen_moves() order with their words (GM_EMPTY_KEY /
        GM_NO_WORD in unused slots) and the index of the best move; a
        primitive or unreachable key has nchild 0 and best -1.  On a
        symmetric table (symmetry=1 / board_symmetry=1) the children are
        reported as the descriptor emits them: as orbit representatives, of
        which a parent may list the same one more than once."""
        torch = self.torch
        keys = np.ascontiguousarray(keys, dtype=np.uint64)
        n, m = len(keys), _lib.GM_MAXCHILD
        if n == 0:
            return (np.zeros((0, m), np.uint64), np.zeros((0, m), np.uint32),
                    np.zeros(0, np.uint8), np.zeros(0, np.int8))
        kd = torch.from_numpy(keys.view(np.int64)).to(self.device)
        cd = torch.empty((n, m), dtype=torch.int64, device=self.device)
        wd = torch.empty((n, m), dtype=torch.int32, device=self.device)
        nd = torch.empty(n, dtype=torch.uint8, device=self.device)
        bd = torch.empty(n, dtype=torch.int8, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(_lib.load().gm_solver_moves(
                self._h, kd.data_ptr(), n, cd.data_ptr(), wd.data_ptr(),
                nd.data_ptr(), bd.data_ptr()))
        return (cd.cpu().numpy().view(np.uint64), wd.cpu().numpy().view(np.uint32),
                nd.cpu().numpy(), bd.cpu().numpy())

    def best_line(self, key=None, cap=None):
        """(keys u64, values u8, remoteness u32) of the optimal line from
        `key` (default: the root) to a primitive position, one kernel launch
        (gm_solver_line); at most `cap` entries (default: one per level).
        On a symmetric table the line runs through orbit representatives, as
        `moves` reports them."""
        torch = self.torch
        if key is None:
            key = self.spec.root_key
        cap = int(self.plan.max_levels) + 1 if cap is None else int(cap)
        kd = torch.empty(max(1, cap), dtype=torch.int64, device=self.device)
        wd = torch.empty(max(1, cap), dtype=torch.int32, device=self.device)
        n = ctypes.c_uint64()
        with torch.cuda.device(self.device):
            _lib.check(_lib.load().gm_solver_line(
                self._h, int(key), kd.data_ptr(), wd.data_ptr(), cap,
                ctypes.byref(n)))
        w = wd[:n.value].cpu().numpy().view(np.uint32)
        return (kd[:n.value].cpu().numpy().view(np.uint64),
                (w & 3).astype(np.uint8), (w >> 2).astype(np.uint32))

    def audit(self, max_bad=64):
        """Re-derive every stored word from its children's stored words
        through the query path (gm_solver_audit): dict with positions, edges,
        mismatches and bad_keys (up to max_bad mismatching keys, u64)."""
        torch = self.torch
        max_bad = int(max_bad)
        bad = torch.empty(max(1, max_bad), dtype=torch.int64, device=self.device)
        out = np.zeros(4, np.uint64)
        with torch.cuda.device(self.device):
            _lib.check(_lib.load().gm_solver_audit(
                self._h, bad.data_ptr(), max_bad, out.ctypes.data))
        return {"positions": int(out[0]), "edges": int(out[1]),
                "mismatches": int(out[2]),
                "bad_keys": bad[:int(out[3])].cpu().numpy().view(np.uint64)}

    def census(self, rem_bins=None, generic=False, levels=True, extremes=True):
        """Positions by value and remoteness, by value and level, and the
        hardest position of each value (gm_solver_census), without copying
        the table: dict with by_remoteness (uint64 [rem_bins + 1, 4], columns
        WIN LOSS TIE DRAW, the last row every remoteness >= rem_bins),
        by_level (uint64 [max_levels, 4]) and extremes, per value a dict with
        count, max_remoteness and key (the smallest key of that value and
        remoteness; None when the value has no position).  rem_bins defaults
        to min(max_levels + 1, 65536): every move advances at least one level,
        so no remoteness exceeds the levels.  generic=True counts through the
        position enumerator and the query path on every layout.  levels=False
        / extremes=False leave that part out (by_level / extremes are None)."""
        torch = self.torch
        nlev = int(self.plan.max_levels)
        rem_bins = min(nlev + 1, 65536) if rem_bins is None else int(rem_bins)
        if not 0 <= rem_bins < 0xFFFFFFFF:
            raise ValueError("rem_bins must be in [0, 2^32 - 1)")
        rd = torch.empty((rem_bins + 1, 4), dtype=torch.int64, device=self.device)
        ld = torch.empty((nlev, 4), dtype=torch.int64, device=self.device) if levels else None
        ex = np.zeros(12, np.uint64) if extremes else None
        with torch.cuda.device(self.device):
            _lib.check(_lib.load().gm_solver_census(
                self._h, _lib.GM_CENSUS_GENERIC if generic else 0, rd.data_ptr(), rem_bins,
                ld.data_ptr() if levels else None, nlev if levels else 0,
                ex.ctypes.data if extremes else None))
        out = {"by_remoteness": rd.cpu().numpy().view(np.uint64),
               "by_level": ld.cpu().numpy().view(np.uint64) if levels else None,
               "extremes": None}
        if extremes:
            out["extremes"] = [
                {"count": int(ex[3 * v]), "max_remoteness": int(ex[3 * v + 1]),
                 "key": None if int(ex[3 * v + 2]) == _lib.GM_EMPTY_KEY else int(ex[3 * v + 2])}
                for v in range(4)]
        return out

    # -- the indexed tablebase (gm_solver_export; db.Tablebase reads it) ------
    def export_range(self, first, count, word_bytes, generic=False, words_cap=None):
        """Tablebase sections of indexes [first, first + count) as device
        tensors (gm_solver_export): (bits int64[count / 64], block_counts
        int32[count / 512], words uint8[n * word_bytes]).  words_cap: room for
        that many words (default: one per index); TableFull when short."""
        torch = self.torch
        first, count, word_bytes = int(first), int(count), int(word_bytes)
        cap = count if words_cap is None else int(words_cap)
        bits = torch.empty(max(1, count // 64), dtype=torch.int64, device=self.device)
        counts = torch.empty(max(1, count // _lib.GM_TB_BLOCK), dtype=torch.int32, device=self.device)
        words = torch.empty(max(16, cap * word_bytes), dtype=torch.uint8, device=self.device)
        n = ctypes.c_uint64()
        with torch.cuda.device(self.device):
            _lib.check(_lib.load().gm_solver_export(
                self._h, _lib.GM_EXPORT_GENERIC if generic else 0, first, count, word_bytes,
                bits.data_ptr(), counts.data_ptr(), words.data_ptr(), cap, ctypes.byref(n)))
        return bits[:count // 64], counts[:count // _lib.GM_TB_BLOCK], words[:n.value * word_bytes]

    def export_tablebase(self, path, chunk=1 << 26, generic=False):
        """Write the finished solve as the indexed tablebase `path`
        (solution.gmtb, db.Tablebase): the reach bitmap over the game's index
        space, a cumulative count per 512-index block and one compact word per
        reached index, all produced on the device `chunk` indexes at a time
        and streamed to the file through one pinned host buffer -- no keys, no
        host copy of the table.  The word width comes from the census' largest
        remoteness.  Returns dict(path, bytes, positions, word_bytes)."""
        import os
        from . import db
        torch = self.torch
        space = self.spec.tb_index_space()
        ext = self.census(rem_bins=0, levels=False)["extremes"]
        wb = db.tb_word_bytes(max(e["max_remoteness"] for e in ext))
        chunk = max(_lib.GM_TB_BLOCK, int(chunk) // _lib.GM_TB_BLOCK * _lib.GM_TB_BLOCK)
        _, bits_off, counts_off, words_off = db.tb_header(space, wb, 0)
        stage = torch.empty(min(chunk, space) * wb, dtype=torch.uint8, pin_memory=True)
        host = stage.numpy()

        def out(fh, at, t):  # device tensor -> file offset `at`, through the pinned buffer
            flat = t.view(torch.uint8).reshape(-1)
            stage[:flat.numel()].copy_(flat)
            fh.seek(at)
            fh.write(host[:flat.numel()].data)

        tmp = path + ".tmp"
        npos = 0
        with open(tmp, "wb") as fh:
            fh.write(b"\0" * db.TB_HEADER)
            fh.seek(counts_off)
            fh.write(np.zeros(1, "<u8").tobytes())
            for first in range(0, space, chunk):
                count = min(chunk, space - first)
                bits, counts, words = self.export_range(first, count, wb, generic)
                out(fh, bits_off + first // 8, bits)
                cum = torch.cumsum(counts.to(torch.int64), 0) + npos
                out(fh, counts_off + 8 * (first // _lib.GM_TB_BLOCK + 1), cum)
                if words.numel():
                    out(fh, words_off + npos * wb, words)
                npos += words.numel() // wb
            fh.seek(0)
            fh.write(db.tb_header(space, wb, npos)[0])
        os.replace(tmp, path)
        return {"path": path, "bytes": words_off + npos * wb, "positions": npos, "word_bytes": wb}

    # -- the keyed tablebase (gm_solver_export_keyed; db.KeyedTablebase reads it) --
    def _export_keyed(self, bucket_bits, word_bytes, generic, cap):
        """One gm_solver_export_keyed call: (rc, out u64[4], dir, keys, words)."""
        torch = self.torch
        stage = torch.empty(max(2, cap * 3 // 2 + 1), dtype=torch.int64, device=self.device)  # cap * 12 bytes
        d = torch.empty((1 << bucket_bits) + 1, dtype=torch.int64, device=self.device)
        keys = torch.empty(max(16, cap * 8), dtype=torch.uint8, device=self.device)
        words = torch.empty(max(16, cap * word_bytes), dtype=torch.uint8, device=self.device)
        out = np.zeros(4, np.uint64)
        with torch.cuda.device(self.device):
            rc = _lib.load().gm_solver_export_keyed(
                self._h, _lib.GM_EXPORT_GENERIC if generic else 0, bucket_bits, word_bytes,
                stage.data_ptr(), d.data_ptr(), keys.data_ptr(), words.data_ptr(), cap, out.ctypes.data)
        return rc, out, d, keys, words

    def export_keyed(self, bucket_bits, word_bytes, generic=False, cap=None):
        """Keyed tablebase sections as device tensors (gm_solver_export_keyed):
        (dir int64[2^bucket_bits + 1], keys uint8[n * key_bytes], words
        uint8[n * word_bytes]) -- the keys by bucket, then ascending, each cut
        to key_bytes = keys.numel() // n bytes.  cap: room for that many
        positions (default: the census' count); TableFull when it is short or
        a bucket holds more than 1,024 positions."""
        bucket_bits, word_bytes = int(bucket_bits), int(word_bytes)
        if cap is None:
            cap = sum(e["count"] for e in self.census(rem_bins=0, levels=False)["extremes"])
        rc, out, d, keys, words = self._export_keyed(bucket_bits, word_bytes, generic, int(cap))
        _lib.check(rc)
        n, kb = int(out[0]), int(out[1])
        return d, keys[:n * kb], words[:n * word_bytes]

    def export_keyed_tablebase(self, path, bucket_bits=None, generic=False, chunk=1 << 26):
        """Write the finished solve as the keyed tablebase `path`
        (solution.gmtk, db.KeyedTablebase): a directory of hash buckets, the
        truncated keys sorted inside each bucket and one compact word per key,
        all produced on the device and streamed to the file through one pinned
        host buffer of `chunk` bytes -- no host copy of the table.  The word
        width comes from the census' largest remoteness; bucket_bits defaults
        to about 256 positions per bucket and grows while a bucket holds more
        than the device sort's 1,024.  Returns dict(path, bytes, positions,
        word_bytes, key_bytes, bucket_bits)."""
        import os
        from . import db
        torch = self.torch
        ext = self.census(rem_bins=0, levels=False)["extremes"]
        npos = sum(e["count"] for e in ext)
        wb = db.tb_word_bytes(max(e["max_remoteness"] for e in ext))
        b = db.tk_default_bits(npos) if bucket_bits is None else int(bucket_bits)
        while True:
            rc, out, d, keys, words = self._export_keyed(b, wb, generic, npos)
            if rc == _lib.GM_EFULL and int(out[2]) > _lib.GM_TK_BUCKET_CAP and b < 32:
                b += 1  # a bucket over the sort's capacity: halve the buckets
                continue
            _lib.check(rc)
            break
        if int(out[0]) != npos:
            raise RuntimeError("the export wrote %d positions, the census counted %d" % (int(out[0]), npos))
        kb = int(out[1])
        head, _, _, _, total = db.tk_header(wb, kb, b, npos)
        stage = torch.empty(max(16, min(int(chunk), max(d.numel() * 8, npos * kb))), dtype=torch.uint8,
                            pin_memory=True)
        host = stage.numpy()
        tmp = path + ".tmp"
        with open(tmp, "wb") as fh:
            fh.write(head)
            for t in (d, keys[:npos * kb], words[:npos * wb]):  # the sections, in file order
                flat = t.view(torch.uint8).reshape(-1)
                for a in range(0, flat.numel(), stage.numel()):
                    part = flat[a:a + stage.numel()]
                    stage[:part.numel()].copy_(part)
                    fh.write(host[:part.numel()].data)
        os.replace(tmp, path)
        return {"path": path, "bytes": total, "positions": npos, "word_bytes": wb, "key_bytes": kb,
                "bucket_bits": b}

    @staticmethod
    def open_tablebase(spec, path, device=None):
        """A saved tablebase (solution.gmtb / solution.gmtk) opened on the GPU
        (gm_solver_open_table; gamesmanmpi_amd.table.OpenTable): the file's
        bytes streamed through one pinned chunk into one device buffer and
        read in place.  The returned object answers query / positions /
        checksum / moves / best_line / audit / census / export_tablebase /
        export_keyed_tablebase as a Solver that has just solved does, and
        raises GmError(GM_EINVAL) for solve(), solve_steps() and checkpoints.
        GmError(GM_EINVAL) for a file whose header is wrong (what db.Tablebase
        / db.KeyedTablebase refuse), GmError(GM_ECORRUPT) for one whose bitmap
        and counts, or directory and keys, disagree."""
        from .table import OpenTable
        return OpenTable(spec, path, device=device)

    def dump(self):
        """(keys u64, value u8, remoteness u32) for every reachable
        position."""
        keys = self.positions()
        w = self.query(keys)
        if (w == _lib.GM_NO_WORD).any():
            raise RuntimeError("unresolved positions in the table")
        return keys, (w & 3).astype(np.uint8), (w >> 2).astype(np.uint32)


def solve(name, params="", positions=0, device=None):
    """Convenience: solve game `name` (reference file stem) on one GPU."""
    s = Solver(GameSpec(name, params), positions=positions, device=device)
    return s.solve(), s
