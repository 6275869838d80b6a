"""A saved tablebase opened on the GPU (gm_solver_open_table, DESIGN.md
section 7j): the bytes of solution.gmtb / solution.gmtk streamed into one
device buffer and read in place by every reader of a solved table.

Stands in for reading a saved solution back key by key from the reference's
resolved / remote shelves (src/cache_dict.py:62-79).  The host readers of the
same files are db.Tablebase and db.KeyedTablebase.

    t = Solver.open_tablebase(spec, "DIR/stats/0/solution.gmtk")
    t.query(keys); t.moves(keys); t.best_line(); t.audit(); t.census()

OpenTable IS a Solver as far as reading goes -- query, positions, checksum,
moves, best_line, audit, census, export_tablebase and export_keyed_tablebase
are Solver's own methods on the handle gm_solver_open_table returns -- and
refuses everything that would solve: solve(), solve_steps(), solve_async(),
set_kernel_timing() and checkpoints raise GmError(GM_EINVAL).
"""
import ctypes
import os

import numpy as np

from . import _lib
from .games import GameSpec
from .solver import Solver


def check_header(spec, path):
    """gm_table_check of the file at `path` (host only, no GPU): dict with
    format ("gmtb" / "gmtk"), positions, word_bytes, key_bytes, bucket_bits,
    index_space, the three section offsets, scratch_bytes and index_bytes.
    GmError(GM_EINVAL) for a file db.Tablebase / db.KeyedTablebase refuse."""
    size = os.path.getsize(path)
    with open(path, "rb") as fh:
        head = fh.read(64)
    out = (ctypes.c_uint64 * 12)()
    _lib.check(_lib.load().gm_table_check(spec.id, head, len(head), size, out))
    v = [int(x) for x in out]
    return {"format": {1: "gmtb", 2: "gmtk"}[v[0]], "positions": v[1], "word_bytes": v[2],
            "key_bytes": v[3], "bucket_bits": v[4], "index_space": v[5],
            "offsets": (v[6], v[7], v[8]), "scratch_bytes": v[9], "index_bytes": v[10],
            "bytes": size}


class OpenTable(Solver):
    """The image of one tablebase file on one GPU (module docstring)."""

    def __init__(self, spec, path, device=None, chunk=1 << 26):
        import torch
        if not torch.cuda.is_available():
            raise RuntimeError("gamesmanmpi_amd needs a ROCm GPU (gfx950); no device is visible")
        self.torch = torch
        self.spec = spec if isinstance(spec, GameSpec) else GameSpec(*spec)
        self.device = torch.device(device if device is not None else "cuda")
        self.path = path
        self.kernel_timing = False
        self.layout = self._planned_layout = "file"
        self.max_table_bytes = 0
        self.rank, self.world = 0, 1
        self.stream = None
        self.flags = self._cflags = 0
        self.staging_records = 0
        self.positions_hint = 0
        self._h = None
        self._tensors = None
        self._bufs = None
        self.info = check_header(self.spec, path)
        size = self.info["bytes"]
        plan = _lib.gm_plan_t()
        plan.table_bytes, plan.table_slots = size, self.info["positions"]
        plan.level_capacity, plan.scratch_bytes = 0, self.info["scratch_bytes"]
        plan.max_levels, plan.mode = self.spec.max_levels, _lib.GM_MODE_FILE
        self.plan = plan
        self.claimed_table_bytes = size
        with torch.cuda.device(self.device):
            image = torch.empty(max(256, size), dtype=torch.uint8, device=self.device)
            scratch = torch.empty(plan.scratch_bytes, dtype=torch.uint8, device=self.device)
            stream = torch.cuda.current_stream(self.device)
            # the file through one pinned chunk into the image
            stage = torch.empty(max(16, min(int(chunk), size)), dtype=torch.uint8, pin_memory=True)
            host = stage.numpy()
            with open(path, "rb") as fh:
                at = 0
                while at < size:
                    n = fh.readinto(memoryview(host)[:min(len(host), size - at)])
                    if not n:
                        raise ValueError("%s shrank while it was read" % path)
                    image[at:at + n].copy_(stage[:n])  # (synchronous: pinned -> device)
                    at += n
            torch.cuda.synchronize(self.device)
            self._tensors = (image, scratch)
            h = ctypes.c_void_p()
            _lib.check(_lib.load().gm_solver_open_table(
                self.spec.id, image.data_ptr(), size, scratch.data_ptr(), plan.scratch_bytes,
                stream.cuda_stream, ctypes.byref(h)))
        self._h = h

    def _refuse(self, what):
        raise _lib.GmError(_lib.GM_EINVAL, "%s: an opened tablebase file is read, never solved" % what)

    def _alloc(self, positions):
        self._refuse("a new plan")

    def solve(self, max_retries=0):
        """GmError(GM_EINVAL), from gm_solver_solve itself."""
        r = _lib.gm_result()
        with self.torch.cuda.device(self.device):
            _lib.check(_lib.load().gm_solver_solve(self._h, ctypes.byref(r)))
        self._refuse("solve")  # (not reached)

    def solve_async(self):
        self._refuse("solve_async")

    @property
    def buffers(self):
        """Checkpoints are of solves: GmError(GM_EINVAL)."""
        self._refuse("checkpoint")

    @property
    def image(self):
        """The file's bytes on the device (uint8 tensor)."""
        return self._tensors[0]

    def dump(self):
        keys = self.positions()
        w = self.query(keys)
        return keys, (w & 3).astype(np.uint8), (w >> 2).astype(np.uint32)


def open_tablebase(spec, path, device=None):
    """Solver.open_tablebase."""
    return OpenTable(spec, path, device=device)
