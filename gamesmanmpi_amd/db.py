"""Solution database written by the launcher's -sd option, and queries on it.

The reference keeps a rank's results in shelve files
`<DIR>/stats/<rank>/{resolved,remote}` (src/cache_dict.py:19-42): value and
remoteness per position key.  The launcher writes the binary counterpart,
`<DIR>/stats/<rank>/solution.npz` + `meta.json` per rank (solver_launcher.py
write_stats), and this module reads any number of rank directories back as
one table:

    python -m gamesmanmpi_amd.db DIR --game GAME_FILE [POSITION ...]

prints `<position>: <VALUE> in <r> moves` for each position (a Python
literal evaluated against nothing but literals, e.g. 4 or '...'), or for the
game's initial position when none is given.  Descriptor-solved tables are
keyed by the packed u64 key (GameSpec.key_of); graph-solved tables (game
files without a descriptor) by str(position).

    python -m gamesmanmpi_amd.db DIR --game GAME_FILE --moves [POSITION ...]

adds, under each position, one row per legal move (the module's gen_moves /
do_move) with the child's value and remoteness from the table, the best move
marked with `*` (best_index below; the rule of gm_solver_moves,
include/gamesman.h).

    python -m gamesmanmpi_amd.db DIR --game GAME_FILE --census

prints the analysis table of the whole solution instead: positions by
remoteness x (Win Lose Tie Draw Total), then by level x the same
(census_of / format_census below; the launcher's --census prints the same
tables from the device's gm_solver_census).  Graph tables have no level
function and print the remoteness table only.  Host only: no GPU is touched.

Indexed games (four_to_one, sum_four_to_one, toot_and_otto_bitstring) may be
saved as an indexed tablebase instead, `<DIR>/stats/0/solution.gmtb` (the
launcher's `-sd DIR --tablebase`, written on the GPU by
Solver.export_tablebase; the format and its reader, Tablebase, are below):
SolutionDB opens it with np.memmap when present and every query above works
on it unchanged, except that --census prints the remoteness table only.

    python -m gamesmanmpi_amd.db DIR --game GAME_FILE --to-tablebase

converts a directory's solution.npz files to that file (write_tablebase).

The other descriptor games (tic_tac_toe_np, mttt, othello_bit_new) have no
index function; their counterpart is the keyed tablebase
`<DIR>/stats/0/solution.gmtk` (Solver.export_keyed_tablebase; the format, its
numpy writer write_keyed_tablebase and its reader KeyedTablebase are below):
truncated keys grouped by hash bucket and sorted inside a bucket, one compact
word per key.  `-sd DIR --tablebase` and `--to-tablebase` write it for those
games, and SolutionDB opens it the same way.

    python -m gamesmanmpi_amd.db DIR --game GAME_FILE --gpu [--audit | --census | --moves] [POSITION ...]

opens the directory's tablebase file on the GPU instead
(Solver.open_tablebase, gm_solver_open_table): positions
and --moves are answered from the image on the device, --census prints the
by-level table and the longest lines too (the launcher's --census output),
and --audit re-derives every stored word from its children's, printing up to
64 mismatching positions, exit status 1 on a mismatch.  Without --gpu nothing
changes and no GPU is touched.
"""
import argparse
import ast
import glob
import json
import os
import sys

import numpy as np

NAMES = ("WIN", "LOSS", "TIE", "DRAW")

# ---------------------------------------------------------------------------
# the indexed tablebase, solution.gmtb
# ---------------------------------------------------------------------------
# A position of an indexed game has an index computed from its key alone
# (gm_tb_index).  The file holds, little-endian:
#   header   64 bytes: magic "GMTBASE1", u32 version, u32 word_bytes, then u64
#            index_space, positions, bitmap offset, counts offset, words
#            offset, file bytes
#   bitmap   index_space / 8 bytes: bit i (of u64 i / 64, bit i % 64) = index
#            i is reached
#   counts   index_space / 512 + 1 u64: reached indexes before each 512-block
#   words    positions * word_bytes: value | remoteness << 2 of the reached
#            indexes, in index order
# A lookup is one bit test, the block's count plus the popcount of the
# block's earlier bitmap words, and one load; no keys are stored and nothing
# is loaded up front.
TB_MAGIC = b"GMTBASE1"
TB_VERSION = 1
TB_HEADER = 64
TB_BLOCK = 512
TB_NAME = "solution.gmtb"
_TB_DTYPES = {1: np.dtype("<u1"), 2: np.dtype("<u2"), 4: np.dtype("<u4")}
NO_WORD = 0xFFFFFFFF
NO_INDEX = 0xFFFFFFFFFFFFFFFF


def tb_word_bytes(max_remoteness):
    """Bytes of a compact word (value | remoteness << 2) that hold every
    remoteness up to max_remoteness."""
    return 1 if max_remoteness <= 63 else 2 if max_remoteness <= 16383 else 4


def tb_header(index_space, word_bytes, positions):
    """The 64 header bytes and the three section offsets."""
    if index_space % TB_BLOCK or word_bytes not in _TB_DTYPES:
        raise ValueError("index space %d / word bytes %d" % (index_space, word_bytes))
    bits_off = TB_HEADER
    counts_off = bits_off + index_space // 8
    words_off = counts_off + 8 * (index_space // TB_BLOCK + 1)
    total = words_off + positions * word_bytes
    head = TB_MAGIC + np.array([TB_VERSION, word_bytes], "<u4").tobytes() + np.array(
        [index_space, positions, bits_off, counts_off, words_off, total], "<u8").tobytes()
    assert len(head) == TB_HEADER
    return head, bits_off, counts_off, words_off


_POP8 = np.array([bin(i).count("1") for i in range(256)], np.uint8)


def _popcount64(x):
    """Set bits of each uint64 of `x` (any shape), as int64."""
    x = np.ascontiguousarray(x, dtype="<u8")
    return _POP8[x.view(np.uint8).reshape(x.shape + (8,))].sum(axis=-1, dtype=np.int64)


def write_tablebase(path, index_space, indexes, words, word_bytes):
    """Write solution.gmtb from (index, word) pairs on the host (pure numpy;
    the device writer is Solver.export_tablebase).  index_space: gm_tb_info's;
    words: value | remoteness << 2."""
    indexes = np.ascontiguousarray(indexes, dtype=np.uint64)
    words = np.ascontiguousarray(words, dtype=np.uint32)
    if len(indexes) != len(words):
        raise ValueError("%d indexes, %d words" % (len(indexes), len(words)))
    order = np.argsort(indexes, kind="stable")
    indexes, words = indexes[order], words[order]
    if len(indexes) and int(indexes[-1]) >= index_space:
        raise ValueError("index %d outside the index space %d" % (int(indexes[-1]), index_space))
    if len(indexes) > 1 and (np.diff(indexes) == 0).any():
        raise ValueError("an index appears twice")
    if word_bytes < 4 and len(words) and int(words.max()) >> (8 * word_bytes):
        raise ValueError("remoteness %d does not fit words of %d byte(s)" % (int(words.max()) >> 2, word_bytes))
    head, _, _, _ = tb_header(index_space, word_bytes, len(indexes))
    reached = np.zeros(index_space, np.uint8)
    reached[indexes.astype(np.int64)] = 1
    counts = np.zeros(index_space // TB_BLOCK + 1, "<u8")
    counts[1:] = np.cumsum(reached.reshape(-1, TB_BLOCK).sum(axis=1, dtype=np.uint64))
    tmp = path + ".tmp"
    with open(tmp, "wb") as f:
        f.write(head)
        f.write(np.packbits(reached, bitorder="little").tobytes())
        f.write(counts.tobytes())
        f.write(words.astype(_TB_DTYPES[word_bytes]).tobytes())
    os.replace(tmp, path)


class Tablebase:
    """solution.gmtb opened with np.memmap: the three sections are mapped,
    nothing is read until a lookup touches it.  spec: the game's GameSpec
    (its gm_tb_index maps keys to indexes)."""

    def __init__(self, path, spec=None):
        self.path, self.spec = path, spec
        size = os.path.getsize(path)
        with open(path, "rb") as f:
            head = f.read(TB_HEADER)
        if len(head) < TB_HEADER or head[:8] != TB_MAGIC:
            raise ValueError("%s is no tablebase (bad magic)" % path)
        version, wb = (int(x) for x in np.frombuffer(head, "<u4", 2, 8))
        space, npos, bits_off, counts_off, words_off, total = (int(x) for x in np.frombuffer(head, "<u8", 6, 16))
        if version != TB_VERSION:
            raise ValueError("%s: tablebase version %d, this reader knows %d" % (path, version, TB_VERSION))
        if wb not in _TB_DTYPES or space % TB_BLOCK:
            raise ValueError("%s: bad header (word bytes %d, index space %d)" % (path, wb, space))
        want = tb_header(space, wb, npos)
        if (bits_off, counts_off, words_off) != want[1:] or total != words_off + npos * wb:
            raise ValueError("%s: section offsets do not match the header's sizes" % path)
        if size != total:
            raise ValueError("%s holds %d bytes, its header says %d (truncated?)" % (path, size, total))
        if spec is not None and spec.tb_index_space() != space:
            raise ValueError("%s: index space %d, %r has %d" % (path, space, spec, spec.tb_index_space()))
        self.index_space, self.positions, self.word_bytes = space, npos, wb
        self.bits = np.memmap(path, "<u8", "r", bits_off, (space // 64,))
        self.counts = np.memmap(path, "<u8", "r", counts_off, (space // TB_BLOCK + 1,))
        self.words = (np.memmap(path, _TB_DTYPES[wb], "r", words_off, (npos,)) if npos
                      else np.zeros(0, _TB_DTYPES[wb]))
        if int(self.counts[-1]) != npos:  # (one page of the counts: every lookup's bound)
            raise ValueError("%s: %d reached indexes counted, %d words" % (path, int(self.counts[-1]), npos))

    def __len__(self):
        return self.positions

    def lookup_indexes(self, indexes):
        """uint32 words (value | remoteness << 2) of tablebase indexes;
        NO_WORD for an unreached index, NO_INDEX or an index outside the space."""
        idx = np.ascontiguousarray(indexes, dtype=np.uint64)
        out = np.full(len(idx), NO_WORD, np.uint32)
        ok = idx < np.uint64(self.index_space)
        if not ok.any():
            return out
        i = idx[ok].astype(np.int64)
        w, b = i >> 6, (i & 63).astype(np.uint64)
        word = np.asarray(self.bits[w])
        hit = ((word >> b) & np.uint64(1)).astype(bool)
        i, w, b, word = i[hit], w[hit], b[hit], word[hit]
        blk = i >> 9
        # the block's earlier bitmap words, then the bits below in this word
        rows = np.asarray(self.bits[(blk[:, None] << 3) + np.arange(8)[None, :]])
        before = np.arange(8)[None, :] < (w & 7)[:, None]
        rank = (np.asarray(self.counts[blk]).astype(np.int64) + (_popcount64(rows) * before).sum(axis=1)
                + _popcount64(word & ((np.uint64(1) << b) - np.uint64(1))))
        if len(rank) and int(rank.max()) >= self.positions:
            raise ValueError("%s: the bitmap and the block counts disagree" % self.path)
        res = np.full(len(hit), NO_WORD, np.uint32)
        res[hit] = np.asarray(self.words[rank]).astype(np.uint32)
        out[ok] = res
        return out

    def lookup_keys(self, keys):
        """uint32 words of packed u64 keys (NO_WORD: not in the table)."""
        if self.spec is None:
            raise ValueError("a tablebase lookup by key needs the game's GameSpec")
        return self.lookup_indexes(self.spec.tb_index(keys))

    def lookup_key(self, key):
        w = int(self.lookup_keys(np.array([key], np.uint64))[0])
        return None if w == NO_WORD else (w & 3, w >> 2)

    def by_remoteness(self, rem_bins=None, chunk=1 << 24):
        """census_of's by_remoteness table, streamed from the words section."""
        top = 0
        for a in range(0, self.positions, chunk):
            top = max(top, int(np.asarray(self.words[a:a + chunk]).max()) >> 2)
        if rem_bins is None:
            rem_bins = top + 1 if self.positions else 0
        by_rem = np.zeros((int(rem_bins) + 1, 4), np.uint64)
        for a in range(0, self.positions, chunk):
            w = np.asarray(self.words[a:a + chunk]).astype(np.int64)
            np.add.at(by_rem, (np.minimum(w >> 2, int(rem_bins)), w & 3), 1)
        return by_rem


# ---------------------------------------------------------------------------
# the keyed tablebase, solution.gmtk
# ---------------------------------------------------------------------------
# For games without an index function (tic_tac_toe_np, mttt, othello_bit_new;
# any keyed table works).  bucket(key) = the top bucket_bits bits of
# mix64(key), 0 when bucket_bits is 0.  The file holds, little-endian:
#   header     64 bytes: magic "GMTBKEY1", u32 version, u32 word_bytes, u32
#              key_bytes, u32 bucket_bits, then u64 positions, directory
#              offset, keys offset, words offset, file bytes
#   directory  2^bucket_bits + 1 u64: dir[h] = positions in buckets below h
#   keys       positions * key_bytes: the low key_bytes bytes of each key,
#              by bucket, then by key ascending (key_bytes holds the OR of all
#              keys, at least 1)
#   words      positions * word_bytes: value | remoteness << 2, same order
# A lookup reads two directory entries and binary-searches one bucket (about
# 256 keys at the default bucket_bits); nothing is loaded up front.
TK_MAGIC = b"GMTBKEY1"
TK_VERSION = 1
TK_HEADER = 64
TK_NAME = "solution.gmtk"
TK_BUCKET = 256  # positions per bucket the default bucket_bits aims at


def mix64(keys):
    """gm_mix64 in numpy: the hash whose top bits choose a key's bucket."""
    x = np.array(keys, dtype=np.uint64, copy=True, ndmin=1)
    with np.errstate(over="ignore"):
        x ^= x >> np.uint64(31)
        x *= np.uint64(0x7fb5d329728ea185)
        x ^= x >> np.uint64(27)
        x *= np.uint64(0x81dadef4bc2dd44d)
        x ^= x >> np.uint64(33)
    return x


def tk_bucket(keys, bucket_bits):
    """Bucket of each key, as int64."""
    if not bucket_bits:
        return np.zeros(len(np.atleast_1d(keys)), np.int64)
    return (mix64(keys) >> np.uint64(64 - bucket_bits)).astype(np.int64)


def tk_default_bits(positions):
    """The smallest bucket_bits for which positions / 2^bits <= TK_BUCKET."""
    b = 0
    while positions > TK_BUCKET << b:
        b += 1
    return b


def tk_header(word_bytes, key_bytes, bucket_bits, positions):
    """The 64 header bytes, the three section offsets and the file's bytes."""
    if word_bytes not in _TB_DTYPES or not 1 <= key_bytes <= 8 or not 0 <= bucket_bits <= 32:
        raise ValueError("word bytes %d / key bytes %d / bucket bits %d" % (word_bytes, key_bytes, bucket_bits))
    dir_off = TK_HEADER
    keys_off = dir_off + 8 * ((1 << bucket_bits) + 1)
    words_off = keys_off + positions * key_bytes
    total = words_off + positions * word_bytes
    head = TK_MAGIC + np.array([TK_VERSION, word_bytes, key_bytes, bucket_bits], "<u4").tobytes() + np.array(
        [positions, dir_off, keys_off, words_off, total], "<u8").tobytes()
    assert len(head) == TK_HEADER
    return head, dir_off, keys_off, words_off, total


def tk_key_bytes(keys):
    """Bytes that hold the OR of `keys` (at least 1)."""
    top = int(np.bitwise_or.reduce(np.asarray(keys, np.uint64))) if len(keys) else 0
    return max(1, (top.bit_length() + 7) // 8)


def write_keyed_tablebase(path, keys, words, word_bytes, bucket_bits=None):
    """Write solution.gmtk from (key, word) pairs on the host (pure numpy; the
    device writer is Solver.export_keyed_tablebase, which this restates byte
    for byte).  words: value | remoteness << 2.  Returns bucket_bits."""
    keys = np.ascontiguousarray(keys, dtype=np.uint64)
    words = np.ascontiguousarray(words, dtype=np.uint32)
    if len(keys) != len(words):
        raise ValueError("%d keys, %d words" % (len(keys), len(words)))
    b = tk_default_bits(len(keys)) if bucket_bits is None else int(bucket_bits)
    if word_bytes < 4 and len(words) and int(words.max()) >> (8 * word_bytes):
        raise ValueError("remoteness %d does not fit words of %d byte(s)" % (int(words.max()) >> 2, word_bytes))
    kb = tk_key_bytes(keys)
    head, _, _, _, _ = tk_header(word_bytes, kb, b, len(keys))
    h = tk_bucket(keys, b)
    order = np.lexsort((keys, h))
    keys, words, h = keys[order], words[order], h[order]
    if len(keys) > 1 and (np.diff(keys) == 0).any():  # (equal keys share a bucket: neighbours after the sort)
        raise ValueError("a key appears twice")
    directory = np.zeros((1 << b) + 1, "<u8")
    directory[1:] = np.cumsum(np.bincount(h, minlength=1 << b))
    tmp = path + ".tmp"
    with open(tmp, "wb") as f:
        f.write(head)
        f.write(directory.tobytes())
        f.write(np.ascontiguousarray(keys.astype("<u8").view(np.uint8).reshape(-1, 8)[:, :kb]).tobytes())
        f.write(words.astype(_TB_DTYPES[word_bytes]).tobytes())
    os.replace(tmp, path)
    return b


class KeyedTablebase:
    """solution.gmtk opened with np.memmap: the three sections are mapped,
    nothing is read until a lookup touches it.  The header is checked against
    the file's size before anything is mapped; a lookup checks the directory
    entries it reads (check_directory() reads all of them)."""

    def __init__(self, path, spec=None):
        self.path, self.spec = path, spec
        size = os.path.getsize(path)
        with open(path, "rb") as f:
            head = f.read(TK_HEADER)
        if len(head) < TK_HEADER or head[:8] != TK_MAGIC:
            raise ValueError("%s is no keyed tablebase (bad magic)" % path)
        version, wb, kb, b = (int(x) for x in np.frombuffer(head, "<u4", 4, 8))
        npos, dir_off, keys_off, words_off, total = (int(x) for x in np.frombuffer(head, "<u8", 5, 24))
        if version != TK_VERSION:
            raise ValueError("%s: keyed tablebase version %d, this reader knows %d" % (path, version, TK_VERSION))
        try:
            want = tk_header(wb, kb, b, npos)
        except ValueError as e:
            raise ValueError("%s: bad header (%s)" % (path, e))
        if (dir_off, keys_off, words_off, total) != want[1:]:
            raise ValueError("%s: section offsets do not match the header's sizes" % path)
        if size != total:
            raise ValueError("%s holds %d bytes, its header says %d (truncated?)" % (path, size, total))
        self.positions, self.word_bytes, self.key_bytes, self.bucket_bits = npos, wb, kb, b
        self.dir = np.memmap(path, "<u8", "r", dir_off, ((1 << b) + 1,))
        self.keys = (np.memmap(path, np.uint8, "r", keys_off, (npos, kb)) if npos
                     else np.zeros((0, kb), np.uint8))
        self.words = (np.memmap(path, _TB_DTYPES[wb], "r", words_off, (npos,)) if npos
                      else np.zeros(0, _TB_DTYPES[wb]))
        if int(self.dir[0]) != 0 or int(self.dir[-1]) != npos:  # (the directory's two ends: every lookup's bounds)
            raise ValueError("%s: the directory counts %d..%d positions, the header %d"
                             % (path, int(self.dir[0]), int(self.dir[-1]), npos))

    def __len__(self):
        return self.positions

    def check_directory(self, chunk=1 << 22):
        """Read the whole directory: ValueError unless it never decreases."""
        n = len(self.dir)
        for a in range(0, n - 1, chunk):
            d = np.asarray(self.dir[a:a + chunk + 1])
            if len(d) > 1 and (d[1:] < d[:-1]).any():
                raise ValueError("%s: the directory decreases" % self.path)

    def _key_at(self, at):
        """u64 keys stored at positions `at` (int64 array)."""
        buf = np.zeros((len(at), 8), np.uint8)
        buf[:, :self.key_bytes] = self.keys[at]
        return buf.view("<u8")[:, 0]

    def lookup_keys(self, keys):
        """uint32 words (value | remoteness << 2) of packed u64 keys; NO_WORD
        for a key the table does not hold.  One bucket range per query, then
        ceil(log2(largest range + 1)) binary-search steps over all of them.
        Opened with a symmetric GameSpec (symmetry=1 / board_symmetry=1), the
        keys are mapped to their orbit representatives first."""
        if self.spec is not None and self.spec.symmetric:
            keys = self.spec.symmetry(keys)
        q = np.ascontiguousarray(keys, dtype=np.uint64)
        out = np.full(len(q), NO_WORD, np.uint32)
        ok = np.ones(len(q), bool)
        if self.key_bytes < 8:  # a bit above the stored bytes: absent, no search
            ok = (q >> np.uint64(8 * self.key_bytes)) == 0
        if not ok.any() or not self.positions:
            return out
        q = q[ok]
        h = tk_bucket(q, self.bucket_bits)
        lo = np.asarray(self.dir[h]).astype(np.int64)
        end = np.asarray(self.dir[h + 1]).astype(np.int64)
        if (end < lo).any() or (end > self.positions).any():
            raise ValueError("%s: the directory decreases or passes the position count" % self.path)
        hi = end.copy()
        for _ in range(int((hi - lo).max()).bit_length()):  # lower bound of q in [lo, hi)
            act = np.flatnonzero(lo < hi)
            if not len(act):
                break
            mid = (lo[act] + hi[act]) >> 1
            less = self._key_at(mid) < q[act]
            lo[act] = np.where(less, mid + 1, lo[act])
            hi[act] = np.where(less, hi[act], mid)
        cand = np.flatnonzero(lo < end)
        hit = cand[self._key_at(lo[cand]) == q[cand]]
        res = np.full(len(q), NO_WORD, np.uint32)
        res[hit] = np.asarray(self.words[lo[hit]]).astype(np.uint32)
        out[ok] = res
        return out

    def lookup_key(self, key):
        w = int(self.lookup_keys(np.array([key], np.uint64))[0])
        return None if w == NO_WORD else (w & 3, w >> 2)

    by_remoteness = Tablebase.by_remoteness


class SolutionDB:
    def __init__(self, root):
        tb = os.path.join(root, "stats", "0", TB_NAME)
        tk = os.path.join(root, "stats", "0", TK_NAME)
        if os.path.exists(tk) and not os.path.exists(tb):
            # a keyed tablebase (one-GPU solves of games without an index): mapped, not loaded
            with open(os.path.join(os.path.dirname(tk), "meta.json")) as f:
                self.meta = json.load(f)
            self.by, self.ranks = "key", 1
            spec = None
            params = self.meta.get("params", "").split(",")
            if "game" in self.meta and ("symmetry=1" in params or "board_symmetry=1" in params):
                from .games import GameSpec  # a symmetric table's spec is its key map
                spec = GameSpec(self.meta["game"], self.meta["params"])
            self.tablebase = KeyedTablebase(tk, spec)
            return
        if os.path.exists(tb):
            # an indexed tablebase (one-GPU solves of indexed games): mapped, not loaded
            with open(os.path.join(os.path.dirname(tb), "meta.json")) as f:
                self.meta = json.load(f)
            from .games import GameSpec
            self.by, self.ranks = "key", 1
            self.tablebase = Tablebase(tb, GameSpec(self.meta["game"], self.meta.get("params", "")))
            return
        self.tablebase = None
        ranks = sorted(glob.glob(os.path.join(root, "stats", "*", "solution.npz")))
        if not ranks:
            raise FileNotFoundError("no stats/<rank>/solution.npz under %r" % root)
        keys, names, val, rem, metas = [], [], [], [], []
        for path in ranks:
            with np.load(path) as z:  # allow_pickle stays False
                if "keys" in z.files:
                    keys.append(z["keys"].astype(np.uint64))
                else:
                    names.append(z["names"])
                val.append(z["value"].astype(np.uint8))
                rem.append(z["remoteness"].astype(np.uint32))
            with open(os.path.join(os.path.dirname(path), "meta.json")) as f:
                metas.append(json.load(f))
        if keys and names:
            raise ValueError("mixed keyed and graph tables under %r" % root)
        self.meta = metas[0]
        self.ranks = len(ranks)
        self.value = np.concatenate(val)
        self.remoteness = np.concatenate(rem)
        if keys:
            self.by = "key"
            k = np.concatenate(keys)
            order = np.argsort(k, kind="stable")
            self.keys = k[order]
            if len(self.keys) > 1 and (np.diff(self.keys) == 0).any():
                raise ValueError("a position appears in two rank files")
            self.value, self.remoteness = self.value[order], self.remoteness[order]
        else:
            self.by = "name"
            self.index = {str(n): i for i, n in enumerate(np.concatenate(names))}

    def __len__(self):
        return len(self.tablebase) if self.tablebase is not None else len(self.value)

    def lookup_key(self, key):
        if self.tablebase is not None:
            return self.tablebase.lookup_key(key)
        i = int(np.searchsorted(self.keys, np.uint64(key)))
        if i == len(self.keys) or int(self.keys[i]) != int(key):
            return None
        return int(self.value[i]), int(self.remoteness[i])

    def lookup_name(self, name):
        i = self.index.get(name)
        return None if i is None else (int(self.value[i]), int(self.remoteness[i]))

    def lookup(self, pos, spec=None):
        """(value, remoteness) of a game position, or None if unreachable."""
        if self.by == "name":
            return self.lookup_name(str(pos))
        if spec is None:
            raise ValueError("a keyed table needs the game's GameSpec")
        key = spec.key_of(pos)
        params = self.meta.get("params", "").split(",")
        if "symmetry=1" in params or "board_symmetry=1" in params:
            # a symmetric solve stored orbit representatives (gm_symmetry);
            # npz tables and both tablebase readers are looked up through here
            from .games import GameSpec
            key = int(GameSpec(spec.name, self.meta["params"]).symmetry(
                np.array([key], np.uint64))[0])
        return self.lookup_key(key)


def best_index(children):
    """Index of the best move among `children`, a list of (value,
    remoteness) in gen_moves order -- the rule of gm_solver_moves: a WIN
    parent (some child is a LOSS) takes the first LOSS child of the smallest
    remoteness; a TIE parent the first TIE child of the largest remoteness
    among TIE children; a DRAW parent the first DRAW child; a LOSS parent
    the first child of the largest remoteness.  None without children or
    with a child the table does not hold."""
    if not children or any(c is None for c in children):
        return None
    WIN, LOSS, TIE, DRAW = range(4)
    vals = [v for v, _ in children]
    if LOSS in vals:
        cand = [(r, i) for i, (v, r) in enumerate(children) if v == LOSS]
        return min(cand)[1]
    for pv in (TIE, DRAW):
        if pv in vals:
            cand = [(-r if pv == TIE else 0, i) for i, (v, r) in enumerate(children) if v == pv]
            return min(cand)[1]
    return min((-r, i) for i, (v, r) in enumerate(children))[1]


def census_of(value, remoteness, levels=None, rem_bins=None):
    """The census of a table held on the host, in gm_solver_census' layout:
    dict with by_remoteness (uint64 [rem_bins + 1, 4]: positions of remoteness
    r and value WIN / LOSS / TIE / DRAW, the last row every remoteness >=
    rem_bins) and by_level (uint64 [max level + 1, 4], or None without
    `levels`, the level of each position).  rem_bins defaults to the largest
    remoteness + 1, which leaves the overflow row empty."""
    value = np.asarray(value).astype(np.int64)
    remoteness = np.asarray(remoteness).astype(np.int64)
    if rem_bins is None:
        rem_bins = int(remoteness.max()) + 1 if len(remoteness) else 0
    by_rem = np.zeros((int(rem_bins) + 1, 4), np.uint64)
    np.add.at(by_rem, (np.minimum(remoteness, int(rem_bins)), value), 1)
    by_lev = None
    if levels is not None:
        levels = np.asarray(levels).astype(np.int64)
        by_lev = np.zeros((int(levels.max()) + 1 if len(levels) else 0, 4), np.uint64)
        np.add.at(by_lev, (levels, value), 1)
    return {"by_remoteness": by_rem, "by_level": by_lev}


def _census_table(title, rows, overflow=None):
    """One table: non-empty rows of `rows` ([n, 4]), then the totals.
    overflow: the index of a last row that collects everything from there on."""
    rows = np.asarray(rows).astype(np.uint64)
    fmt = "%12s" + " %14s" * 5
    out = [fmt % (title, "Win", "Lose", "Tie", "Draw", "Total")]
    for i, row in enumerate(rows.tolist()):
        if sum(row):
            label = ">=%d" % i if i == overflow else "%d" % i
            out.append(fmt % ((label,) + tuple(row) + (sum(row),)))
    tot = [int(x) for x in rows.sum(axis=0, dtype=np.uint64)] if len(rows) else [0] * 4
    out.append(fmt % (("Total",) + tuple(tot) + (sum(tot),)))
    return out


def format_census(by_remoteness, by_level=None):
    """The analysis table as text: remoteness x (Win Lose Tie Draw Total),
    non-empty rows only, with a totals line; then, with by_level, level x the
    same.  The last row of by_remoteness is the overflow row (census_of)."""
    lines = _census_table("Remoteness", by_remoteness, overflow=len(by_remoteness) - 1)
    if by_level is not None:
        lines.append("")
        lines.extend(_census_table("Level", by_level))
    return "\n".join(lines)


def db_census(db, spec=None, rem_bins=None):
    """census_of a SolutionDB: keyed tables get their levels from
    GameSpec.host_level, graph tables (by name) have none."""
    levels = None
    if getattr(db, "tablebase", None) is not None:
        # no inverse index: the remoteness table only, as graph tables
        return {"by_remoteness": db.tablebase.by_remoteness(rem_bins), "by_level": None}
    if db.by == "key":
        if spec is None:
            raise ValueError("a keyed table needs the game's GameSpec")
        levels = spec.host_level(db.keys)
    return census_of(db.value, db.remoteness, levels, rem_bins)


def position_moves(db, mod, pos, spec=None):
    """[(move, child position, (value, remoteness) or None)] for every legal
    move of a non-primitive position, in gen_moves order."""
    from .solver_launcher import ensure_src_utils
    utils = ensure_src_utils()  # the constants the module itself imports
    if mod.primitive(pos) != utils.UNDECIDED:
        return []
    out = []
    for mv in mod.gen_moves(pos):
        child = mod.do_move(pos, mv)
        out.append((mv, child, db.lookup(child, spec)))
    return out


def convert_to_tablebase(root, spec):
    """stats/<rank>/solution.npz of a keyed table -> stats/0/solution.gmtb
    for an indexed game, stats/0/solution.gmtk for a game without an index
    (+ "format": "gmtb" / "gmtk" in its meta.json).  The npz files stay;
    SolutionDB prefers the tablebase."""
    db = SolutionDB(root)
    if db.tablebase is not None:
        raise ValueError("%r already holds a tablebase" % root)
    if db.by != "key":
        raise ValueError("graph tables (by position name) have no index")
    from . import _lib
    from .games import GameSpec
    # the format follows the TABLE's own params, not the game file's: a
    # symmetric solve (symmetry=1 / board_symmetry=1) holds representatives
    # only and has no index, whatever the plain game has
    if "params" in db.meta:
        spec = GameSpec(db.meta.get("game", spec.name), db.meta["params"])
    try:
        space = spec.tb_index_space()
    except _lib.GmError:
        space = None  # no index function: the keyed tablebase
    words = db.value.astype(np.uint32) | (db.remoteness.astype(np.uint32) << 2)
    wb = tb_word_bytes(int(db.remoteness.max()) if len(db) else 0)
    d = os.path.join(root, "stats", "0")
    os.makedirs(d, exist_ok=True)
    meta = dict(db.meta, positions=len(db), word_bytes=wb)
    meta.pop("owned_by_rank", None)
    if space is None:
        # (game and params stay the table's own: a symmetric solve's are its key map)
        path = os.path.join(d, TK_NAME)
        meta.setdefault("game", spec.name)
        meta.setdefault("params", spec.params)
        meta.update(format="gmtk",bucket_bits=write_keyed_tablebase(path, db.keys, words, wb))
    else:
        idx = spec.tb_index(db.keys)
        if (idx == np.uint64(NO_INDEX)).any():
            raise ValueError("the table holds keys that are no position of %r" % (spec,))
        path = os.path.join(d, TB_NAME)
        meta.update(game=spec.name, params=spec.params, format="gmtb")
        write_tablebase(path, space, idx, words, wb)
    with open(os.path.join(d, "meta.json"), "w") as f:
        json.dump(meta, f, indent=1)
    return path


def open_on_gpu(db, spec=None, device=None):
    """The tablebase file of SolutionDB `db` opened on the GPU
    (Solver.open_tablebase), under the table's own game and params (a
    symmetric solve's are its key map), else `spec`."""
    if getattr(db, "tablebase", None) is None:
        raise ValueError("--gpu opens a tablebase (solution.gmtb / solution.gmtk); this directory holds "
                         "solution.npz files (convert them with --to-tablebase)")
    from .games import GameSpec
    from .solver import Solver
    if "game" in db.meta:
        spec = GameSpec(db.meta["game"], db.meta.get("params", ""))
    if spec is None:
        raise ValueError("a tablebase needs the game's GameSpec")
    return Solver.open_tablebase(spec, db.tablebase.path, device=device)


def plain_position(pos):
    """A position as the queries above spell it: nested tuples on one line
    (GameSpec.pos_of gives board games as numpy arrays)."""
    if hasattr(pos, "tolist"):
        pos = pos.tolist()
    return tuple(plain_position(p) for p in pos) if isinstance(pos, (list, tuple)) else pos


def gpu_main(args, db, mod, spec):
    """main() with --gpu: the same questions answered from the file's image
    on the device."""
    from . import _lib
    try:
        t = open_on_gpu(db, spec)
    except (ValueError, _lib.GmError) as e:
        raise SystemExit("--gpu: %s" % e)
    spec = t.spec
    if args.audit:
        a = t.audit(64)
        print("audit: %d positions, %d edges, %d mismatches" % (a["positions"], a["edges"], a["mismatches"]))
        for k in a["bad_keys"].tolist():
            print("  mismatch at %s" % (plain_position(spec.pos_of(k)),))
        return 1 if a["mismatches"] else 0
    if args.census:
        from .solver_launcher import census_report
        c = t.census(rem_bins=args.rem_bins)
        wit = [(e["count"], e["max_remoteness"], None if e["key"] is None else spec.pos_of(e["key"]))
               for e in c["extremes"]]
        print(census_report(c["by_remoteness"], c["by_level"], wit)[0])
        return 0
    todo = [ast.literal_eval(p) for p in args.positions] or [mod.initial_position()]
    keys, known = [], []
    for pos in todo:
        try:
            keys.append(spec.key_of(pos))
            known.append(True)
        except _lib.GmError:  # no key: outside the game's state space
            keys.append(_lib.GM_EMPTY_KEY)
            known.append(False)
    keys = np.array(keys, np.uint64)
    words = t.query(keys)
    children, cwords, nchild, best = t.moves(keys) if args.moves else (None, None, None, None)
    rc = 0
    for i, pos in enumerate(todo):
        w = int(words[i])
        if not known[i] or w == NO_WORD:
            print("%s: not reachable" % (pos,))
            rc = 1
            continue
        print("%s: %s in %d moves" % (pos, NAMES[w & 3], w >> 2))
        if args.moves and nchild[i]:
            for j, mv in enumerate(mod.gen_moves(pos)):
                cw = int(cwords[i, j])
                what = "not reachable" if cw == NO_WORD else "%s in %d moves" % (NAMES[cw & 3], cw >> 2)
                print("  %s -> %s: %s%s" % (mv, mod.do_move(pos, mv), what, " *" if j == int(best[i]) else ""))
                if cw == NO_WORD:
                    rc = 1
    return rc


def main(argv=None):
    ap = argparse.ArgumentParser(prog="gamesmanmpi_amd.db")
    ap.add_argument("statsdir")
    ap.add_argument("--game", required=True, help="the game file that was solved")
    ap.add_argument("--moves", action="store_true",
                    help="list every legal move of each position with the child's "
                         "value and remoteness; `*` marks the best move")
    ap.add_argument("--census", action="store_true",
                    help="print the whole solution's positions by remoteness and by level "
                         "(Win Lose Tie Draw Total per row) instead of looking positions up")
    ap.add_argument("--rem-bins", type=int, default=None, metavar="N",
                    help="--census: remoteness rows 0..N-1, then one row for the rest "
                         "(default: every remoteness its own row)")
    ap.add_argument("--to-tablebase", action="store_true",
                    help="convert the directory's solution.npz files to the indexed tablebase "
                         "stats/0/solution.gmtb (indexed games: four_to_one, sum_four_to_one, "
                         "toot_and_otto_bitstring) or, for the other descriptor games, to the keyed "
                         "tablebase stats/0/solution.gmtk, and exit")
    ap.add_argument("--gpu", action="store_true",
                    help="open the directory's tablebase (solution.gmtb / solution.gmtk) on the GPU "
                         "(Solver.open_tablebase) and answer there: queries and --moves from the device, "
                         "--census with the by-level table, --audit")
    ap.add_argument("--audit", action="store_true",
                    help="--gpu: re-derive every stored word from its children's stored words; prints the "
                         "counts and up to 64 mismatching positions, exit status 1 on a mismatch")
    ap.add_argument("positions", nargs="*")
    args = ap.parse_intermixed_args(argv)
    if args.audit and not args.gpu:
        ap.error("--audit reads the tablebase on the device: add --gpu")
    from . import _lib
    from .solver_launcher import ensure_src_utils, load_game
    ensure_src_utils()
    mod = load_game(args.game)
    if args.to_tablebase:
        from .games import spec_for_module
        spec = spec_for_module(mod, os.path.splitext(os.path.basename(args.game))[0])
        try:
            print(convert_to_tablebase(args.statsdir, spec))
        except (ValueError, _lib.GmError) as e:
            raise SystemExit("--to-tablebase: %s" % e)
        return 0
    db = SolutionDB(args.statsdir)
    spec = None
    if db.by == "key":
        from .games import spec_for_module
        spec = spec_for_module(mod, os.path.splitext(os.path.basename(args.game))[0])
    if args.gpu:
        return gpu_main(args, db, mod, spec)
    if args.census:
        c = db_census(db, spec, args.rem_bins)
        print(format_census(c["by_remoteness"], c["by_level"]))
        return 0
    todo = [ast.literal_eval(p) for p in args.positions] or [mod.initial_position()]
    rc = 0
    for pos in todo:
        try:
            r = db.lookup(pos, spec)
        except _lib.GmError:  # no key: outside the game's state space
            r = None
        if r is None:
            print("%s: not reachable" % (pos,))
            rc = 1
        else:
            print("%s: %s in %d moves" % (pos, NAMES[r[0]], r[1]))
            if args.moves:
                rows = position_moves(db, mod, pos, spec)
                best = best_index([c for _, _, c in rows])
                for i, (mv, child, c) in enumerate(rows):
                    what = "not reachable" if c is None else "%s in %d moves" % (NAMES[c[0]], c[1])
                    print("  %s -> %s: %s%s" % (mv, child, what, " *" if i == best else ""))
                    if c is None:
                        rc = 1
    return rc


if __name__ == "__main__":
    sys.exit(main())
