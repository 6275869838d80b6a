"""The RANKED index of connect four (csrc/gm_ranked_connect.h) on the host:
gm_ranked_slots and gm_plan(GM_F_RANKED) against the index written out again
here in Python -- height vectors level by level in ascending hvcode order
(hvcode = sum h_x (H+1)^x), a block of 2^L slots per height vector addressed
by the stack bits (bit off_x + y = 1: the piece at (x, y) is X, off_x =
sum_{c<x} h_c), levels padded to 512 slots, a slot a position iff it holds
ceil(L / 2) X pieces.  No GPU and no table: the arithmetic alone, up to 6x5
where slots pass 2^32."""
import ctypes
import functools
import itertools
import random

import numpy as np
import pytest

from test_connect_four_cpu import c4_params, c4_table, py_key

NO_INDEX = 0xFFFFFFFFFFFFFFFF


def spec_of(board, extra=""):
    from gamesmanmpi_amd.games import GameSpec
    return GameSpec("connect_four", c4_params(*board) + extra)


@functools.lru_cache(maxsize=None)
def py_index(C, H):
    """(block base per height vector, first slot per level, total slots)."""
    by_level = {}
    for hv in itertools.product(range(H + 1), repeat=C):
        code = sum(h * (H + 1) ** x for x, h in enumerate(hv))
        by_level.setdefault(sum(hv), []).append((code, hv))
    base, lvstart, at = {}, [], 0
    for L in range(C * H + 1):
        lvstart.append(at)
        for j, (_, hv) in enumerate(sorted(by_level[L])):
            base[hv] = at + (j << L)
        at += ((len(by_level[L]) << L) + 511) // 512 * 512
    return base, lvstart, at


def py_stacks(key, C, H):
    """(heights, stack bits, level) of a gravity board's key, or None."""
    A = C * H
    if key >> (2 * A):
        return None
    xs, os_ = key & ((1 << A) - 1), key >> A
    if xs & os_:
        return None
    hv, bits, L = [], 0, 0
    for x in range(C):
        col = [((xs | os_) >> (C * y + x)) & 1 for y in range(H)]
        h = sum(col)
        if col != [1] * h + [0] * (H - h):
            return None
        for y in range(h):
            bits |= ((xs >> (C * y + x)) & 1) << (L + y)
        hv.append(h)
        L += h
    if bin(bits).count("1") != (L + 1) // 2:
        return None
    return tuple(hv), bits, L


def py_slot(key, C, H):
    st = py_stacks(key, C, H)
    if st is None:
        return NO_INDEX, 0xFFFFFFFF
    hv, bits, L = st
    return py_index(C, H)[0][hv] + bits, L


def plan(spec, flags):
    from gamesmanmpi_amd import _lib
    p = _lib.gm_plan_t()
    rc = _lib.load().gm_plan(spec.id, 0, flags, 0, ctypes.byref(p))
    return rc, p


def board_key(C, H, columns):
    """columns: per column a string of X / O from the bottom up."""
    cells = ["-"] * (C * H)
    for x, col in enumerate(columns):
        for y, c in enumerate(col):
            cells[C * y + x] = c
    return py_key("".join(cells))


def test_slots_of_every_4x4_position():
    from gamesmanmpi_amd import _lib
    t = c4_table("4x4_4")
    spec = spec_of((4, 4, 4))
    assert len(t["keys"]) == 161029
    slots, levels = spec.ranked_slots(t["keys"])
    rc, p = plan(spec, _lib.GM_F_RANKED)
    assert rc == 0 and p.mode == _lib.GM_MODE_RANKED
    assert len(np.unique(slots)) == len(slots) and int(slots.max()) < p.table_slots
    pop = np.array([bin(int(k)).count("1") for k in t["keys"]], np.uint32)
    np.testing.assert_array_equal(levels, pop)
    np.testing.assert_array_equal(levels, t["level"])
    want = np.array([py_slot(int(k), 4, 4)[0] for k in t["keys"]], np.uint64)
    np.testing.assert_array_equal(slots, want)


NON_POSITIONS_4x4 = {
    "a floating piece": py_key("----" "X---" + "-" * 8),
    "an X / O overlap": py_key("X---" + "-" * 12) | py_key("O---" + "-" * 12),
    "two more X than O": py_key("XX--" + "-" * 12),
    "a bit above 2A": py_key("X---" + "-" * 12) | 1 << 32,
}


@pytest.mark.parametrize("what", sorted(NON_POSITIONS_4x4))
def test_non_positions_have_no_slot(what):
    key = NON_POSITIONS_4x4[what]
    slots, levels = spec_of((4, 4, 4)).ranked_slots(np.array([key, 0], np.uint64))
    assert int(slots[0]) == NO_INDEX and int(levels[0]) == 0xFFFFFFFF
    assert (int(slots[1]), int(levels[1])) == (0, 0)  # the empty board beside it
    assert py_slot(key, 4, 4)[0] == NO_INDEX


def test_6x5_slots_pass_2_32():
    C, H = 6, 5
    rnd = random.Random(65)

    def filled(heights):
        """a balanced colouring of the stacks: X on ceil(L / 2) random cells"""
        L = sum(heights)
        xs = set(rnd.sample(range(L), (L + 1) // 2))
        cols, at = [], 0
        for h in heights:
            cols.append("".join("X" if at + y in xs else "O" for y in range(h)))
            at += h
        return board_key(C, H, cols)

    heights = [(5,) * 6, (0,) * 6, (5, 5, 5, 5, 4, 0), (4, 4, 4, 4, 4, 4), (5, 5, 5, 5, 5, 0), (5, 4, 5, 4, 5, 3),
               (3, 5, 5, 5, 5, 4), (5, 5, 5, 5, 3, 5), (1, 5, 5, 5, 5, 5), (5, 5, 4, 5, 5, 4)]
    assert {sum(h) for h in heights} >= {0, 24, 25, 26, 27, 28, 30}
    keys = np.array([filled(h) for h in heights], np.uint64)
    slots, levels = spec_of((C, H, 4)).ranked_slots(keys)
    want = [py_slot(int(k), C, H) for k in keys]
    assert slots.tolist() == [w[0] for w in want]
    assert levels.tolist() == [w[1] for w in want] == [sum(h) for h in heights]
    base, lvstart, total = py_index(C, H)
    assert total >= 63 ** 6 and int(slots[0]) > 1 << 32 and int(slots.max()) < total
    # a level wider than 2^32 slots, and slots of it more than 2^32 apart
    widths = np.diff(lvstart + [total])
    assert int(widths.max()) > 1 << 32


def test_child_slot_arithmetic_on_5x4():
    """slot(child) = child block base + the parent's stack bits with the
    mover's colour bit inserted at off_x + h_x."""
    C, H = 5, 4
    spec = spec_of((C, H, 4))
    base, _, _ = py_index(C, H)
    rnd = random.Random(54)
    keys = []
    while len(keys) < 200:  # random playouts from the root: reachable positions
        k = 0
        for _ in range(rnd.randrange(C * H)):
            pr, nc, ch = spec.host_expand(np.array([k], np.uint64))
            if nc[0] == 0:
                break
            k = int(ch[0, rnd.randrange(int(nc[0]))])
        keys.append(k)
    keys = np.array(keys, np.uint64)
    pr, nc, ch = spec.host_expand(keys)
    checked = 0
    for i, k in enumerate(keys):
        hv, bits, L = py_stacks(int(k), C, H)
        open_cols = [x for x in range(C) if hv[x] < H]
        if nc[i] == 0:
            continue
        assert int(nc[i]) == len(open_cols)
        got, lv = spec.ranked_slots(ch[i, :nc[i]])
        for x, slot, cl in zip(open_cols, got.tolist(), lv.tolist()):
            q = sum(hv[:x]) + hv[x]
            colour = 1 if L % 2 == 0 else 0  # X moves at even levels
            cbits = (bits & ((1 << q) - 1)) | (colour << q) | ((bits >> q) << (q + 1))
            chv = hv[:x] + (hv[x] + 1,) + hv[x + 1:]
            assert slot == base[chv] + cbits and cl == L + 1
            checked += 1
    assert checked > 400


def test_plan():
    from gamesmanmpi_amd import _lib
    from gamesmanmpi_amd.games import GameSpec
    L = _lib.load()
    spec = spec_of((5, 4, 4))
    rc, p = plan(spec, _lib.GM_F_RANKED)
    assert rc == 0 and p.mode == _lib.GM_MODE_RANKED and p.table_slots == py_index(5, 4)[2]
    rc, p = plan(spec, 0)
    assert rc == 0 and p.mode == _lib.GM_MODE_BUCKETED
    rc, p = plan(spec_of((5, 4, 4), ",board_symmetry=1"), _lib.GM_F_RANKED)
    assert rc == _lib.GM_EINVAL and b"board_symmetry=1 has no ranked layout" in L.gm_last_error()
    # md5 shards of this layout are out of scope
    p = _lib.gm_plan_t()
    assert L.gm_plan_keyed_shard(spec.id, 0, 2, 0, _lib.GM_F_RANKED_SHARD, 0, ctypes.byref(p)) == _lib.GM_EINVAL
    # 6x5 plans (11 bits a slot), 7x5 passes 2^36 slots
    rc, p = plan(spec_of((6, 5, 4)), _lib.GM_F_RANKED)
    assert rc == 0 and p.table_slots == py_index(6, 5)[2] and p.table_bytes < 88e9
    rc, p = plan(spec_of((7, 4, 4)), _lib.GM_F_RANKED)
    assert rc == 0 and p.mode == _lib.GM_MODE_RANKED
    rc, p = plan(spec_of((5, 6, 4)), _lib.GM_F_RANKED)
    assert rc == 0 and p.table_slots == py_index(5, 6)[2]
    rc, p = plan(spec_of((4, 7, 4)), _lib.GM_F_RANKED)
    assert rc == 0  # H = 7 is the tallest board
    # toot-and-otto plans as before, with and without the flag
    toot = GameSpec("toot_and_otto_bitstring", "length=4,height=3")
    r0, p0 = plan(toot, 0)
    r1, p1 = plan(toot, _lib.GM_F_RANKED)
    assert r0 == r1 == 0 and p0.mode == p1.mode == _lib.GM_MODE_RANKED
    assert (p0.table_slots, p0.table_bytes, p0.scratch_bytes) == (p1.table_slots, p1.table_bytes, p1.scratch_bytes)
    # a game without the layout ignores the flag
    ttt = GameSpec("tic_tac_toe_np")
    assert plan(ttt, _lib.GM_F_RANKED)[1].mode == plan(ttt, 0)[1].mode


def test_toot_slots_are_its_tablebase_indexes():
    """gm_ranked_slots serves toot-and-otto too: its RANKED slot is gm_tb_index's."""
    from gamesmanmpi_amd import _lib
    from gamesmanmpi_amd.games import GameSpec
    toot = GameSpec("toot_and_otto_bitstring", "length=4,height=3")
    rnd = random.Random(43)
    keys = [toot.root_key]
    for _ in range(100):  # random playouts
        k = toot.root_key
        for _ in range(rnd.randrange(1, 13)):
            pr, nc, ch = toot.host_expand(np.array([k], np.uint64))
            if nc[0] == 0:
                break
            k = int(ch[0, rnd.randrange(int(nc[0]))])
        keys.append(k)
    keys = np.array(keys + [toot.root_key ^ 1], np.uint64)  # (and a key that is no position)
    slots, levels = toot.ranked_slots(keys)
    np.testing.assert_array_equal(slots, toot.tb_index(keys))
    assert int(slots[-1]) == NO_INDEX and int(slots[:-1].max()) < toot.tb_index_space()
    assert levels[:-1].tolist() == [bin(int(k) & ((1 << 24) - 1)).count("1") for k in keys[:-1]]
    with pytest.raises(_lib.GmError):
        GameSpec("tic_tac_toe_np").ranked_slots(np.zeros(1, np.uint64))
