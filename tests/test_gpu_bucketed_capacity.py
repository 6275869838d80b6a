"""GPU: BUCKETED levels at the edge of their staging capacity, on one GPU and
on md5 shards (gm_bucketed_run.h, gm_bucketed_shard.h).

A level is first built count-free (children straight to provisioned regions:
256 coarse partitions of `cap` records on one GPU and in the shards' local-
dedup form, W owner regions of Emax / W records in the shards' occurrence
form) and redone counted when a region overflows.  The plan's staging (Emax >=
2^20 records) never overflows on a test-sized game, so these tests create
solvers with Solver(staging_records=N): the buffers keep the plan's sizes,
the library is told a table that ends where N staging records end, and every
byte past that end holds a canary -- an overrun changes a canary byte instead
of faulting.

N comes from CPU-side counts over the oracle's edge list (oracle/, checker
only): per level the out-edges and the fullest provisioned region (a numpy
restatement of mix64 >> 56, and spec.owners_host for the md5 owners).  A
region overflows exactly when its level total exceeds its share (every flush
reserves its run on the region's cursor, so the last reservation ends at the
total), which makes the number of redone levels predictable: each tight case
asserts on the CPU that its N redoes some levels and not others before it
touches the GPU, and afterwards that the forward launch count shows exactly
that many (a redone level costs 5 more launches than a count-free one).
Words are compared with the oracle position by position."""
import functools

import numpy as np
import pytest

from conftest import CASES

pytestmark = pytest.mark.gpu

EXACT = 128    # _lib.GM_F_BK_EXACT
LOCAL = 16384  # _lib.GM_F_BKS_LOCAL
GM_EFULL = -3
ERR_OFFSET = 40  # DevState.err: after five u64 counters at the head of the scratch
KBKC = 256


def _mix64(x):
    """gm_solver.hip mix64 (the splitmix64-style finaliser) on uint64 arrays."""
    x = np.array(x, dtype=np.uint64)
    with np.errstate(over="ignore"):
        x ^= x >> np.uint64(31)
        x *= np.uint64(0x7fb5d329728ea185)
        x ^= x >> np.uint64(27)
        x *= np.uint64(0x81dadef4bc2dd44d)
        x ^= x >> np.uint64(33)
    return x


def _cap(n):
    """A coarse partition's provisioned share of n staging records: n / 256
    rounded down to whole chunks of the chunked staging (solve_bucketed)."""
    sh = 14
    while sh > 6 and n // KBKC < (1 << sh):
        sh -= 1
    return (n // KBKC) >> sh << sh


class Graph:
    """The oracle's solved graph of one game as key arrays."""

    def __init__(self, game, params):
        from gamesmanmpi_amd.games import GameSpec
        from oracle.oracle import Game  # checker only
        self.spec = GameSpec(game, params)
        self.sol = Game(game, params).solve(1 << 23)
        try:
            pc, pl, cc, cl = self.sol.edge_list(8)
        except RuntimeError:
            pc, pl, cc, cl = self.sol.edge_list(24)
        self.pk = self.spec.encode_batch(pc, pl)  # parent key of every edge
        self.ck = self.spec.encode_batch(cc, cl)  # child key of every edge
        self.keys = np.unique(np.concatenate([np.array([self.spec.root_key], np.uint64), self.ck]))
        assert len(self.keys) == self.sol.count
        pi, ci = np.searchsorted(self.keys, self.pk), np.searchsorted(self.keys, self.ck)
        self.T = int(self.spec.max_levels)
        level = np.full(len(self.keys), -1, np.int64)
        level[np.searchsorted(self.keys, np.uint64(self.spec.root_key))] = 0
        for lv in range(self.T):  # every move advances one level
            m = level[pi] == lv
            if not m.any():
                break
            level[ci[m]] = lv + 1
        assert (level >= 0).all()
        self.level, self.pi, self.ci = level, pi, ci
        self.plev = level[pi]                                   # level of every edge's parent
        self.part = (_mix64(self.ck) >> np.uint64(56)).astype(np.int64)  # coarse partition of its child
        self.width = np.bincount(level, minlength=self.T)       # positions per level
        self.edges = np.bincount(self.plev, minlength=self.T)   # out-edges per level
        # fullest coarse partition per level
        self.fullest = np.bincount(self.plev * KBKC + self.part, minlength=self.T * KBKC).reshape(self.T, KBKC).max(1)

    # one GPU: forward launches of a solve with `redone` levels redone: the
    # count-free expand and its scan per level that holds positions and is not
    # the last, fine + dedup + scan + compact per level with children, and
    # count + two column scans + scan + the exact expand per redone level
    def base_launches(self):
        expanding = int((self.width[:self.T - 1] > 0).sum())
        return 2 * expanding + 4 * int((self.edges > 0).sum())

    def redone_levels(self, n):
        return [int(lv) for lv in range(self.T) if self.fullest[lv] > _cap(n)]

    def shards(self, world):
        """Per (shard, level): records sent per owner (occurrence form),
        the fullest coarse partition and the unique children per owner (local-
        dedup form)."""
        own = self.spec.owners_host(self.keys, world).astype(np.int64)
        po, co = own[self.pi], own[self.ci]
        T = self.T
        sent = np.bincount((po * T + self.plev) * world + co, minlength=world * T * world).reshape(world, T, world)
        coarse = np.bincount((po * T + self.plev) * KBKC + self.part,
                             minlength=world * T * KBKC).reshape(world, T, KBKC).max(2)
        pair = np.unique(po * len(self.keys) + self.ci)  # (sending shard, child) once
        pg, pc = pair // len(self.keys), pair % len(self.keys)
        uniq = np.bincount((pg * T + self.level[pc] - 1) * world + own[pc],
                           minlength=world * T * world).reshape(world, T, world)
        return {"sent": sent, "coarse": coarse, "uniq": uniq}


@functools.lru_cache(maxsize=None)
def graph(name):
    return Graph(*CASES[name])


@functools.lru_cache(maxsize=None)
def graph_of(game, params):
    return Graph(game, params)


def _fill_canary(s):
    table = s.buffers[0]
    assert 0 < s.claimed_table_bytes < table.numel()
    table[s.claimed_table_bytes:].fill_(0xA5)


def _canary_intact(s):
    s.torch.cuda.synchronize(s.device)
    tail = s.buffers[0][s.claimed_table_bytes:]
    return bool((tail == 0xA5).all().item())


def _tight(spec, n, positions, flags=0):
    from gamesmanmpi_amd.solver import Solver
    s = Solver(spec, layout="bucketed", positions=positions, flags=flags, staging_records=n, kernel_timing=True)
    _fill_canary(s)
    return s


def _assert_oracle(g, dumps):
    keys = np.concatenate([d[0] for d in dumps])
    val = np.concatenate([d[1] for d in dumps])
    rem = np.concatenate([d[2] for d in dumps])
    assert len(keys) == g.sol.count and len(np.unique(keys)) == len(keys)
    spec, sol = g.spec, g.sol
    for k, v, m in zip(keys.tolist(), val.tolist(), rem.tolist()):
        assert (v, m) == tuple(sol.lookup(spec.decode(k))), (k, v, m)


def _assert_same_table(a, b):
    """Two dumps hold the same (key, value, remoteness) rows; the order of
    the unique keys inside a bucket is the LDS hash's slot order, which a
    collision's insertion order decides, so the rows are compared by key."""
    oa, ob = np.argsort(a[0]), np.argsort(b[0])
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x[oa], y[ob])


@functools.lru_cache(maxsize=None)
def _free_checksum(name):
    """checksum() of the unconstrained bucketed solve (the plan's staging)."""
    from gamesmanmpi_amd.solver import Solver
    g = graph(name)
    s = Solver(g.spec, layout="bucketed", positions=g.sol.count, kernel_timing=True)
    r = s.solve()
    assert r.n_expand_launches == g.base_launches()  # no level redone
    return s.checksum()


def _redone(g, r):
    extra = r.n_expand_launches - g.base_launches()
    assert extra >= 0 and extra % 5 == 0, (r.n_expand_launches, g.base_launches())
    return extra // 5


# ---------------------------------------------------------------------------
# one GPU
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name,words", [("toot_4x3", True), ("othello_4x4", True), ("toot_4x4", False)])
def test_gpu_mixed_forms_one_gpu(name, words):
    """N = the widest level's out-edges: the share rounds down to at most the
    widest level's mean partition, so that level (and those near it) is
    redone while the narrow ones stay count-free.  toot 4x3 and 4x4 run the
    fixed-board / generic toot kernels, othello 4x4 the generic K_OTHELLO
    instantiation.  toot 4x4 (3.4 M positions): checksum against the golden
    fingerprint only."""
    import json
    import os
    from conftest import GOLDEN
    g = graph(name) if words else Graph(*CASES[name])  # (the large graph is not kept)
    n = int(g.edges.max())
    want = g.redone_levels(n)
    with_children = int((g.edges > 0).sum())
    assert 0 < len(want) < with_children, (n, _cap(n), g.fullest.tolist())  # the CPU-side precondition
    s = _tight(g.spec, n, g.sol.count)
    r = s.solve()
    assert _canary_intact(s)
    assert (r.positions, r.edges, r.root_line) == (g.sol.count, g.sol.edges, g.sol.root_line)
    redone = _redone(g, r)
    print("%s: N=%d cap=%d redone=%d of %d levels with children" % (name, n, _cap(n), redone, with_children))
    assert 0 < redone < with_children
    assert redone == len(want)
    if words:
        _assert_oracle(g, [s.dump()])
        assert s.checksum() == _free_checksum(name)
    else:
        e = json.load(open(os.path.join(GOLDEN, "checksums.json")))[name]
        c = s.checksum()
        assert (c["checksum"], c["positions"], c["win"], c["loss"], c["tie"]) == (
            e["checksum"], e["positions"], e["win"], e["loss"], e["tie"])


# the boards of test_gpu_edge_shapes.KEYED_SHAPES that the bucketed levels serve
# and whose widest level emits at most 1024 children (by the oracle's counts:
# 2, 8, 8, 56, 636 and 0; toot 2x4 emits 1408 and othello 4x4 16596)
SMALL_BOARDS = [
    ("toot_and_otto_bitstring", "length=1,height=1"),
    ("toot_and_otto_bitstring", "length=2,height=1"),
    ("toot_and_otto_bitstring", "length=1,height=3"),
    ("toot_and_otto_bitstring", "length=2,height=2"),
    ("toot_and_otto_bitstring", "length=3,height=2"),
    ("othello_bit_new", "length=2,height=2"),   # the root is primitive: no level has children
]


@pytest.mark.parametrize("game,params", SMALL_BOARDS)
def test_gpu_every_level_redone(game, params):
    """N = 1024, the smallest the library accepts: a partition's share is 0,
    so every level with children overflows and is redone; the same solver
    with GM_F_BK_EXACT (counted from the start) gives the identical dump."""
    g = graph_of(game, params)
    assert g.edges.max(initial=0) <= 1024  # the CPU-side precondition
    assert _cap(1024) == 0
    with_children = int((g.edges > 0).sum())
    s = _tight(g.spec, 1024, max(64, g.sol.count))
    r = s.solve()
    assert _canary_intact(s)
    assert _redone(g, r) == with_children
    d = s.dump()
    _assert_oracle(g, [d])
    x = _tight(g.spec, 1024, max(64, g.sol.count), flags=EXACT)
    x.solve()
    assert _canary_intact(x)
    _assert_same_table(d, x.dump())


@pytest.mark.parametrize("odd", [0, 1])
def test_gpu_exactly_full_and_one_short(odd):
    """N == the widest level's out-edges solves; one record fewer returns
    GM_EFULL before any kernel writes past the staging: canary intact, no
    device error bit.  With level_capacity even and odd: the arrays ahead of
    the staging are padded to 8 bytes, which the staging capacity has to
    account for (an odd level_capacity used to put the last staging array 4
    bytes past the table's end)."""
    from gamesmanmpi_amd import _lib
    g = graph("toot_4x3")
    n = int(g.edges.max())
    positions = g.sol.count + (g.sol.count + odd) % 2  # the plan adds 64 to it
    s = _tight(g.spec, n, positions)
    assert int(s.plan.level_capacity) % 2 == odd
    r = s.solve()
    assert _canary_intact(s)
    assert (r.positions, r.edges, r.root_line) == (g.sol.count, g.sol.edges, g.sol.root_line)
    _assert_oracle(g, [s.dump()])
    assert s.checksum() == _free_checksum("toot_4x3")
    t = _tight(g.spec, n - 1, positions)
    with pytest.raises(_lib.TableFull) as e:
        t.solve()
    assert e.value.code == GM_EFULL
    msg = str(e.value)
    assert "emits" in msg and "children" in msg, msg
    assert _canary_intact(t)
    err = t.buffers[2][ERR_OFFSET:ERR_OFFSET + 4].cpu().numpy().view(np.uint32)[0]
    assert err == 0


def test_gpu_redo_then_stop_and_resume():
    """A tight solve stopped just after its first redone level, and one
    stopped in the middle of the backward pass, resume to the words of the
    uninterrupted tight solve."""
    g = graph("toot_4x3")
    n = int(g.edges.max())
    want = g.redone_levels(n)
    assert want
    whole = _tight(g.spec, n, g.sol.count)
    whole.solve()
    ref = whole.dump()
    T = g.T
    for cut in (want[0] + 1, 2 * T - 1 - want[0], T + T // 2):
        s = _tight(g.spec, n, g.sol.count)
        assert s.solve_steps(0, cut) is None
        r = s.solve_steps(cut, 0)
        assert _canary_intact(s)
        assert (r.positions, r.root_line) == (g.sol.count, g.sol.root_line)
        _assert_same_table(ref, s.dump())


def test_gpu_second_solve_on_a_tight_solver():
    """The overflow flag and the partition cursors start over: a second solve
    on the same tight solver redoes the same levels and gives the same table."""
    g = graph("toot_4x3")
    n = int(g.edges.max())
    s = _tight(g.spec, n, g.sol.count)
    r0 = s.solve()
    d0 = s.dump()
    r1 = s.solve()
    assert _canary_intact(s)
    assert _redone(g, r0) == _redone(g, r1) == len(g.redone_levels(n))
    _assert_same_table(d0, s.dump())
    _assert_oracle(g, [d0])


# ---------------------------------------------------------------------------
# md5 shards
# ---------------------------------------------------------------------------
def _shard_case(world, flags):
    """(N, the (shard, level) pairs that are redone at N) for toot 4x3 on
    `world` md5 shards.  N is the largest per-shard level count -- records a
    shard sends or receives on one level -- the smallest capacity that solves.
    Occurrence form: shard g redoes level L when an owner's records exceed
    the owner region N / W.  Local-dedup form: when a coarse partition of its
    own children exceeds cap(N); the unique children per owner must fit N / W
    (that overflow is GM_EFULL by design) -- checked here."""
    g = graph("toot_4x3")
    st = g.shards(world)
    sent = st["sent"]
    if flags & LOCAL:
        n = int(sent.sum(2).max())  # a shard's own children on one level (received: unique children, fewer)
        assert st["uniq"].sum(0).max() <= n
        assert st["uniq"].max() <= n // world, (int(st["uniq"].max()), n // world)
        over = st["coarse"] > _cap(n)
    else:
        n = int(max(sent.sum(2).max(), sent.sum(0).max()))
        over = sent.max(2) > n // world
    active = sent.sum(2) > 0
    assert 0 < int(over.sum()) < int(active.sum()), (n, int(over.sum()), int(active.sum()))
    return g, n, over, active


def _shard_base_launches(g, world, flags):
    """Forward launches of the sharded solve with no (shard, level) redone
    (run_bucketed_shards documents the arithmetic)."""
    own = g.spec.owners_host(g.keys, world).astype(np.int64)
    width = np.bincount(own * g.T + g.level, minlength=world * g.T).reshape(world, g.T)
    st = g.shards(world)
    sends = st["sent"].sum(2) > 0
    n = 2 * int((width[:, :g.T - 1] > 0).sum())       # count-free expand + scan
    if flags & LOCAL:
        n += 4 * int(sends.sum())                      # fine, dedup, scan, owner binning
    n += 8 * int((width[:, 1:] > 0).sum())             # hist .. scan (7) + compact on the receiving side
    return n


@pytest.mark.parametrize("world,flags", [(3, 0), (3, LOCAL), (8, 0), (8, LOCAL)])
def test_gpu_md5_shards_mixed_forms(world, flags):
    from gamesmanmpi_amd.keyed import group_keyed_solve
    g, n, over, active = _shard_case(world, flags)  # the CPU-side precondition
    held = []

    def prepare(shards):
        held.extend(shards)
        for s in shards:
            _fill_canary(s)

    r, shards = group_keyed_solve(g.spec, world, flags=flags, staging_records=n, prepare=prepare)
    assert all(_canary_intact(s) for s in shards)
    assert (r.positions, r.edges, r.root_line) == (g.sol.count, g.sol.edges, g.sol.root_line)
    extra = r.n_expand_launches - _shard_base_launches(g, world, flags)
    print("world %d flags %d: N=%d redone=%d of %d (shard, level) pairs" % (world, flags, n, extra // 5,
                                                                           int(active.sum())))
    assert extra % 5 == 0
    assert 0 < extra // 5 < world * g.T
    assert extra // 5 == int(over.sum())
    dumps = [s.dump() for s in shards]
    for rank, d in enumerate(dumps):  # every position is read from its one owner
        if len(d[0]):
            assert (g.spec.owners_host(d[0], world) == rank).all()
    _assert_oracle(g, dumps)


@pytest.mark.parametrize("world,flags", [(3, 0), (8, LOCAL)])
def test_gpu_md5_shards_one_short(world, flags):
    """One record below the largest per-shard level count: GM_EFULL on the
    whole group, returned (no shard left waiting in an exchange), canaries
    intact."""
    from gamesmanmpi_amd import _lib
    from gamesmanmpi_amd.keyed import group_keyed_solve
    g, n, _, _ = _shard_case(world, flags)
    held = []

    def prepare(shards):
        held.extend(shards)
        for s in shards:
            _fill_canary(s)

    with pytest.raises(_lib.TableFull) as e:
        group_keyed_solve(g.spec, world, flags=flags, staging_records=n - 1, prepare=prepare)
    assert e.value.code == GM_EFULL
    assert len(held) == world and all(_canary_intact(s) for s in held)


def test_staging_records_other_layouts_refuse():
    from gamesmanmpi_amd.games import GameSpec
    from gamesmanmpi_amd.solver import Solver
    with pytest.raises(ValueError):
        Solver(GameSpec(*CASES["toot_4x3"]), layout="hashed", staging_records=4096)
