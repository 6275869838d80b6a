"""GPU: k_graph_round / gm_graph_solve, the retrograde of game files without
a device descriptor, on synthetic graphs against tests/graph_reference.py
(the reference's reducers restated; pinned to the golden tables by
tests/test_graph_reference_cpu.py).  Every word, the counts and the root are
compared bit for bit.

The graphs are acyclic by construction (edges run to higher ids only) and
then relabelled by a random permutation that keeps the root at 0, so the
kernel's scan order is unrelated to the topological order and most rounds
read and write the same words."""
import ctypes
import re

import numpy as np
import pytest

from graph_reference import DRAW, LOSS, TIE, UNDECIDED, WIN, GraphCycle, solve_graph

pytestmark = pytest.mark.gpu
ALL = (WIN, LOSS, TIE, DRAW)


class Edges:
    """A graph under construction, ids in topological order."""

    def __init__(self, n):
        self.n = n
        self.prim = np.full(n, UNDECIDED, np.uint8)
        self.parent, self.child = [], []

    def add(self, parent, child):
        parent, child = np.atleast_1d(parent).astype(np.int64), np.atleast_1d(child).astype(np.int64)
        assert parent.shape == child.shape and (child > parent).all() and (child < self.n).all()
        self.parent.append(parent)
        self.child.append(child)

    def clear(self, j, prim=UNDECIDED):
        """Position j loses its moves and gets the code `prim`."""
        keep = [p != j for p in self.parent]
        self.parent = [p[q] for p, q in zip(self.parent, keep)]
        self.child = [c[q] for c, q in zip(self.child, keep)]
        self.prim[j] = prim

    def graph(self, rng=None):
        """The GameGraph; with rng, relabelled by a random permutation (root
        kept at 0).  A parent's children keep the order they were added in."""
        from gamesmanmpi_amd.generic import GameGraph
        n = self.n
        parent = np.concatenate(self.parent) if self.parent else np.zeros(0, np.int64)
        child = np.concatenate(self.child) if self.child else np.zeros(0, np.int64)
        perm = np.arange(n)
        if rng is not None and n > 2:
            perm[1:] = 1 + rng.permutation(n - 1)
        prim = np.empty(n, np.uint8)
        prim[perm] = self.prim
        order = np.argsort(perm[parent], kind="stable")
        deg = np.bincount(perm[parent], minlength=n)
        assert (deg[prim != UNDECIDED] == 0).all()
        offsets = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
        return GameGraph([str(i) for i in range(n)], prim, offsets, perm[child][order].astype(np.uint32))


def random_dag(rng, n, mean_degree=3, window=None, leaves=0.3, codes=ALL, dup=0.0):
    """n positions; a position is primitive with probability `leaves` (its
    code drawn from `codes`), else it has 1 .. 2 mean_degree - 1 children
    among the next `window` ids (default: all higher ids).  dup: that share of
    the edges is listed 2..5 times."""
    e = Edges(n)
    leaf = rng.random(n) < leaves
    leaf[0], leaf[n - 1] = n == 1, True
    e.prim[leaf] = rng.choice(np.array(codes, np.uint8), int(leaf.sum()))
    deg = np.where(leaf, 0, rng.integers(1, 2 * mean_degree, n))
    parent = np.repeat(np.arange(n), deg)
    room = n - 1 - parent
    if window:
        room = np.minimum(room, window)
    child = parent + 1 + (rng.random(len(parent)) * room).astype(np.int64)
    if dup:
        times = np.where(rng.random(len(parent)) < dup, rng.integers(2, 6, len(parent)), 1)
        parent, child = np.repeat(parent, times), np.repeat(child, times)
    if len(parent):
        e.add(parent, child)
    return e


def gpu_solve(g):
    from gamesmanmpi_amd.generic import GenericSolver
    s = GenericSolver(g)
    return s.solve(), s.words


def check(g, root=None):
    """Solve g on the GPU and compare everything with the reference module;
    returns (result, words u32, heights)."""
    want, high = solve_graph(g.prim, g.offsets, g.children, heights=True)
    want = np.array(want, np.uint32)
    r, words = gpu_solve(g)
    np.testing.assert_array_equal(words, want)
    assert (r.positions, r.edges, r.primitives) == (g.n, len(g.children), int((g.prim != UNDECIDED).sum()))
    assert (r.root_value, r.root_remoteness) == (int(want[0] & 3), int(want[0] >> 2))
    if root is not None:
        assert r.root_value == root
    # after round k every position of height < k is resolved, whatever else
    # the round picked up from words written earlier in the same launch
    assert 1 <= r.levels <= max(high) + 1 and r.n_resolve_launches == r.levels
    return r, want, np.array(high)


def kids(g, i):
    return g.children[g.offsets[i]:g.offsets[i + 1]].astype(np.int64)


@pytest.mark.parametrize("code", ALL)
def test_one_primitive_position(code):
    e = Edges(1)
    e.prim[0] = code
    r, w, _ = check(e.graph(), root=code)
    assert (r.root_remoteness, r.levels, r.edges, r.primitives) == (0, 1, 0, 1)


@pytest.mark.parametrize("codes,root", [((WIN, WIN, WIN), LOSS), ((WIN, LOSS, TIE, DRAW), WIN),
                                        ((WIN, TIE, DRAW, TIE), TIE), ((DRAW, WIN, DRAW), DRAW)])
def test_root_of_primitive_children(codes, root):
    e = Edges(1 + len(codes))
    e.prim[1:] = codes
    e.add(np.zeros(len(codes), np.int64), 1 + np.arange(len(codes)))
    r, _, _ = check(e.graph(np.random.default_rng(1)), root=root)
    assert (r.root_remoteness, r.levels) == (1, 2)


@pytest.mark.parametrize("n", [255, 256, 257])
def test_sizes_around_one_block(n):
    """n around kBlock = 256: a last block of 255 threads past the end, an
    exact block, a second block of one position."""
    rng = np.random.default_rng(n)
    check(random_dag(rng, n).graph(rng))


# seeds chosen on the CPU (the reference module) so that the four graphs give
# the root the four values; the assertion keeps them honest
@pytest.mark.parametrize("seed,root", [(0, WIN), (1, LOSS), (2, TIE), (31, DRAW)])
def test_all_primitive_codes_and_every_root_value(seed, root):
    rng = np.random.default_rng(seed)
    g = random_dag(rng, 3000, window=40, dup=0.05).graph(rng)
    _, w, _ = check(g, root=root)
    assert set((w & 3).tolist()) == set(ALL) and set(g.prim[g.prim != UNDECIDED].tolist()) == set(ALL)


def test_more_positions_than_one_grid_stride_pass():
    """n = 600,000 with mean degree 3: gm_graph_solve launches at most
    launch_grid() = 8 blocks per compute unit, of kBlock = 256 threads each
    -- 524,288 threads on the 256 compute units of an MI355X -- so 75,712
    threads walk a second position and the `i += gridDim.x * blockDim.x`
    stride is exercised.  (The plain-Python reference takes about 3 s on
    this many positions: the size is the smallest round one past the grid;
    the device's compute-unit count is checked, not assumed.)"""
    import torch
    n = 600_000
    assert n > torch.cuda.get_device_properties(0).multi_processor_count * 8 * 256
    rng = np.random.default_rng(20)
    g = random_dag(rng, n, mean_degree=4, leaves=0.25, window=1 << 13).graph(rng)
    assert 2.9 < len(g.children) / g.n < 3.1
    r, w, _ = check(g)
    assert r.positions == n and set((w & 3).tolist()) == set(ALL)


def test_tie_parents_with_longer_win_children():
    """TIE parents whose WIN children lie deeper than their TIE children:
    the remoteness is 1 + the largest over ALL children, not
    over the TIE children.  Built on purpose (a TIE leaf beside the WIN end of
    a chain) and counted in a random graph as well."""
    rng = np.random.default_rng(7)
    m = 40
    base = random_dag(rng, 2000, window=30, codes=(WIN, TIE, TIE, DRAW, LOSS))
    e = Edges(base.n + 2 * m)
    e.prim[:base.n] = base.prim
    e.prim[base.n:] = TIE
    e.parent, e.child = list(base.parent), list(base.child)
    # a chain c0 .. c0 + m - 1 that ends in a primitive LOSS: the position at distance d from the end is a WIN
    # in d for odd d; the positions after the chain are TIE leaves
    c0 = base.n
    e.prim[c0:c0 + m - 1] = UNDECIDED
    e.prim[c0 + m - 1] = LOSS
    e.add(np.arange(c0, c0 + m - 1), np.arange(c0 + 1, c0 + m))
    made = []
    for k, j in enumerate(range(c0 - 41, c0 - 1, 2)):  # 20 positions of the random part get new moves:
        e.clear(j)
        e.add([j, j], [c0 + m + k, c0 + m - 2 - 2 * k])  # a TIE leaf, then a WIN in 1 + 2k
        made.append((j, 2 + 2 * k))
    g = e.graph(None)
    _, w, _ = check(g)
    for j, rem in made:
        assert w[j] == (TIE | rem << 2)
    rng2 = np.random.default_rng(8)
    g = e.graph(rng2)
    _, w, _ = check(g)
    val, rem = w & 3, w >> 2
    n_found = 0
    for i in np.flatnonzero((val == TIE) & (g.prim == UNDECIDED)):
        c = kids(g, i)
        ties, wins = rem[c][val[c] == TIE], rem[c][val[c] == WIN]
        n_found += bool(len(ties) and len(wins) and wins.max() > ties.max())
    assert n_found >= 20


def test_draw_beside_tie_children():
    """Parents with DRAW and TIE children (and no LOSS child) are TIE; with
    DRAW and WIN children only, DRAW."""
    rng = np.random.default_rng(11)
    g = random_dag(rng, 4000, window=50, leaves=0.4, codes=(TIE, DRAW, DRAW, WIN)).graph(rng)
    _, w, _ = check(g)
    val = w & 3
    both = draws = 0
    for i in np.flatnonzero(g.prim == UNDECIDED):
        v = set(val[kids(g, i)].tolist())
        if {TIE, DRAW} <= v and LOSS not in v:
            assert val[i] == TIE
            both += 1
        if DRAW in v and not v & {TIE, LOSS}:
            assert val[i] == DRAW
            draws += 1
    assert both >= 50 and draws >= 50


def test_duplicate_children():
    """The same child listed 2..5 times by a third of the edges: the words do
    not change, the edge count does."""
    rng = np.random.default_rng(13)
    e = random_dag(rng, 3000, window=60, dup=0.35)
    g = e.graph(rng)
    dups = sum(len(c) - len(set(c.tolist())) for c in (kids(g, i) for i in range(g.n)))
    assert dups > 1000
    r, _, _ = check(g)
    _, w, _ = check(e.graph(None))
    # the same graph with every child listed once
    once = Edges(e.n)
    once.prim = e.prim
    pc = np.unique(np.stack([np.concatenate(e.parent), np.concatenate(e.child)]), axis=1)
    once.add(pc[0], pc[1])
    r1, w1, _ = check(once.graph(None))
    assert r1.edges == r.edges - dups
    np.testing.assert_array_equal(w, w1)


def test_wide_positions():
    """One position with 300 children and one with 65: more than a wave has
    lanes, and one more than a wave."""
    rng = np.random.default_rng(17)
    e = random_dag(rng, 2500, window=400, leaves=0.35)
    for j, width in ((3, 300), (700, 65)):
        e.clear(j)
        e.add(np.full(width, j), j + 1 + rng.choice(1500, width, replace=False))
    e.add([0], [3])
    g = e.graph(rng)
    widths = np.diff(g.offsets)
    assert sorted(widths.tolist())[-2:] == [65, 300]
    check(g)


def test_deep_chain_with_side_branches():
    """A chain 3,000 deep, every position of it with side branches into a
    random graph of TIE and DRAW leaves (so no WIN cuts the count short: the
    remoteness is the height), and below the root a second, bare chain of
    3,000 alternating WIN / LOSS positions: thousands of rounds, remoteness
    past 2,047 (11 bits) for three of the values, on positions the scan meets
    in no particular order.

    The rounds: a round resolves at least the positions whose children were
    resolved before it, so height + 1 rounds always suffice; a round may also
    pick up words written earlier in the same launch, so fewer can do.  The
    figure is printed and bounded from above; no lower bound holds in
    general."""
    rng = np.random.default_rng(19)
    depth, n = 3000, 9000
    base = random_dag(rng, n, window=25, leaves=0.35, codes=(TIE, DRAW))
    e = Edges(n + depth)
    e.prim[:n] = base.prim
    e.parent, e.child = list(base.parent), list(base.child)
    # the first chain: positions 0, 2, 4, ..; each keeps its random children too
    chain = 2 * np.arange(depth + 1)
    e.prim[chain[:-1]] = UNDECIDED
    e.clear(chain[-1], LOSS)
    e.add(chain[:-1], chain[1:])
    # the second: positions n .. n + depth - 1, entered from the root
    e.prim[n + depth - 1] = LOSS
    e.add(np.arange(n, n + depth - 1), np.arange(n + 1, n + depth))
    e.add([0], [n])
    g = e.graph(rng)
    r, w, high = check(g)
    val, rem = w & 3, w >> 2
    print("chain: height %d, rounds %d, largest remoteness %s" % (
        high.max(), r.levels, [int(rem[val == v].max()) for v in (WIN, LOSS, TIE)]))
    assert high[0] >= depth
    assert min(rem[val == v].max() for v in (WIN, LOSS, TIE)) > 2047


# ---- errors -----------------------------------------------------------------
def test_undecided_leaf_is_an_error():
    from gamesmanmpi_amd import _lib
    rng = np.random.default_rng(23)
    e = random_dag(rng, 5000, window=50)
    leaf = int(np.flatnonzero(e.prim != UNDECIDED)[-7])
    e.prim[leaf] = UNDECIDED
    with pytest.raises(_lib.GmError, match="non-primitive-without-moves") as err:
        gpu_solve(e.graph(rng))
    assert err.value.code == _lib.GM_ECORRUPT


def test_cycle_inside_a_large_graph():
    """One back edge in a 20,000-position graph: the positions of the cycle
    and everything above them never resolve, and are counted."""
    from gamesmanmpi_amd import _lib
    rng = np.random.default_rng(29)
    n = 20000
    e = random_dag(rng, n, window=200)
    g = e.graph(rng)
    # close a cycle: a child of position a gets a as a further child
    a, b = next((i, int(c)) for i in range(5000, n) if g.prim[i] == UNDECIDED
                for c in kids(g, i) if g.prim[c] == UNDECIDED)
    children = np.insert(g.children, g.offsets[b + 1], a)
    offsets = g.offsets.copy()
    offsets[b + 1:] += 1
    with pytest.raises(GraphCycle):
        solve_graph(g.prim, offsets, children)
    # unresolved: whatever reaches a (b does, through a)
    parents = np.repeat(np.arange(n), np.diff(offsets))
    stuck = np.zeros(n, bool)
    stuck[a] = True
    while True:
        more = np.zeros(n, bool)
        more[parents[stuck[children]]] = True
        more &= ~stuck
        if not more.any():
            break
        stuck |= more
    assert stuck[b] and 2 <= stuck.sum() < n
    from gamesmanmpi_amd.generic import GameGraph, GenericSolver
    with pytest.raises(_lib.GmError, match="never resolve") as err:
        GenericSolver(GameGraph(g.names, g.prim, offsets, children)).solve()
    assert err.value.code == _lib.GM_ECORRUPT
    got = re.search(r"(\d+) of (\d+) positions never resolve", str(err.value))
    assert (int(got.group(1)), int(got.group(2))) == (int(stuck.sum()), n)


@pytest.mark.parametrize("root", [3, 4, 1 << 40])
def test_root_outside_the_graph_is_refused(root):
    """gm_graph_solve with root >= n (GenericSolver always passes 0)."""
    import torch
    from gamesmanmpi_amd import _lib
    dev = torch.device("cuda")
    prim = torch.tensor([UNDECIDED, WIN, LOSS], dtype=torch.uint8, device=dev)
    offsets = torch.tensor([0, 2, 2, 2], dtype=torch.int64, device=dev)
    children = torch.tensor([1, 2], dtype=torch.int32, device=dev)
    words = torch.full((3,), 0x55, dtype=torch.int32, device=dev)
    scratch = torch.zeros(4096, dtype=torch.uint8, device=dev)
    r = _lib.gm_result()

    def call(root):
        return _lib.load().gm_graph_solve(prim.data_ptr(), offsets.data_ptr(), children.data_ptr(), 3, root,
                                          words.data_ptr(), scratch.data_ptr(),
                                          torch.cuda.current_stream(dev).cuda_stream, ctypes.byref(r))
    assert call(root) == _lib.GM_EINVAL
    torch.cuda.synchronize(dev)
    assert (words.cpu().numpy() == 0x55).all()  # nothing ran
    assert call(2) == 0 and (r.root_value, r.root_remoteness) == (LOSS, 0)  # the last position is a root
    assert call(0) == 0 and (r.root_value, r.root_remoteness) == (WIN, 1)
