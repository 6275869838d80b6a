"""Test-only CPU yardstick for the loopy explicit-graph retrograde
(gm_graph_solve_loopy): rules A to D of DESIGN.md §7k as worklists in plain
Python.  Not shipped, not a fallback, and not the kernel's shape: the kernel
runs rounds synchronous in remoteness over a list of open positions; here
every phase takes finished words from a heap in order of remoteness and
pushes them to the parents.

  A  founded positions: a position is resolved when its last child is (a
     count of unresolved child slots per position), by
     graph_reference.reduce_children -- exactly solve_graph's word.
  B  WIN / LOSS attractor: the WIN and LOSS words leave the heap in order of
     remoteness.  A LOSS word makes every open parent WIN in one more; a WIN
     word takes one slot off each open parent's count of children that are
     not WIN yet, and the parent whose count reaches 0 is LOSS in one more
     (the word that took the last slot has the largest remoteness).
  C  TIE: the TIE words leave the heap in order of remoteness; every open
     parent is TIE in one more.
  D  the rest is DRAW in 0."""
import heapq

from graph_reference import DRAW, LOSS, TIE, UNDECIDED, WIN, NoMoves, reduce_children

NO_WORD = 0xFFFFFFFF


def solve_loopy(prim, offsets, children):
    """(words, counts): words[i] = value | remoteness << 2 of every position,
    counts = (founded, resolved by B, by C, by D).  Raises NoMoves on an
    UNDECIDED position without moves."""
    prim, off, ch = (a.tolist() if hasattr(a, "tolist") else [int(x) for x in a]
                     for a in (prim, offsets, children))
    n = len(prim)
    if len(off) != n + 1 or off[0] != 0 or off[n] != len(ch):
        raise ValueError("offsets do not describe %d positions and %d children" % (n, len(ch)))
    parents = [[] for _ in range(n)]          # one entry per child slot: a parent listed twice counts twice
    for i in range(n):
        if prim[i] == UNDECIDED and off[i] == off[i + 1]:
            raise NoMoves("position %d is UNDECIDED and has no moves" % i)
        for c in ch[off[i]:off[i + 1]]:
            parents[c].append(i)
    value, rem = [None] * n, [0] * n

    # A
    waiting = [off[i + 1] - off[i] for i in range(n)]
    work = [i for i in range(n) if prim[i] != UNDECIDED]
    for i in work:
        value[i] = prim[i]
    founded = 0
    while work:
        i = work.pop()
        founded += 1
        for p in parents[i]:
            waiting[p] -= 1
            if waiting[p] == 0:
                value[p], rem[p] = reduce_children([(value[c], rem[c]) for c in ch[off[p]:off[p + 1]]])
                work.append(p)

    # B
    not_win = [off[i + 1] - off[i] for i in range(n)]
    heap = [(rem[i], i) for i in range(n) if value[i] in (WIN, LOSS)]
    heapq.heapify(heap)
    attractor = 0
    while heap:
        r, i = heapq.heappop(heap)
        for p in parents[i]:
            if value[i] == WIN:
                not_win[p] -= 1
            if value[p] is not None:
                continue
            if value[i] == LOSS:
                value[p] = WIN
            elif not_win[p] == 0:
                value[p] = LOSS
            else:
                continue
            rem[p] = r + 1
            attractor += 1
            heapq.heappush(heap, (r + 1, p))

    # C
    heap = [(rem[i], i) for i in range(n) if value[i] == TIE]
    heapq.heapify(heap)
    ties = 0
    while heap:
        r, i = heapq.heappop(heap)
        for p in parents[i]:
            if value[p] is None:
                value[p], rem[p] = TIE, r + 1
                ties += 1
                heapq.heappush(heap, (r + 1, p))

    # D
    draws = 0
    for i in range(n):
        if value[i] is None:
            value[i], rem[i] = DRAW, 0
            draws += 1
    return [v | r << 2 for v, r in zip(value, rem)], (founded, attractor, ties, draws)


def csr(prim, kids):
    """(prim u8, offsets i64, children u32) numpy arrays from a list of codes
    and {position: [children]}."""
    import numpy as np
    deg = [len(kids.get(i, ())) for i in range(len(prim))]
    flat = [c for i in range(len(prim)) for c in kids.get(i, ())]
    return (np.asarray(prim, np.uint8), np.concatenate([[0], np.cumsum(deg)]).astype(np.int64),
            np.asarray(flat, np.uint32))


# The five hand graphs of DESIGN.md §7k: (prim, children, words, counts).
HAND_GRAPHS = [
    ([4, 4, 1], {0: [1], 1: [0, 2]}, [9, 4, 1], (1, 2, 0, 0)),
    ([4, 4, 0], {0: [1, 2], 1: [0]}, [3, 3, 0], (1, 0, 0, 2)),
    ([4, 4, 2], {0: [1], 1: [0, 2]}, [10, 6, 2], (1, 0, 2, 0)),
    # both TIE conventions: 5 is founded (1 + the largest of ALL children: 2), 0 is not (1 + the least TIE child: 1)
    ([4, 4, 2, 4, 1, 4], {0: [1, 2, 3, 5], 1: [0], 3: [4], 5: [2, 3]}, [6, 10, 2, 4, 1, 10], (4, 0, 2, 0)),
    # the trap: 0 has the founded LOSS child 2 (in 4) and the attractor LOSS child 1 (in 2): WIN in 3, not in 5
    ([4, 4, 4, 4, 4, 4, 4, 1, 4], {0: [1, 2, 3], 1: [8], 2: [4], 3: [0], 4: [5], 5: [6], 6: [7], 8: [7, 3]},
     [12, 9, 17, 17, 12, 9, 4, 1, 4], (5, 4, 0, 0)),
]
