"""Test-only CPU yardstick for the explicit-graph retrograde (gm_graph_solve,
k_graph_round): a memoised post-order over a CSR graph in plain Python.  Not
shipped, not a fallback: the product path has only the kernel.

The reducers are restated from the reference's job loop, not from the
kernel (the order-independent reading):

  value       src/process.py:187-197 ranks the children's values LOSS 3 >
              TIE 2 > DRAW 1 > WIN 0, takes the largest and negates it
              (src/utils.py:20-29: WIN <-> LOSS, TIE and DRAW stay).
  remoteness  src/process.py:199-220, then + 1 (:254-255): where a LOSS child
              takes part the smaller remoteness wins and a WIN beside a LOSS
              is dropped, so a WIN parent counts 1 + the least remoteness of
              its LOSS children; every other pairing keeps the larger, so any
              other parent counts 1 + the largest remoteness of all its
              children.  A primitive position has remoteness 0 (:122, :243).

tests/test_graph_reference_cpu.py pins this module to the golden tables."""
WIN, LOSS, TIE, DRAW, UNDECIDED = 0, 1, 2, 3, 4
NO_WORD = 0xFFFFFFFF

_RANK = (0, 3, 2, 1)            # by value code: WIN, LOSS, TIE, DRAW
_BY_RANK = (WIN, DRAW, TIE, LOSS)
_NEGATE = (LOSS, WIN, TIE, DRAW)


class GraphCycle(ValueError):
    """The graph has a cycle: its positions never resolve."""


class NoMoves(ValueError):
    """An UNDECIDED position without moves: it never resolves either."""


def reduce_children(kids):
    """(value, remoteness) of a parent from its children's (value,
    remoteness) pairs, at least one; a child listed twice counts twice."""
    top, least_loss, most = 0, None, 0
    for v, r in kids:
        if _RANK[v] > top:
            top = _RANK[v]
        if v == LOSS and (least_loss is None or r < least_loss):
            least_loss = r
        if r > most:
            most = r
    value = _NEGATE[_BY_RANK[top]]
    return value, 1 + (least_loss if value == WIN else most)


def solve_graph(prim, offsets, children, heights=False):
    """Words (value | remoteness << 2, a list of int) of every position of
    the graph: prim[i] the primitive code of position i (UNDECIDED = 4: it has
    moves), children[offsets[i]:offsets[i + 1]] its children in move order.
    Every position is solved, reachable from position 0 or not.  Raises
    GraphCycle on a cycle and NoMoves on an UNDECIDED position without moves.
    heights=True: also each position's height (the longest path down to a
    primitive position; a round-by-round retrograde needs at most the largest
    height + 1 rounds)."""
    prim, off, ch = (a.tolist() if hasattr(a, "tolist") else [int(x) for x in a]
                     for a in (prim, offsets, children))
    n = len(prim)
    if len(off) != n + 1 or off[0] != 0 or off[n] != len(ch):
        raise ValueError("offsets do not describe %d positions and %d children" % (n, len(ch)))
    if not 0 <= min(prim) <= max(prim) <= UNDECIDED:
        raise ValueError("primitive codes are 0 .. 4")
    rem, high = [0] * n, [0] * n
    value = [p & 3 for p in prim]                                  # a primitive position: its code, remoteness 0
    state = bytearray(0 if p == UNDECIDED else 2 for p in prim)   # 0: not seen, 1: on the stack, 2: solved
    nxt = off[:n]                                                  # per position: the next child to look at
    for start in range(n):
        if state[start]:
            continue
        state[start] = 1
        stack = [start]
        while stack:
            i = stack[-1]
            j, b = nxt[i], off[i + 1]
            while j < b and state[ch[j]] == 2:
                j += 1
            nxt[i] = j
            if j < b:
                c = ch[j]
                if state[c] == 1:
                    raise GraphCycle("position %d is reached again from %d" % (c, i))
                state[c] = 1
                stack.append(c)
                continue
            a = off[i]
            if a == b:
                raise NoMoves("position %d is UNDECIDED and has no moves" % i)
            value[i], rem[i] = reduce_children([(value[c], rem[c]) for c in ch[a:b]])
            high[i] = 1 + max(high[c] for c in ch[a:b])
            state[i] = 2
            stack.pop()
    words = [v | r << 2 for v, r in zip(value, rem)]
    return (words, high) if heights else words
