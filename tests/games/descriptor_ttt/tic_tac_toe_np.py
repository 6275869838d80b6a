"""A tic-tac-toe game file for launcher and db tests: the game-module API
(initial_position / primitive / gen_moves / do_move) answered by the product's
own device descriptor run on the host (GameSpec.host_expand).  A position is
the board as a tuple of three rows of three small integers -- the nine int8
cells the descriptor's codec reads, in an immutable form that prints on one
line and that the db command line can take as a literal.  A move is the index
of the child in gen_moves() order.  It carries no rules of its own, so it
checks plumbing (file name -> descriptor, -sd output, db queries), not the
rules: run the launcher on it with --no-verify."""
import numpy as np

_spec = None


def _s():
    global _spec
    if _spec is None:
        from gamesmanmpi_amd.games import GameSpec
        _spec = GameSpec("tic_tac_toe_np", "")
    return _spec


def _pos(key):
    return tuple(tuple(int(c) for c in row) for row in _s().pos_of(key))


def _expand(pos):
    pr, nc, ch = _s().host_expand(np.array([_s().key_of(pos)], np.uint64))
    return int(pr[0]), [int(k) for k in ch[0, :int(nc[0])]]


def initial_position():
    return _pos(_s().root_key)


def primitive(pos):
    return _expand(pos)[0]


def gen_moves(pos):
    return list(range(len(_expand(pos)[1])))


def do_move(pos, move):
    return _pos(_expand(pos)[1][move])
