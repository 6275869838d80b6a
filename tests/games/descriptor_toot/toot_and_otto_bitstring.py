"""A toot-and-otto game file for launcher tests, 3 x 3: the game-module API
(initial_position / primitive / gen_moves / do_move) answered by the product's
own device descriptor run on the host (GameSpec.host_expand), positions being
the latin-1 bitstrings the descriptor's codec gives.  A move is the index of
the child in gen_moves() order.  It carries no rules of its own, so it checks
plumbing (file name -> descriptor, -sd output, db queries), not the rules:
run the launcher on it with --no-verify."""
import numpy as np

length, height = 3, 3
area = length * height

_spec = None


def _s():
    global _spec
    if _spec is None:
        from gamesmanmpi_amd.games import GameSpec
        _spec = GameSpec("toot_and_otto_bitstring", "length=%d,height=%d" % (length, height))
    return _spec


def _expand(pos):
    pr, nc, ch = _s().host_expand(np.array([_s().key_of(pos)], np.uint64))
    return int(pr[0]), [int(k) for k in ch[0, :int(nc[0])]]


def initial_position():
    return _s().pos_of(_s().root_key)


def primitive(pos):
    return _expand(pos)[0]


def gen_moves(pos):
    return list(range(len(_expand(pos)[1])))


def do_move(pos, move):
    return _s().pos_of(_expand(pos)[1][move])
