"""Connect Four on a `length` x `height` board, `connect` in a row to win,
written against the reference's game-module API (README.md:28-88;
docs/source/game_modules.rst:11-33) so the reference's own solvers can load
it.  It is Toot-and-Otto without the hands: pieces drop to the lowest blank
cell of a column, X moves first, and the player who completes a line of
`connect` equal pieces (horizontal, vertical or diagonal) wins, so the
position handed to the next mover is a LOSS for that mover.

A position is a str of length*height characters from "-XO"; cell (x, y) is at
index length*y + x with y = 0 the bottom row, so str(pos) is the position
itself (as in mttt.py).  length, height and connect may be edited before
solving, like the reference games' "Feel free to edit" constants.
"""
import src.utils

length = 5
height = 4
connect = 4

BLANK, X, O = "-", "X", "O"


def initial_position():
    return BLANK * (length * height)


def _mover(pos):
    # X moves when the piece count is even
    return X if (len(pos) - pos.count(BLANK)) % 2 == 0 else O


def gen_moves(pos):
    top = length * (height - 1)
    return [x for x in range(length) if pos[top + x] == BLANK]


def do_move(pos, move):
    for y in range(height):
        i = length * y + move
        if pos[i] == BLANK:
            return pos[:i] + _mover(pos) + pos[i + 1:]
    raise ValueError("column %d is full" % move)


_lines_of = {}


def _lines():
    """The cell indices of every line of `connect` cells on the board (read
    from the constants at call time, so they may be edited after import)."""
    shape = (length, height, connect)
    if shape not in _lines_of:
        out = []
        for dx, dy in ((1, 0), (0, 1), (1, 1), (1, -1)):
            for x in range(length):
                for y in range(height):
                    ex, ey = x + (connect - 1) * dx, y + (connect - 1) * dy
                    if 0 <= ex < length and 0 <= ey < height:
                        out.append(tuple(length * (y + i * dy) + x + i * dx
                                         for i in range(connect)))
        _lines_of[shape] = out
    return _lines_of[shape]


def primitive(pos):
    # a line of either colour is looked for before fullness, as tic-tac-toe does
    for line in _lines():
        who = pos[line[0]]
        if who != BLANK and all(pos[i] == who for i in line):
            return src.utils.LOSS
    if BLANK not in pos:
        return src.utils.TIE
    return src.utils.UNDECIDED
