"""Cat and mouse: a small loopy game for the graph path (--loopy).

A WIDTH x HEIGHT board, cells numbered row by row:

     0  1 |  2  3  H        H  the hole (cell 4)
     5  6 |  7  8  9        C  the cheese (cell 10)
     C 11 | 12  B  B        B  the burrow (cells 13, 14)

The mouse moves first, then the two alternate; nobody may pass.  The mouse
steps up, down, left or right to a cell the cat is not on, and never back
to the left across the gate `|` (columns left of GATE).  The cat steps like
a king, may step onto the mouse, and is too big for the burrow.

  * the cat steps onto the mouse: the mouse, to move, has lost;
  * the mouse steps into the hole: the cat, to move, has lost;
  * the mouse steps onto the cheese: it eats and stays -- a tie.

Nothing else ends the game, and positions come back: a mouse that shuttles
between the burrow's two cells while the cat walks up and down in front of
the hole goes on forever.  Right of the gate the cheese is out of reach, so
what neither side can force there is a DRAW; left of it both can still end
the game at the cheese, and the reference ranks a TIE above a DRAW.  A
position is (mouse, cat, side to move)."""
import src.utils

WIDTH, HEIGHT = 5, 3
GATE = 2
HOLE, CHEESE = 4, 10
BURROW = (13, 14)
MOUSE_START, CAT_START = 0, 7
MOUSE, CAT = 0, 1
_ROOK = ((0, -1), (-1, 0), (1, 0), (0, 1))
_KING = _ROOK + ((-1, -1), (1, -1), (-1, 1), (1, 1))


def initial_position():
    return (MOUSE_START, CAT_START, MOUSE)


def _steps(cell, directions):
    x, y = cell % WIDTH, cell // WIDTH
    return [(y + dy) * WIDTH + x + dx for dx, dy in directions
            if 0 <= x + dx < WIDTH and 0 <= y + dy < HEIGHT]


def gen_moves(pos):
    mouse, cat, turn = pos
    if turn == MOUSE:
        return [c for c in _steps(mouse, _ROOK)
                if c != cat and not mouse % WIDTH >= GATE > c % WIDTH]
    return [c for c in _steps(cat, _KING) if c not in BURROW]


def do_move(pos, move):
    mouse, cat, turn = pos
    return (move, cat, CAT) if turn == MOUSE else (mouse, move, MOUSE)


def primitive(pos):
    mouse, cat, turn = pos
    if mouse == cat:
        return src.utils.LOSS
    if turn == CAT and mouse == HOLE:
        return src.utils.LOSS
    if turn == CAT and mouse == CHEESE:
        return src.utils.TIE
    return src.utils.UNDECIDED
