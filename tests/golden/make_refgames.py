#!/usr/bin/env python3
"""Record what the reference's own game modules answer on the playouts the
drop-in guard replays (GameSpec.verify / verify_symmetries, seed 0), so that
tests/test_launcher.py and tests/test_symmetry_cpu.py run without the
reference: tests/golden/refgames/<case>.json, read back by
tests/recorded_games.py.

Per case: the root, and for every position the guard asked about its
str(pos), primitive(pos), gen_moves(pos) (the moves themselves when they are
plain integers, else only their number) and do_move(pos, move) per move, in
the module's order; for modules with symmetry_functions(), each function's
name, order and its image of every position it was applied to; the module's
board size (length, height) where it has one.  Positions
are canonical bytes in hex (ndarray -> int8 bytes, int -> ASCII digits, str
-> ISO-8859-1).  src_utils.json holds the constants and the negate / to_str
tables of the reference's src/utils.py.  All of it is data the reference's
programs return while they run; none of their text is copied.

Needs the built library (the guard runs the descriptor on the host).

Usage:  python tests/golden/make_refgames.py --reference DIR
"""
import argparse
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)

import make_golden  # noqa: E402

OUT = os.path.join(HERE, "refgames")
SAMPLES = 150  # what the tests ask of verify / verify_symmetries

# case -> (reference game file, module overrides, GameSpec params of a second,
# symmetric replay or None)
CASES = {
    "four_to_one": ("four_to_one.py", {}, None),
    "mttt": ("mttt.py", {}, None),
    "tic_tac_toe_np": ("tic_tac_toe_np.py", {}, None),
    "toot_6x4": ("toot_and_otto_bitstring.py", {}, None),
    "toot_4x3": ("toot_and_otto_bitstring.py", {"length": 4, "height": 3}, None),
    "othello_4x4": ("othello_bit_new.py", {"length": 4, "height": 4}, "length=4,height=4,symmetry=1"),
}


def hexpos(pos):
    return make_golden.canon_bytes(pos).hex()


def kind_of(pos):
    if isinstance(pos, np.ndarray):
        return {"kind": "ndarray", "shape": list(pos.shape)}
    if isinstance(pos, (int, np.integer)):
        return {"kind": "int"}
    return {"kind": "str"}


class Recorder:
    """The module's API, every answer written down."""

    def __init__(self, mod):
        self.mod = mod
        self.rec = {"str": {}, "primitive": {}, "moves": {}, "children": {}}
        self._moves = {}
        self.rec["attrs"] = {n: int(getattr(mod, n)) for n in ("length", "height") if hasattr(mod, n)}
        for name, v in self.rec["attrs"].items():
            setattr(self, name, v)
        if hasattr(mod, "symmetry_functions"):
            self.rec["symmetries"] = []
            self.symmetry_functions = self._symmetry_functions

    def initial_position(self):
        pos = self.mod.initial_position()
        self.rec["root"] = hexpos(pos)
        self.rec["position"] = kind_of(pos)
        return pos

    def primitive(self, pos):
        p = int(self.mod.primitive(pos))
        self.rec["str"][hexpos(pos)] = str(pos)
        self.rec["primitive"][hexpos(pos)] = p
        return p

    def gen_moves(self, pos):
        moves = list(self.mod.gen_moves(pos))
        plain = all(isinstance(m, int) for m in moves)
        self.rec["moves"][hexpos(pos)] = moves if plain else len(moves)
        self.rec["children"].setdefault(hexpos(pos), [None] * len(moves))
        self._moves[hexpos(pos)] = moves
        return moves

    def do_move(self, pos, move):
        i = [j for j, m in enumerate(self._moves[hexpos(pos)]) if m is move][0]
        child = self.mod.do_move(pos, move)
        self.rec["children"][hexpos(pos)][i] = hexpos(child)
        return child

    def _symmetry_functions(self):
        out = []
        for f, order in self.mod.symmetry_functions():
            entry = {"name": f.__name__, "order": int(order), "map": {}}
            self.rec["symmetries"].append(entry)

            def g(pos, f=f, entry=entry):
                img = f(pos)
                entry["map"][hexpos(pos)] = hexpos(img)
                return img
            g.__name__ = f.__name__
            out.append((g, order))
        return out


def record_case(case):
    from gamesmanmpi_amd.games import GameSpec, spec_for_module
    fname, overrides, sym_params = CASES[case]
    stem = os.path.splitext(fname)[0]
    mod = make_golden.load_ref_game(fname, "gm_record_" + case, **overrides)
    r = Recorder(mod)
    spec = spec_for_module(r, stem)
    assert spec.verify(r, samples=SAMPLES) == SAMPLES
    if sym_params is not None:
        sym = GameSpec(stem, sym_params)
        assert sym.verify_symmetries(r, samples=SAMPLES) == SAMPLES
        assert sym.verify(r, samples=SAMPLES) == SAMPLES
    r.rec.update(case=case, game=stem, overrides=overrides)
    return r.rec


def record_utils(reference):
    import importlib.util
    spec = importlib.util.spec_from_file_location("ref_utils", os.path.join(reference, "src", "utils.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    names = ("WIN", "LOSS", "TIE", "DRAW", "UNDECIDED", "PRIMITIVES", "PRIMITIVE_REMOTENESS",
             "UNKNOWN_REMOTENESS")
    out = {"constants": {n: getattr(ref, n) for n in names},
           "STATE_MAP": sorted([int(k), v] for k, v in ref.STATE_MAP.items()),
           "negate": [ref.negate(x) for x in range(5)],
           "to_str": [ref.to_str(x) for x in range(5)]}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="the reference's checkout")
    args = ap.parse_args()
    make_golden.REF = args.reference
    os.makedirs(OUT, exist_ok=True)
    for case in CASES:
        rec = record_case(case)
        with open(os.path.join(OUT, case + ".json"), "w") as f:
            json.dump(rec, f, sort_keys=True, separators=(",", ":"))
        print(case, len(rec["primitive"]), "positions")
    with open(os.path.join(OUT, "src_utils.json"), "w") as f:
        json.dump(record_utils(args.reference), f, sort_keys=True, indent=1)


if __name__ == "__main__":
    main()
