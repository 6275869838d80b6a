"""The reference's game modules as recorded answers (tests/golden/refgames,
written by tests/golden/make_refgames.py from the reference's own files):
RecordedGame offers the game-file API (initial_position / primitive /
gen_moves / do_move, symmetry_functions where the module has them) and
answers from the recording, for exactly the positions the recording holds --
a position outside it is a KeyError, never a guess."""
import json
import os

import numpy as np

REFGAMES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "refgames")


def recorded_json(name):
    with open(os.path.join(REFGAMES, name + ".json")) as f:
        return json.load(f)


class RecordedGame:
    def __init__(self, case):
        rec = recorded_json(case)
        self._rec = rec
        self.__file__ = rec["game"] + ".py"
        self.overrides = rec["overrides"]
        for k, v in rec["attrs"].items():
            setattr(self, k, v)
        if "symmetries" in rec:
            self.symmetry_functions = self._symmetry_functions

    # positions <-> the recording's keys (canonical bytes in hex)
    def _hex(self, pos):
        kind = self._rec["position"]["kind"]
        if kind == "ndarray":
            return np.asarray(pos).astype(np.int8).tobytes().hex()
        if kind == "int":
            return str(int(pos)).encode("ascii").hex()
        return pos.encode("ISO-8859-1").hex()

    def _pos(self, hx):
        p = self._rec["position"]
        raw = bytes.fromhex(hx)
        if p["kind"] == "ndarray":
            return np.frombuffer(raw, dtype=np.int8).reshape(p["shape"]).copy()
        if p["kind"] == "int":
            return int(raw)
        return raw.decode("ISO-8859-1")

    def initial_position(self):
        return self._pos(self._rec["root"])

    def primitive(self, pos):
        hx = self._hex(pos)
        # what the reference's str(pos) was: the guard compares str(pos)
        assert str(pos) == self._rec["str"][hx], (str(pos), self._rec["str"][hx])
        return self._rec["primitive"][hx]

    def gen_moves(self, pos):
        m = self._rec["moves"][self._hex(pos)]
        return list(range(m)) if isinstance(m, int) else list(m)

    def do_move(self, pos, move):
        hx = self._hex(pos)
        m = self._rec["moves"][hx]
        i = move if isinstance(m, int) else m.index(move)
        return self._pos(self._rec["children"][hx][i])

    def _symmetry_functions(self):
        out = []
        for s in self._rec["symmetries"]:
            def f(pos, table=s["map"]):
                return self._pos(table[self._hex(pos)])
            f.__name__ = s["name"]
            out.append((f, s["order"]))
        return out
