"""The registry's host answers are pinned: for every descriptor the tests and
the benchmark use, what gm_game_lookup / gm_game_info / gm_root /
gm_symmetry_count / gm_tb_info / gm_plan answer (or refuse, with code and
text) equals tests/golden/registry/abi_answers.json, recorded from the
library before the game kinds got one dispatch and one registry
(csrc/gm_games.h, csrc/gm_registry.h).  No kernel is launched here.

    python tests/test_registry_host.py --record     rewrites the file
"""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ANSWERS = os.path.join(ROOT, "tests", "golden", "registry", "abi_answers.json")

SUMS = ["0", "0:0", "0:7", "5:0", "1:1:1", "2:5:7", "2:5:0:6", "3:3:3", "3:7:7:7", "4:4:4", "4:6:3", "6:6:6:6",
        "6:9:4:11", "7:7", "7:7:7", "7:7:7:7", "7:7:7:15", "7:7:7:7:7", "15:15", "15:15:15:15", "15:15:15:15:7",
        "15:15:15:15:15", "15:15:15:15:31", "31:31", "31:31:3", "31:31:3:15", "31:31:1:127", "31:31:7:7:15",
        "31:31:9:6:3", "31:31:191", "31:31:192", "31:31:443", "31:31:444", "31:31:31:63", "31:31:31:31:31:31",
        "31:31:31:31:31:63", "31:31:31:31:31:127", "31:31:31:31:31:255", "31:63:31:31:31:31",
        "31:127:31:31:31:31", "31:255:31:31:31:31", "127:127:7"]
TOOT = [(1, 1), (1, 3), (2, 1), (2, 2), (2, 4), (3, 2), (3, 3), (3, 4), (4, 3), (4, 4), (5, 4), (6, 4)]
CONNECT = [(2, 2, 2), (3, 2, 3), (1, 4, 4), (4, 1, 4), (3, 3, 3), (4, 3, 3), (4, 4, 3), (4, 4, 4), (5, 4, 4),
           (6, 5, 4), (6, 6, 4), (4, 4, 5)]


def descriptors():
    out = [("four_to_one", "")] + [("four_to_one", "start=%d" % n) for n in (0, 1, 2, 3, 4, 20, 40, 64, 300, 3000)]
    out += [("sum_four_to_one", "heaps=" + h) for h in SUMS]
    for sym in ("", ",board_symmetry=1"):
        out += [("tic_tac_toe_np", sym[1:]), ("mttt", sym[1:])]
        out += [("toot_and_otto_bitstring", sym[1:])]
        out += [("toot_and_otto_bitstring", "length=%d,height=%d%s" % (l, h, sym)) for l, h in TOOT]
        out += [("othello_bit_new", "length=%d,height=%d%s" % (n, n, sym)) for n in (2, 4)]
        out += [("connect_four", sym[1:])]
        out += [("connect_four", "length=%d,height=%d,connect=%d%s" % (l, h, k, sym)) for l, h, k in CONNECT]
    out += [("othello_bit_new", "length=4,height=4,symmetry=1"), ("othello_bit_new", "length=2,height=2,symmetry=1")]
    # one parameter set per refusal of the descriptor builder
    out += [("four_to_one", "start=-1"), ("sum_four_to_one", ""), ("sum_four_to_one", "heaps=" + ":".join(["1"] * 17)),
            ("sum_four_to_one", "heaps=3:-2"), ("sum_four_to_one", "heaps=3:2000000000"), ("sum_four_to_one", "heaps="),
            ("sum_four_to_one", "heaps=" + ":".join(["65535"] * 4)),
            ("sum_four_to_one", "heaps=1073741824:1073741824"),
            ("toot_and_otto_bitstring", "length=6,height=5"), ("toot_and_otto_bitstring", "length=0,height=4"),
            ("othello_bit_new", "length=4,height=3"), ("othello_bit_new", "length=6,height=6"),
            ("othello_bit_new", "length=1,height=1"), ("othello_bit_new", "length=3,height=3,board_symmetry=1"),
            ("connect_four", "length=7,height=6,connect=4"), ("connect_four", "length=9,height=3,connect=4"),
            ("connect_four", "length=0,height=4,connect=1"), ("connect_four", "length=4,height=4,connect=0"),
            ("connect_four", "length=4,height=4,connect=5"), ("chess", ""),
            ("tic_tac_toe_np", "symmetry=1"), ("sum_four_to_one", "heaps=3:3,symmetry=1"),
            ("sum_four_to_one", "heaps=3:3,board_symmetry=1"), ("four_to_one", "start=4,board_symmetry=1"),
            ("othello_bit_new", "length=4,height=4,symmetry=1,board_symmetry=1")]
    return out


def answer(name, params):
    """Everything the registry and the plans say about one descriptor."""
    from gamesmanmpi_amd import _lib
    lib = _lib.load()
    err = lambda rc: {"code": rc, "text": lib.gm_last_error().decode(errors="replace")}  # noqa: E731
    gid = ctypes.c_int(-1)
    rc = lib.gm_game_lookup(name.encode(), params.encode(), ctypes.byref(gid))
    if rc:
        return {"refused": err(rc)}
    bound, levels, bits = ctypes.c_uint64(), ctypes.c_uint32(), ctypes.c_uint32()
    assert lib.gm_game_info(gid, ctypes.byref(bound), ctypes.byref(levels), ctypes.byref(bits)) == 0
    root, nsym, tb = ctypes.c_uint64(), ctypes.c_uint32(), ctypes.c_uint64()
    assert lib.gm_root(gid, ctypes.byref(root)) == 0
    assert lib.gm_symmetry_count(gid, ctypes.byref(nsym)) == 0
    rc = lib.gm_tb_info(gid, ctypes.byref(tb))
    a = {"bound": bound.value, "levels": levels.value, "key_bits": bits.value, "root": root.value,
         "symmetry_count": nsym.value, "tb_info": tb.value if rc == 0 else {"code": rc}}
    for tag, flags in (("plan", 0), ("plan_hash_table", _lib.GM_F_HASH_TABLE),
                       ("plan_keyed", _lib.GM_F_FORCE_HASHED)):
        p = _lib.gm_plan_t()
        rc = lib.gm_plan(gid, 0, flags, 0, ctypes.byref(p))
        a[tag] = err(rc) if rc else {f: getattr(p, f) for f, _ in _lib.gm_plan_t._fields_}
    return a


def test_registry_answers_are_the_recorded_ones():
    with open(ANSWERS) as f:
        rows = json.load(f)
    assert [(r["name"], r["params"]) for r in rows] == descriptors()
    refused = 0
    for r in rows:
        assert answer(r["name"], r["params"]) == r["answer"], (r["name"], r["params"])
        refused += "refused" in r["answer"]
    assert len(rows) >= 140 and refused >= 25


if __name__ == "__main__" and sys.argv[1:] == ["--record"]:
    sys.path.insert(0, ROOT)
    os.makedirs(os.path.dirname(ANSWERS), exist_ok=True)
    with open(ANSWERS, "w") as f:
        json.dump([{"name": n, "params": p, "answer": answer(n, p)} for n, p in descriptors()], f, indent=0)
        f.write("\n")
