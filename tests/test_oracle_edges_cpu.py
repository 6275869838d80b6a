"""The yardstick at the word forms' switch point: the oracle's row solver
(oracle/oracle_mt.c, what the GPU tests of tests/test_gpu_word_form_edges.py
compare with) against the scalar DFS oracle (oracle/oracle.c, pinned to the
reference's golden tables by tests/test_oracle.py) at root digit sums 253 and
254, word for word."""
import numpy as np
import pytest

from oracle.oracle import Game


@pytest.mark.parametrize("heaps,total", [("3:3:247", 253), ("3:3:248", 254)])
def test_oracle_rows_match_dfs_at_the_form_edge(heaps, total):
    assert sum(int(h) for h in heaps.split(":")) == total
    g = Game("sum_four_to_one", "heaps=" + heaps)
    r = g.solve_rows()
    r.refresh(True)
    d = g.solve(1 << 13)
    assert d.count == 4 * 4 * (int(heaps.split(":")[2]) + 1) < 4000
    assert (r.count, r.edges, r.root_line) == (d.count, d.edges, d.root_line)
    c, cl, v, m = d.dump(stride=24)
    ranks = np.array([int(bytes(c[i, :cl[i]])) for i in range(len(v))], np.int64)
    np.testing.assert_array_equal(np.sort(ranks), np.arange(d.count))
    words = np.array([r.word(int(k)) for k in ranks], np.uint32)
    np.testing.assert_array_equal(words & 3, v)
    np.testing.assert_array_equal(words >> 2, m)
    assert r.stats["win"] + r.stats["loss"] == d.count and int((v == 0).sum()) == r.stats["win"]
