"""The group checks every sharded layout shares (gamesmanmpi_amd/csrc/
gm_xchg.h, xchg_mode): gm_solve_group refuses shards out of rank order and a
group that holds only part of its plan, with GM_EINVAL and before any work is
enqueued; the same shards, in order, then solve.  One 2-shard group per
layout, each at that layout's smallest sharded test shape."""
import ctypes

import pytest

pytestmark = pytest.mark.gpu

# layout -> (game, params, golden summary entry or None: the CPU oracle)
SHAPES = {
    "planes": ("sum_four_to_one", "heaps=31:31:3:15", None),
    "dense": ("sum_four_to_one", "heaps=15:15:15:15:31", None),
    "bucketed": ("tic_tac_toe_np", "", "tic_tac_toe_np"),
    "ranked": ("toot_and_otto_bitstring", "length=4,height=3", "toot_4x3"),
}


def _solve_group(shards):
    from gamesmanmpi_amd import _lib
    arr = (ctypes.c_void_p * len(shards))(*[s.handle.value for s in shards])
    r = _lib.gm_result()
    with shards[0].torch.cuda.device(shards[0].device):
        rc = _lib.load().gm_solve_group(arr, len(shards), ctypes.byref(r))
    return rc, r


@pytest.mark.parametrize("layout", sorted(SHAPES))
def test_group_order_and_size_are_checked(layout, golden_summary):
    import torch
    from gamesmanmpi_amd import _lib
    from gamesmanmpi_amd.games import GameSpec
    from gamesmanmpi_amd.keyed import _shard_bound
    from gamesmanmpi_amd.solver import Solver
    game, params, golden = SHAPES[layout]
    spec = GameSpec(game, params)
    if golden:
        want = (golden_summary[golden]["positions"], golden_summary[golden]["root_line"])
    else:
        from oracle.oracle import Game
        sol = Game(game, params).solve(1 << 22)
        want = (sol.count, sol.root_line)
    dev = torch.device("cuda")
    stream = torch.cuda.Stream(device=dev)
    per = _shard_bound(spec, 2, 0) if layout in ("bucketed", "ranked") else 0
    shards = [Solver(spec, positions=per, device=dev, layout=layout, rank=g, world=2, stream=stream) for g in range(2)]
    torch.cuda.synchronize(dev)
    rc, _ = _solve_group(shards[::-1])  # ranks 1, 0
    assert rc == _lib.GM_EINVAL, (rc, _lib.load().gm_last_error())
    rc, _ = _solve_group(shards[:1])  # one shard of a two-shard plan, no communicator
    assert rc == _lib.GM_EINVAL, (rc, _lib.load().gm_last_error())
    rc, r = _solve_group(shards)
    assert rc == 0, (rc, _lib.load().gm_last_error())
    res = shards[0]._result(r)
    assert (res.positions, res.root_line) == want
