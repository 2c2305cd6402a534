"""Model check (CPU, pure Python) of the commit order of the pair walk (walk_kernel.inc, `PAIR`; kernels_walk_pair.hip): an expansion's
winners are committed as THREE groups one after the other — those whose similarity comes from a table column (the level under the
table only), those whose integer dot was found in the pair's LDS cache, those whose code row is fetched — not in slot order, and which
winner lands in which group depends on what the partner wave happened to fetch before.  On the pool model of
tests/test_commit_equivalence.py, as tests/test_walk_up_table_model.py does it for two groups: for random pools, `limit`, `ahead` and
winner sets, ANY split of the winners into the three groups (empty groups included) leaves the same poppable prefix (positions < limit)
and the same stale-window flag as slot order, with and without the pre-screen; and a whole walk whose every expansion is committed
that way, with a fresh random split per expansion, pops what the reference heap pops."""
import random

import pytest

from tests.test_commit_equivalence import Walk, _level, reference_pops
from tests.test_walk_up_table_model import commit


def _split3(rng, winners):
    """a random split into (table, cache, rows), slot order kept inside each group; now and then one or two groups take everything"""
    weights = rng.choice([(1, 1, 1), (1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 1, 1), (1, 1, 0), (1, 0, 1), (1, 4, 2)])
    groups = ([], [], [])
    for w in winners:
        groups[rng.choices((0, 1, 2), weights)[0]].append(w)
    return groups


@pytest.mark.parametrize("cap,n_sims", [(64, 3), (64, 40), (128, 6), (256, 1000)])
def test_any_split_into_three_groups_leaves_the_same_poppable_pool_and_the_same_window_flag(cap, n_sims):
    rng = random.Random(cap * 977 + n_sims)
    for trial in range(400):
        nodes = rng.sample(range(4 * cap), rng.randrange(0, cap + 1) + rng.randrange(1, 65))
        keys = [(rng.randrange(n_sims), nd) for nd in nodes]               # unique (the node is in the key), many equal similarities
        n_win = rng.randrange(1, min(64, len(keys)) + 1)
        winners, pool = keys[:n_win], sorted(keys[n_win:], reverse=True)[:cap]
        limit = rng.choice([0, 1, 2, rng.randrange(0, cap + 1), cap])
        ahead = rng.randrange(0, 4)
        for prescreen in (False, True):
            want_pool, want_ok = commit(pool, cap, limit, ahead, winners, prescreen)
            for _ in range(8):
                got_pool, ok = list(pool), True
                groups = _split3(rng, winners)
                assert sorted(groups[0] + groups[1] + groups[2]) == sorted(winners)
                for g in groups:
                    got_pool, ok_g = commit(got_pool, cap, limit, ahead, g, prescreen)
                    ok = ok and ok_g
                assert got_pool[:max(limit, 0)] == want_pool[:max(limit, 0)], (trial, prescreen, limit)
                assert ok == want_ok, (trial, prescreen, limit, ahead)


class PairWalk(Walk):
    """the model walk with the pair kernel's commit order: a fresh random split of every expansion's winners into three groups"""

    def __init__(self, *a, rng=None, **kw):
        super().__init__(*a, **kw)
        self.rng = rng
        self.sizes = [0, 0, 0]

    def _winners(self, node, vis):
        win = super()._winners(node, vis)                                  # the filter is claimed in slot order, as before
        groups = _split3(self.rng, win)
        for i, g in enumerate(groups):
            self.sizes[i] += len(g)
        return groups[0] + groups[1] + groups[2]


@pytest.mark.parametrize("n,M,ef,cap,la", [(300, 8, 64, 64, 4), (500, 16, 48, 64, 3), (800, 32, 200, 256, 4), (600, 64, 112, 128, 3), (150, 8, 17, 64, 1)])
def test_a_walk_committed_in_three_groups_pops_what_the_reference_pops(n, M, ef, cap, la):
    for seed in range(10):
        rng = random.Random(811 * n + seed)
        adj, keys = _level(rng, n, M)
        entry = rng.randrange(n)
        want, want_vis = reference_pops(adj, keys, entry, ef, M)
        for prescreen in (False, True):
            a = Walk(adj, keys, entry, ef, M, cap, la, prescreen)
            b = PairWalk(adj, keys, entry, ef, M, cap, la, prescreen, rng=random.Random(seed))
            while a.pool and len(a.pops) < ef:
                a.round_sequential()
                b.round_sequential()
                assert a.pops == b.pops and a.vis == b.vis, (seed, prescreen)   # equal pops after every round = equal stale decisions
                limit = ef - len(a.pops)
                assert a.pool[:limit] == b.pool[:limit], (seed, prescreen)
            assert not (b.pool and len(b.pops) < ef)
            assert b.pops == want and b.vis == want_vis
            assert all(s > 0 for s in b.sizes)                                  # every group took part
