"""Model check (CPU, pure Python) of the commit order of the level under the table (walk_kernel.inc, `UPT`): an expansion's
winners that have a node one level up are committed first (their similarity comes from a table column), the others after them (from
their code rows) — not in slot order.  On the pool model of tests/test_commit_equivalence.py: for random pools, `limit`, `ahead` and
winner sets, committing an ARBITRARY subset first and the rest after leaves the same poppable prefix (positions < limit) and the same
stale-window flag as slot order, with and without the pre-screen; and a whole walk whose every expansion is committed that way pops
what the reference heap pops.  Keys are (similarity, node) pairs compared like the kernel's packed 64-bit keys — similarity in the
high word, node index in the low word — and the similarities are drawn from a few values only, so ties in the high word are the rule."""
import random

import pytest

from tests.test_commit_equivalence import Walk, _level, reference_pops


def commit(pool, cap, limit, ahead, winners, prescreen):
    """walk_kernel.inc commit + insert_serial over `winners` in the given order, on a COPY of the pool (descending list of unique keys):
    -> (pool, window_ok).  A key is a tuple (similarity, node): tuple order = the order of the packed u64."""
    pool = list(pool)
    window_ok = True
    if prescreen:
        if limit <= 0:
            return pool, window_ok                                       # bar = ~0: nothing passes
        bar = pool[limit - 1] if limit - 1 < len(pool) else (-1, -1)       # an empty position holds the smallest key
        winners = [w for w in winners if w > bar]
    for w in winners:
        pos = sum(1 for e in pool if e > w)
        if pos < limit:
            pool.insert(pos, w)
            del pool[cap:]
            if pos < ahead:
                window_ok = False
    return pool, window_ok


@pytest.mark.parametrize("cap,n_sims", [(64, 3), (64, 40), (128, 6), (256, 1000)])
def test_any_subset_first_leaves_the_same_poppable_pool_and_the_same_window_flag(cap, n_sims):
    rng = random.Random(cap * 131 + n_sims)
    for trial in range(400):
        nodes = rng.sample(range(4 * cap), rng.randrange(0, cap + 1) + rng.randrange(1, 65))
        keys = [(rng.randrange(n_sims), nd) for nd in nodes]               # unique (the node is in the key), many equal similarities
        n_win = rng.randrange(1, min(64, len(keys)) + 1)
        winners, pool = keys[:n_win], sorted(keys[n_win:], reverse=True)[:cap]
        limit = rng.choice([0, 1, 2, rng.randrange(0, cap + 1), cap])
        ahead = rng.randrange(0, 4)
        for prescreen in (False, True):
            want_pool, want_ok = commit(pool, cap, limit, ahead, winners, prescreen)
            for _ in range(6):
                first = [w for w in winners if rng.random() < rng.choice([0.0, 0.25, 0.5, 1.0])]
                rest = [w for w in winners if w not in first]
                got_pool, ok1 = commit(pool, cap, limit, ahead, first, prescreen)
                got_pool, ok2 = commit(got_pool, cap, limit, ahead, rest, prescreen)
                assert got_pool[:max(limit, 0)] == want_pool[:max(limit, 0)], (trial, prescreen, limit)
                assert (ok1 and ok2) == want_ok, (trial, prescreen, limit, ahead)
            # the flag is a property of the LARGEST winner alone: it falls iff fewer than `ahead` pool entries beat it (and it is let in)
            top = max(winners)
            beat = sum(1 for e in pool if e > top)
            assert want_ok == (not (beat < ahead and beat < limit)), (trial, prescreen)


class UpWalk(Walk):
    """the model walk with the level under the table's commit order: winners whose node is in `upper` first, the others after"""

    def __init__(self, *a, upper=(), **kw):
        super().__init__(*a, **kw)
        self.upper = set(upper)

    def _winners(self, node, vis):
        win = super()._winners(node, vis)                                  # the filter is claimed in slot order, as before
        return [w for w in win if w[1] in self.upper] + [w for w in win if w[1] not in self.upper]


@pytest.mark.parametrize("n,M,ef,cap,la", [(300, 8, 64, 64, 4), (500, 16, 48, 64, 4), (800, 32, 200, 256, 4), (600, 64, 112, 128, 4), (150, 8, 17, 64, 1)])
def test_a_walk_committed_table_winners_first_pops_what_the_reference_pops(n, M, ef, cap, la):
    for seed in range(10):
        rng = random.Random(555 * n + seed)
        adj, keys = _level(rng, n, M)
        entry = rng.randrange(n)
        upper = [v for v in range(n) if rng.random() < 0.25]               # a quarter of the nodes have a node one level up
        want, want_vis = reference_pops(adj, keys, entry, ef, M)
        for prescreen in (False, True):
            a = Walk(adj, keys, entry, ef, M, cap, la, prescreen)
            b = UpWalk(adj, keys, entry, ef, M, cap, la, prescreen, upper=upper)
            while a.pool and len(a.pops) < ef:
                a.round_sequential()
                b.round_sequential()
                assert a.pops == b.pops and a.vis == b.vis, (seed, prescreen)   # equal pops after every round = equal stale decisions
                limit = ef - len(a.pops)
                assert a.pool[:limit] == b.pool[:limit], (seed, prescreen)
            assert not (b.pool and len(b.pops) < ef)
            assert b.pops == want and b.vis == want_vis
