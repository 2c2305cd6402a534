"""GPU: every search path stays exact across cos_index_append and cos_index_delete on a handle whose caches are WARM.

Around the resident graph a handle keeps derived state, each with its own rule for when it goes stale: the level-table operand and its
per-ef sets, the locality-order ranks, the norms beside the adjacency, the per-stream workspaces (table buffer, order buffers, digit
rows) and the host-pipe workspaces, the exact filter's bitset, the flat scan's workspace, the host mirrors of the levels.
tests/mutation_scenario.py states one history of seven appends and deletes on the CPU oracle (tests/test_mutation_scenario.py proves
that every step moves the answers).  Here a handle with every walk feature on lives through that history and runs the whole search
matrix BEFORE the first step and AFTER every step, so that every cache is warm when the next step arrives.  At each point

  * its graph is the oracle's, slot for slot;
  * every search of the matrix equals, bit for bit (ids, score bits, counts, per-query status), the same search on `cold`: a fresh
    handle that got this graph by upload, every feature off — it has never seen another graph, so whatever `warm` carried over shows;
  * every search equals the oracle's on every 7th query and on all the queries near the deleted vectors — a mistake both handles share;
  * the launch reports (cos_index_last_walk_split) that the table, with the CURRENT graph's column count, and the cut were really taken.

No test here runs a build with an invalidation removed: a table or a rank array of the old graph's size indexed with the new graph's
node numbers reads out of bounds.  Sensitivity rests on the three legs above and on the CPU conditions of the scenario."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import helpers as H
from tests import mutation_scenario as M

pytestmark = pytest.mark.gpu

TOP_K = 10
LAT4, LAT, TABLE_MIN, ORDER_MIN, CHAIN_SIDE_MIN = 4, 16, 64, 128, 256     # the knobs of tests/test_gpu_walk_plan.py
FULL_ITEMS = ("plan", "mags", "mags_small_launch", "ef", "exact", "host", "scans")
SMALL_ITEMS = ("plan", "mags", "host")


# ------------------------------------------------------------------------------------------------
# handles
# ------------------------------------------------------------------------------------------------
def _handle(p, feature_thresholds=False):
    import cosdata_amd as ca
    from cosdata_amd import _lib
    st = ca.StorageType(ca.StorageKind(p.storage), p.resolution)
    hp = ca.HNSWHyperParams(num_layers=p.num_layers, ef_construction=p.ef_construction, ef_search=p.ef_search,
                            level_0_neighbors_count=p.level0_neighbors_count, neighbors_count=p.neighbors_count)
    mk = lambda: ca.HNSWIndex(p.dim, hp, ca.DistanceMetric(p.metric), st, (p.range_lo, p.range_hi), p.shortlist_size, seed=p.seed)
    if not feature_thresholds:
        return mk()
    with _lib.tuning(walk_chain_min_b=CHAIN_SIDE_MIN, walk_side_min_b=CHAIN_SIDE_MIN):   # read at create
        return mk()


def _features_on(ix):
    import cosdata_amd as ca
    ix.set_latency_waves(LAT4)
    ix.set_latency_mode(LAT)
    ix.set_walk_table(ca.HNSWIndex.WALK_TABLE_AUTO, TABLE_MIN)
    ix.set_walk_order(ORDER_MIN)
    return ix


def _features_off(ix):
    ix.set_walk_order(0)
    ix.set_walk_table(0, 0)
    ix.set_latency_mode(0)
    ix.set_latency_waves(0)
    return ix


def _warm_built(sc):
    return _features_on(_handle(sc.params, True).upload_vectors(sc.X[:M.N0]).build(M.BATCH))


def _cold(sc, warm, at):
    ix = _handle(sc.params).upload_vectors(sc.X[:at])
    ix.upload_graph(warm.download_graph(), warm.download_root())
    return _features_off(ix)


def _same_graph(a, b):
    assert len(a) == len(b)
    for l, ((ia, na), (ib, nb)) in enumerate(zip(a, b)):
        assert np.array_equal(ia, ib), f"level {l}: node ids differ"
        assert np.array_equal(na, nb), f"level {l}: {int((na != nb).any(axis=1).sum())} rows differ"


# ------------------------------------------------------------------------------------------------
# the search matrix
# ------------------------------------------------------------------------------------------------
def _lists(ids, sc, cnt, status=None):
    """(ids, score bits, counts[, status]) with everything past a query's count blanked: what a call promises"""
    ids, sc = np.array(ids).view(np.uint32), np.array(sc).view(np.uint32)
    cnt = np.array(cnt).view(np.uint32)
    past = np.arange(ids.shape[-1])[None, :] >= cnt.reshape(-1, 1)
    ids.reshape(-1, ids.shape[-1])[past] = 0
    sc.reshape(-1, sc.shape[-1])[past] = 0
    return (ids, sc, cnt) + (() if status is None else (np.array(status, np.int32),))


def _dev_search(ix, Q, top_k=TOP_K):
    import torch
    dev = torch.device("cuda:0")
    B = Q.shape[0]
    q = torch.from_numpy(np.ascontiguousarray(Q)).to(dev)
    ids = torch.zeros(B, top_k, dtype=torch.int32, device=dev)
    sc = torch.zeros(B, top_k, dtype=torch.float32, device=dev)
    cnt = torch.zeros(B, dtype=torch.int32, device=dev)
    st = torch.zeros(B, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    ix.batch_search_device(q.data_ptr(), B, top_k, ids.data_ptr(), sc.data_ptr(), cnt.data_ptr(), st.data_ptr(), 0)
    torch.cuda.synchronize()
    return _lists(ids.cpu().numpy(), sc.cpu().numpy(), cnt.cpu().numpy(), st.cpu().numpy())


def _matrix(ix, sc, items, plan=None):
    """every search of `items` on one handle -> ({name: arrays}, {name: what the oracle is asked for it}).  `plan(B, ef, visited)` runs
    after every launch on stream 0 (the launch report is per stream)."""
    from cosdata_amd import _lib
    Q, Qv = sc.Q, sc.Qv
    out, spec = {}, {}

    def dev(name, qk, B, ef=sc.params.ef_search, visited=0):
        out[name] = _dev_search(ix, (Qv if qk == "Qv" else Q)[:B])
        spec[name] = ("search", qk, B, TOP_K, ef, visited)
        if plan:
            plan(B, ef, visited)

    def host(name, qk, B, k):
        ids, s, cnt, rc, status = ix.batch_search((Qv if qk == "Qv" else Q)[:B], k, return_status=True)
        assert rc == 0, name
        out[name] = _lists(ids, s, cnt, status)
        spec[name] = ("search", qk, B, k, sc.params.ef_search, 0)

    if "plan" in items:        # 1. four-wave kernel with table | one-wave kernel | throughput with table | ordered with table | chain + side stream
        for B in (1, 4, 16, 64, 128, 300):
            dev(f"dev_{B}", "Q", B)
        dev("dev_victims", "Qv", Qv.shape[0])
    if "mags" in items:        # 2. the norms beside the adjacency: gather | refill | read by the rule
        for B in ((1023, 1024, 4096) if "mags_small_launch" in items else (1024, 4096)):
            dev(f"dev_{B}", "Q", B)
    if "mags_small_launch" in items:
        with _lib.tuning(walk_adj_mag=2):                      # ... and read at a small launch
            dev("dev_300_adj_mag_2", "Q", 300)
    if "ef" in items:          # 3. ef back and forth: one table set per key, each of the current graph
        ef0 = sc.params.ef_search
        try:
            for ef in (64, 257):
                ix.set_ef_search(ef)
                dev(f"dev_300_ef_{ef}", "Q", 300, ef=ef)
        finally:
            ix.set_ef_search(ef0)
    if "exact" in items:       # 4. the exact filter's bitset: its stride follows the largest level
        try:
            ix.set_visited_mode(1)
            for B in (64, 300):
                dev(f"dev_{B}_exact", "Q", B, visited=1)
        finally:
            ix.set_visited_mode(0)
    if "host" in items:        # 5. host entry point: host-pipe workspaces, the wide finalize, the per-level lists, pipelined chunks
        host("host_300", "Q", 300, TOP_K)
        host("host_300_top_200", "Q", 300, 200)
        host("host_victims", "Qv", Qv.shape[0], TOP_K)
        with _lib.tuning(host_pipeline_min_b=256):             # 300 queries = chunks of 256 + 44, a workspace each
            host("host_300_pipelined", "Q", 300, TOP_K)
        ids, sims, counts = ix.ann_search_batch(Q[:300])
        out["ann_300"] = _lists(ids, sims, counts)
        spec["ann_300"] = ("ann", 300)
    if "scans" in items:       # 6. exhaustive scans on the same handle
        for qk, k in (("Q", 10), ("Q", 40), ("Qv", 10)):       # (40: the 256-key pool)
            out[f"flat_{qk}_{k}"] = _lists(*ix.flat_search((Qv if qk == "Qv" else Q)[:64], k))
            spec[f"flat_{qk}_{k}"] = ("flat", qk, 64, k)
    if "scans" in items or "brute" in items:
        for qk in ("Q", "Qv"):
            ids, s = ix.bruteforce_topk((Qv if qk == "Qv" else Q)[:64], 10)
            out[f"brute_{qk}_10"] = (ids.view(np.uint32), s.view(np.uint32))
            spec[f"brute_{qk}_10"] = ("brute", qk, 64, 10)
    return out, spec


def _plan_checker(ix, p, counts):
    """the launch that just ran on stream 0 took the table, of the graph as it is NOW (`counts`: the oracle's level sizes), and the cut
    wherever walk_plan.h puts them for this handle's knobs"""
    def check(B, ef, visited):
        sp = ix.last_walk_split()
        assert sp.queries == B
        cuts = ix.walk_order_cuts()
        assert cuts
        ordered = B >= ORDER_MIN and ef <= 256
        assert sp.cut_after_level == (cuts[0] if ordered else 0), (B, ef, visited)
        lmin, cols = ix.walk_table_info()
        if p.storage == O.STORAGE_U8:
            want = B <= LAT4 or B >= TABLE_MIN
        elif p.storage == O.STORAGE_SUBBYTE and p.resolution == 2:
            want = B >= TABLE_MIN                               # (the four-wave kernel reads the table over u8 codes only)
        else:
            assert (lmin, cols) == (0, 0)                       # no level table for this storage: every plan with one is refused
            want = False
        if want:
            assert lmin >= 1 and cols == sum(counts[lmin:]) and [ix.level_count(l) for l in range(len(counts))] == counts, (lmin, cols, counts)
        assert (sp.table_level_min, sp.table_cols) == ((lmin, cols) if want else (0, 0)), (B, ef, visited)
        assert (sp.table_evals > 0) == want, (B, ef, visited)
    return check


def _plain_checker(ix):
    def check(B, ef, visited):
        sp = ix.last_walk_split()
        assert sp.queries == B and sp.table_level_min == 0 and sp.table_cols == 0 and sp.cut_after_level == 0 and sp.table_evals == 0
    return check


def _assert_oracle(oix, sc, at, got, spec):
    """every entry against the oracle: every 7th query of a prefix of Q, every query of Qv, every query of a scan"""
    p = sc.params
    searched = {}
    for name, s in spec.items():
        if s[0] == "search":
            key = s[1], s[3], s[4], s[5]
            searched[key] = max(searched.get(key, 0), s[2])
    ref = {}
    try:
        for (qk, k, ef, visited), maxB in searched.items():
            oix.set_ef_search(ef)
            oix.set_visited_mode(visited)
            q = sc.Qv[:maxB] if qk == "Qv" else sc.Q[:maxB:7]
            ids, s, cnt, rc, status = oix.search_batch(q, k, threads=4, raise_on_error=False)
            ref[qk, k, ef, visited] = _lists(ids, s, cnt, status)
    finally:
        oix.set_ef_search(p.ef_search)
        oix.set_visited_mode(0)
    for name, s in spec.items():
        g = got[name]
        if s[0] == "search":
            _, qk, B, k, ef, visited = s
            rows = np.arange(B) if qk == "Qv" else np.arange(0, B, 7)
            r = ref[qk, k, ef, visited]
            for a, b, what in zip(g, r, ("ids", "score bits", "counts", "status")):
                assert np.array_equal(a[rows], b[:rows.size]), f"{name}: {what} differ from the oracle's"
        elif s[0] == "ann":
            ids, sims, counts = g
            for b in range(0, s[1], 7):
                oi, osim, olc = oix.ann_search(sc.Q[b])
                assert np.array_equal(counts[b], olc), f"{name}: query {b}: level counts {counts[b]} vs {olc}"
                off = 0
                for slot, c in enumerate(int(c) for c in olc):
                    assert np.array_equal(ids[b, slot, :c], oi[off:off + c]), f"{name}: query {b} slot {slot}: walk ids differ"
                    assert np.array_equal(sims[b, slot, :c], osim[off:off + c].view(np.uint32)), f"{name}: query {b} slot {slot}: sims differ"
                    off += c
        elif s[0] == "flat":
            r = _lists(*oix.flat_search_batch((sc.Qv if s[1] == "Qv" else sc.Q)[:s[2]], s[3], threads=4))
            for a, b, what in zip(g, r, ("ids", "score bits", "counts")):
                assert np.array_equal(a, b), f"{name}: {what} differ from the oracle's"
        else:
            oi, osc = O.bruteforce_topk(sc.X[:at], (sc.Qv if s[1] == "Qv" else sc.Q)[:s[2]], s[3], threads=4)
            assert np.array_equal(g[0], oi) and np.array_equal(g[1], osc.view(np.uint32)), f"{name}: differs from the oracle's"


# ------------------------------------------------------------------------------------------------
# one handle through one history
# ------------------------------------------------------------------------------------------------
class Timeline:
    """`warm` and the oracle side by side, at one point of the history (0 = before the first step).  check() runs the matrix there;
    goto() applies steps, and runs the matrix unchecked at a point nobody checked so that the caches are warm whatever was selected."""

    def __init__(self, sc, items, make_warm=_warm_built, apply=None, make_oracle=None):
        self.sc, self.items = sc, items
        self.oix = make_oracle(sc) if make_oracle else sc.oracle()
        self.warm = make_warm(sc)
        self.apply = apply or sc.apply
        self.point, self.warmed, self.cols = 0, False, None

    @property
    def at(self):
        return self.sc.n_at[self.point]

    def goto(self, point):
        assert point >= self.point
        while self.point < point:
            if not self.warmed:
                _matrix(self.warm, self.sc, self.items)
            self.sc.apply(self.oix, self.point)
            self.apply(self.warm, self.point)
            self.point += 1
            self.warmed = False
            assert self.warm.n == self.at and self.warm.level_count(0) == self.at + 1
        return self

    def check(self):
        sc, warm, oix = self.sc, self.warm, self.oix
        _same_graph(warm.download_graph(), oix.export_graph())
        counts = M.level_counts(oix)
        cold = _cold(sc, warm, self.at)
        got, spec = _matrix(warm, sc, self.items, _plan_checker(warm, sc.params, counts))
        self.warmed = True
        ref, _ = _matrix(cold, sc, self.items, _plain_checker(cold))
        cold.close()
        for name in spec:
            assert len(got[name]) == len(ref[name])
            for a, b, what in zip(got[name], ref[name], ("ids", "score bits", "counts", "status")):
                bad = np.flatnonzero((a != b).reshape(a.shape[0], -1).any(axis=1))
                assert bad.size == 0, f"point {self.point}, {name}: {what} of {bad.size} queries differ from the cold handle's (first: {bad[:5]})"
        _assert_oracle(oix, sc, self.at, got, spec)
        # the table follows the graph: an append that adds nodes to the table levels adds columns
        lmin, cols = warm.walk_table_info()
        if self.point and lmin and sc.steps[self.point - 1][0] == "append" and sc.history[self.point - 1][1] >= 300:
            assert self.cols is not None and cols > self.cols, (self.point, cols, self.cols)
        self.cols = cols
        # the exhaustive scans read rows, not the graph: they still return a deleted id, like the oracle's; the host filters.
        # (The walk's answers after a delete are the oracle's, asserted above: a delete whose own walk does not reach the node on some
        # level leaves it linked there, in the reference too.)
        gone = [what for kind, what in sc.steps[:self.point] if kind == "delete"]
        if gone and sum(g.size for g in gone) >= 40:
            for name, s in spec.items():
                if s[0] in ("flat", "brute") and s[1] == "Qv":
                    assert np.isin(got[name][0], np.concatenate(gone)).any(), name
        if self.at > M.N0 + 1:
            assert (got["dev_300"][0] >= np.uint32(M.N0)).any() and (got["host_300"][0] >= np.uint32(M.N0)).any()   # appended vectors are found


_timelines = {}


def _check_at(key, point, last, new):
    tl = _timelines.get(key)
    if tl is None or tl.point > point:
        tl = _timelines[key] = new()
    tl.goto(point).check()
    if point == last:
        _timelines.pop(key).warm.close()


@pytest.fixture(scope="module")
def scenarios():
    made = {}

    def get(name):
        if name not in made:
            made[name] = {"full": lambda: M.make(), "short": lambda: M.make(M.SHORT_HISTORY),
                          "q2": lambda: M.make(M.SHORT_HISTORY, dim=128, storage=O.STORAGE_SUBBYTE, resolution=2),
                          "f16": lambda: M.make(M.SHORT_HISTORY, storage=O.STORAGE_F16)}[name]()
        return made[name]
    yield get
    for tl in _timelines.values():
        tl.warm.close()
    _timelines.clear()


@pytest.mark.parametrize("point", range(len(M.FULL_HISTORY) + 1))
def test_warm_handle_follows_the_full_history(scenarios, point):
    """u8 x 96, append 1 / 700 / 800, delete 1 / 39 / 120, append 300; the whole matrix at every point.  Guards, in cos_index_append
    (builder.hip): cos_graph_changed(LEVELS) (with it walk_operands.hip cos_ensure_level_table's table_sets.clear() and the
    workspace's table buffer regrown by get_workspace when the set's stride grows), cos_flat_ws_release (kernels_flat.hip
    cos_flat_ws_release: the stored code sums and zero-norm flags of the old corpus), the levels' host mirrors (builder.hip:458-459);
    in cos_index_delete (builder.hip): cos_graph_changed(ADJACENCY), the host mirrors, and the argued NON-invalidation of the level table and
    the locality order; in engine.hip: vis_tab_prepare's stride of the grown graph over a bitset that is all-zero between launches,
    walk_operands.hip cos_ensure_adj_mags after every graph change, the host pipe's chunk workspaces."""
    sc = scenarios("full")
    _check_at("full", point, len(M.FULL_HISTORY), lambda: Timeline(sc, FULL_ITEMS))


def _oracle_restored(sc):
    """the oracle's side of _warm_uploaded: an imported graph has the link state of a reload, not the build's"""
    src = sc.oracle()
    return O.OracleIndex(sc.params).set_vectors(sc.X[:M.N0]).import_graph(src.export_graph(), src.root_raw()).restore_link_state()


def _warm_uploaded(sc):
    """a handle that got its graph by upload and searched on it, then restored the link state"""
    src = sc.oracle()
    ix = _handle(sc.params, True).upload_vectors(sc.X[:M.N0])
    ix.upload_graph(src.export_graph(), src.root_raw())
    _features_on(ix)
    _matrix(ix, sc, SMALL_ITEMS)
    return ix.restore_link_state()


class _Borrowed:
    """upload_vectors_device + append_device: the handle reads the caller's table, which holds every row of the history from the start"""

    def __init__(self, sc):
        import torch
        self.sc = sc
        self.Xd = torch.from_numpy(sc.X).cuda()

    def make_warm(self, sc):
        return _features_on(_handle(sc.params, True).upload_vectors_device(self.Xd.data_ptr(), M.N0, keepalive=self.Xd).build(M.BATCH))

    def apply(self, ix, step):
        kind, what = self.sc.steps[step]
        if kind == "append":
            ix.append_device(self.Xd.data_ptr(), what[1] - what[0], M.BATCH, keepalive=self.Xd)
        else:
            ix.delete(what)


def _small_timeline(case, sc):
    if case == "uploaded":
        return Timeline(sc, SMALL_ITEMS, make_warm=_warm_uploaded, make_oracle=_oracle_restored)
    if case == "borrowed":
        b = _Borrowed(sc)
        return Timeline(sc, SMALL_ITEMS + ("brute",), make_warm=b.make_warm, apply=b.apply)
    return Timeline(sc, SMALL_ITEMS)


@pytest.mark.parametrize("point", range(len(M.SHORT_HISTORY) + 1))
@pytest.mark.parametrize("case", ["q2", "f16", "uploaded", "borrowed"])
def test_warm_handle_follows_the_short_history(scenarios, case, point):
    """append 700, delete 40, append 300 with matrix items 1, 2 (1024 and 4096 queries) and 5.
    q2: quaternary codes x 128 — the level table exists from 128 dims and the workspace's digit rows (engine.hip get_workspace, qdig)
    belong to it; f16: no table — the row path and the refused table plans, the locality order alone (builder.hip:401);
    uploaded: a graph that came by upload, searched, then cos_index_restore_link_state (builder.hip:359-360) and the history;
    borrowed: the caller's grown table (builder.hip:421-422, 435) — the rerank and the brute force read it."""
    sc = scenarios(case if case in ("q2", "f16") else "short")
    _check_at(case, point, len(M.SHORT_HISTORY), lambda: _small_timeline(case, sc))


def test_searching_transaction_history_follows_the_oracle():
    """the 14 random steps of test_gpu_append.py::test_random_interleaving_of_appends_and_deletes_follows_the_oracle (seed 1) on a
    handle with every walk feature on, a search after EVERY step (4, 16, 64, 128 or 300 queries, drawn): the graph and the answers are
    the oracle's and the launch took the table of the graph as it is.  Guards the same lines as the full history (builder.hip:401-405,
    630-632) under appends of 1 ... 400 and deletes of 1 ... 25 ids in an order no scenario chose."""
    seed = 1
    rng, pick = np.random.default_rng(1000 + seed), np.random.default_rng(77)
    dim, n0, total = 64, 800, 3200
    X = H.clustered_corpus(total, dim, n_centers=24, seed=40 + seed)
    p = O.HNSWParams(dim=dim, num_layers=4, ef_construction=40, ef_search=40, seed=seed, level0_neighbors_count=32, neighbors_count=16)
    oix = O.OracleIndex(p).set_vectors(X[:n0])
    oix.build_rounds(96)
    dix = _features_on(_handle(p, True).upload_vectors(X[:n0]).build(96))
    at, dead = n0, set()
    for step in range(15):                                       # (step 0: a search in front of the first change)
        if step:
            if at < total and (rng.random() < 0.6 or at - len(dead) < 50):
                m = int(min(total - at, rng.choice([1, 7, 60, 400])))
                oix.append(X[at:at + m], 96)
                dix.append(X[at:at + m], 96)
                at += m
            else:
                live = np.array(sorted(set(range(at)) - dead), np.uint32)
                k = int(rng.choice([1, 3, 25]))
                ids = rng.choice(live, size=min(k, live.size), replace=False).astype(np.uint32)
                oix.delete(ids)
                dix.delete(ids)
                dead |= set(ids.tolist())
            _same_graph(dix.download_graph(), oix.export_graph())
        B = int(pick.choice([4, 16, 64, 128, 300]))
        Q = H.queries_from(X[:at], B, noise=0.05, seed=100 + step)
        got = _dev_search(dix, Q)
        _plan_checker(dix, p, M.level_counts(oix))(B, p.ef_search, 0)
        ids, s, cnt, rc, status = oix.search_batch(Q, TOP_K, threads=4, raise_on_error=False)
        for a, b, what in zip(got, _lists(ids, s, cnt, status), ("ids", "score bits", "counts", "status")):
            assert np.array_equal(a, b), f"step {step}, {B} queries: {what} differ from the oracle's"
    assert at > n0 and dead
    dix.close()


def _postings(n_docs, vocab, seed):
    rng = np.random.default_rng(seed)
    terms = np.sort(rng.choice(1 << 31, vocab, replace=False)).astype(np.uint32)
    docs, tfs, offsets = [], [], [0]
    for t in range(vocab):
        d = np.sort(rng.choice(n_docs, int(rng.integers(1, n_docs // 8)), replace=False)).astype(np.uint32)
        docs.append(d)
        tfs.append(np.array([O.bm25_tf(int(c), int(dl), 100.0, 1.5, 0.75) for c, dl in zip(rng.integers(1, 6, d.size), rng.integers(20, 300, d.size))], np.float32))
        offsets.append(offsets[-1] + d.size)
    return terms, np.array(offsets, np.uint64), np.concatenate(docs), np.concatenate(tfs)


def test_hybrid_calls_follow_an_append_to_the_dense_index(scenarios):
    """cos_hybrid_search_batch and cos_hybrid_search_mixed (dense + BM25 arms, 300 queries: table and cut) before and after 700 vectors
    are appended to the dense index: a hybrid context walks on a dense stream of its own, i.e. a workspace of its own under the dense
    handle (engine.hip get_workspace), whose table buffer must regrow with table_stride (builder.hip:402) — against the oracle composition."""
    import cosdata_amd as ca
    sc = scenarios("short")
    B, k = 300, 10
    n_docs = sc.n_at[1]
    oix = sc.oracle()
    dix = _warm_built(sc)
    terms, offsets, docs, tfs = _postings(n_docs, 120, 9)
    bm = ca.BM25Index(terms, offsets, docs, tfs, n_docs)
    rng = np.random.default_rng(5)
    qt = [rng.choice(terms, int(rng.integers(1, 6)), replace=False).astype(np.uint32) for _ in range(B)]
    q_off = np.concatenate([[0], np.cumsum([t.size for t in qt])]).astype(np.uint32)
    q_terms = np.concatenate(qt)
    bm_lists = [O.bm25_search(terms, offsets, docs, tfs, n_docs, t, 3 * k)[0] for t in qt]
    Q = sc.Q[:B]
    arms = np.full(B, ca.ARM_DENSE_BM25, np.uint8)
    with ca.HybridContext() as ctx:
        for point in (0, 1):
            if point:
                sc.apply(oix, 0)
                sc.apply(dix, 0)
                assert sc.steps[0][0] == "append" and dix.n == M.N0 + 700
            od = oix.search_batch(Q, 3 * k, threads=4)
            calls = {"batch": ca.hybrid_search_batch(dix, bm, Q, q_terms, q_off, k, 60.0),
                     "mixed": ca.hybrid_search_mixed(ctx, dix, None, bm, arms, Q, None, (q_terms, q_off), k, 60.0)}
            assert any((od[0][i, :od[2][i]] >= M.N0).any() for i in range(B)) == bool(point)    # the dense half finds the appended vectors
            for name, (ids, s, cnt) in calls.items():
                for i in range(B):
                    fi, fs = O.rrf_fuse(od[0][i, :od[2][i]], bm_lists[i], 60.0, k)
                    c = int(cnt[i])
                    assert c == fi.size and np.array_equal(ids[i, :c], fi), (point, name, i, ids[i, :c], fi)
                    assert np.array_equal(s[i, :c].view(np.uint32), fs.view(np.uint32)), (point, name, i)
    bm.close()
    dix.close()
