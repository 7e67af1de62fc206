"""The partitioned search that verifies its pairs in LDS (csrc/group_inplace.hip, route bit `search_inplace`) against
a brute-force all-pairs Hamming count in numpy (keys of one length within d substitutions). GPU only."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


@pytest.fixture(scope="module")
def F():
    import fastqdedup_amd
    return fastqdedup_amd


def _family(n, L, lo, hi, seed):
    """n random keys that share the bases [lo, hi): all pairwise candidates of the segment that holds them."""
    rows = np.random.default_rng(seed).choice(ACGT, size=(n, L))
    rows[:, lo:hi] = rows[0, lo:hi]
    return rows


def _reads(kind):
    """The reads of one case, as a list of key bytes."""
    from fastqdedup_amd.synth import synth_keys
    rng = np.random.default_rng(9)
    if kind == "L32":           # some N: three bit planes, one word
        rows = synth_keys(6000, 32, 32, 31, sub_rate=1.5e-2, n_rate=2e-3)
    elif kind == "L64":         # ACGT only: two planes, two words, segments across the word boundary
        rows = synth_keys(4000, 64, 64, 32, sub_rate=8e-3, n_rate=0.0)
    elif kind == "ragged":      # copies of one molecule cut to 30, 31 and 32 bases
        rows = synth_keys(4000, 32, 32, 33, sub_rate=2e-2)
        return [bytes(r[:30 + i % 3]) for i, r in enumerate(rows)]
    elif kind == "lowc12":      # three skewed symbols, 3-base segments: long chains of equal hashes, edges by the 100 000
        rows = rng.choice(ACGT[:3], size=(3000, 12), p=[0.5, 0.3, 0.2])
    elif kind == "big":         # with one bucket bit and no marking: two buckets of thousands of items
        rows = synth_keys(3000, 32, 32, 34, sub_rate=1.5e-2, n_rate=2e-3)
    elif kind == "crowd":       # ~440 distinct keys share their first half, among 400 random ones
        rows = rng.choice(ACGT, size=(1300, 32))
        rows[:900] = rows[0]
        for r in rows[:900]:    # ... and differ from one second half in up to two bases
            r[rng.integers(16, 32, size=2)] = rng.choice(ACGT, size=2)
    elif kind == "over":        # 2000 keys sharing segment 0 of three: 2 M candidate pairs, more than the first lists hold
        rows = np.concatenate([synth_keys(3000, 32, 32, 35, sub_rate=1.5e-2, n_rate=2e-3), _family(2000, 32, 0, 10, 36)])
    elif kind == "L100":        # records of two uint4
        rows = synth_keys(3000, 100, 100, 37, sub_rate=5e-3, n_rate=1e-3)
    return [bytes(r) for r in np.ascontiguousarray(rows)]


def _brute(keys, d):
    """Sorted (i, j), i < j, of the keys of one length within Hamming distance d."""
    lens = np.array([len(k) for k in keys])
    out = []
    for L in np.unique(lens):
        idx = np.flatnonzero(lens == L)
        a = np.frombuffer(b"".join(keys[i] for i in idx), dtype=np.uint8).reshape(len(idx), L)
        for lo in range(0, len(idx), 128):
            r, c = np.nonzero((a[lo:lo + 128, None, :] != a[None, :, :]).sum(axis=2) <= d)
            r, c = idx[lo + r], idx[c]
            out += zip(r[r < c].tolist(), c[r < c].tolist())
    return sorted(out)


def _collapsed(F, kind):
    """A context holding the unique table of the reads of `kind`, and its keys in row order."""
    reads = _reads(kind)
    raw = np.frombuffer(b"".join(reads), dtype=np.uint8)
    sizes = [len(r) for r in reads]
    ctx = F.Context(0)
    if kind == "L64":           # (the automatic geometry starts from "ACGNT", three planes)
        present = np.zeros(128, dtype=np.uint8)
        present[list(b"ACGT")] = 1
        ctx.configure(present, 64, False)
    fixed = min(sizes) == max(sizes)
    ctx.pack_keys(raw, None if fixed else np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64), sizes[0] if fixed else 0)
    n_unique = ctx.collapse()
    first = ctx.unique_table(n_unique, labels=False, kept=False)[0]
    return ctx, [reads[int(i)] for i in first]


def _edges(ctx, d):
    e = np.empty((ctx.find_edges(d), 2), dtype=np.uint32)
    ctx.export_edges(e)
    found = sorted(map(tuple, e.tolist()))
    assert len(set(found)) == len(found), "an edge is listed twice"
    return found


BIG = {"FQD_GROUP_BUCKET_BITS": "1", "FQD_GROUP_NO_REFINE": "1"}
CROWD = {"FQD_GROUP_CROWDED_LIMIT": "64", "FQD_GROUP_NO_SLABS": "1"}      # (buckets are marked under exact sizes only)


@pytest.mark.parametrize("kind,d,env", [("L32", 1, {}), ("L32", 2, {}), ("L32", 3, {}), ("L64", 2, {}), ("ragged", 2, {}),
                                        ("lowc12", 3, {}), ("big", 1, BIG), ("big", 2, BIG), ("crowd", 2, CROWD)])
def test_edges_equal_brute_force(F, monkeypatch, kind, d, env):
    """pack_keys -> collapse -> find_edges -> export_edges with the in-place kernel pinned: several passes in one
    partition, two words per plane, staged lengths, an edge buffer that has to grow (lowc12), buckets beyond the slice
    (big), and a marked bucket left to the refinement or the tiles (crowd)."""
    monkeypatch.setenv("FQD_EDGES", "grouped")
    monkeypatch.setenv("FQD_GROUP_VERIFY", "inplace")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    ctx, keys = _collapsed(F, kind)
    found = _edges(ctx, d)
    route, want = ctx.route(), _brute(keys, d)
    assert route["search_inplace"] and route["search_grouped"] and not route["search_sort"], route
    assert found == want and want
    assert ctx.edge_stats()["edges"] == len(found)
    assert kind != "lowc12" or (len(want) > max(1024, len(keys)) and route["search_retried"]), route
    assert kind != "crowd" or route["search_refined"] or route["search_tiles"], route


def test_lists_beyond_their_budget_turn_the_context_in_place(F, monkeypatch):
    """The automatic way in: candidate lists that outgrow FQD_GROUP_CAND_BUDGET send a context of one-uint4 records in
    place (once: the second search starts there); FQD_GROUP_VERIFY=list keeps the sort path. A need is reported only by
    lists that overflowed -- the first ones hold 2^20 pairs -- so the keys include a family of 2000 that share segment
    0, and marking is off: the family's bucket would otherwise leave through the tiles before any list fills."""
    monkeypatch.setenv("FQD_EDGES", "grouped")
    monkeypatch.setenv("FQD_GROUP_CAND_BUDGET", "1000")
    monkeypatch.setenv("FQD_GROUP_NO_REFINE", "1")
    ctx, keys = _collapsed(F, "over")
    want = _brute(keys, 2)
    assert _edges(ctx, 2) == want and want
    route = ctx.route()
    assert route["search_inplace"] and route["search_retried"] and not route["search_sort"], route
    assert _edges(ctx, 2) == want
    route = ctx.route()
    assert route["search_inplace"] and not route["search_retried"] and not route["search_sort"], route
    monkeypatch.setenv("FQD_GROUP_VERIFY", "list")
    ctx, keys = _collapsed(F, "over")
    assert _edges(ctx, 2) == want
    assert ctx.route()["search_sort"] and not ctx.route()["search_inplace"], ctx.route()


def test_cluster_keys_fused_route_retries_in_place(F, oracle, monkeypatch):
    """fqd_cluster_keys with the fused collapse: the search that continues the collapse's pass 0 meets lists beyond the
    budget (2100 reads share segment 1 of three), runs whole once more and arrives in place; the warm call starts there."""
    from fastqdedup_amd.synth import fixed_offsets, synth_keys
    monkeypatch.setenv("FQD_FUSED_MIN_READS", "100000")
    monkeypatch.setenv("FQD_EDGES", "grouped")
    monkeypatch.setenv("FQD_GROUP_CAND_BUDGET", "1000")
    monkeypatch.setenv("FQD_GROUP_NO_REFINE", "1")      # (else the family's bucket is marked and leaves through the tiles)
    n, L, d = 210_000, 32, 2       # (the fused collapse starts above 2^8 buckets of 800 reads)
    keys = synth_keys(n, L, L, 38, sub_rate=5e-3, n_rate=1e-4)
    keys[::100] = _family(n // 100, L, 10, 21, 39)
    raw = np.ascontiguousarray(keys).reshape(-1)
    ctx = F.Context(0)
    for method in ("directional", "adjacency"):
        want = oracle.dedup(raw, fixed_offsets(n, L), max_distance=d, method=method)
        for job in range(2):
            got = F.cluster_keys(raw, key_len=L, max_distance=d, method=method, context=ctx)
            assert (got.n_unique, got.n_clusters) == (want["n_unique"], want["n_clusters"]), (method, job, got.route)
            assert np.array_equal(got.kept_read_ids, want["kept_read_ids"]), (method, job)
        assert got.route["search_inplace"] and not got.route["search_sort"], (method, got.route)


def test_records_above_one_uint4_keep_the_lists(F, monkeypatch):
    monkeypatch.setenv("FQD_EDGES", "grouped")
    monkeypatch.setenv("FQD_GROUP_VERIFY", "inplace")
    monkeypatch.setenv("FQD_GROUP_CAND_BUDGET", "1000")
    ctx, keys = _collapsed(F, "L100")
    assert _edges(ctx, 2) == _brute(keys, 2) != []
    assert ctx.route()["search_grouped"] and not ctx.route()["search_inplace"], ctx.route()
