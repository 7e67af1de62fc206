"""The one-launch neighbour search of small unique tables (csrc/small_search.hip, route bit
`search_small`) against a brute-force all-pairs Hamming count in numpy: an edge exists iff two keys
have one length and differ in at most d positions. GPU only."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

METHODS = ("highest_count", "adjacency", "directional")


@pytest.fixture(scope="module")
def F():
    import fastqdedup_amd
    return fastqdedup_amd


def _reads(kind):
    """The reads of one case, as a list of key bytes."""
    from fastqdedup_amd.synth import synth_keys
    rng = np.random.default_rng(7)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    if kind == "L32":           # three bit planes, rows in LDS, one bin
        rows = synth_keys(800, 32, 32, 11, sub_rate=1.5e-2)
    elif kind == "L64":         # two words per plane: an LDS tile above 64 KB
        rows = synth_keys(800, 64, 64, 12, sub_rate=8e-3)
    elif kind == "lowc12":      # three skewed symbols, 3-base segments: chains of 5 to 100 keys, on either side of the crowded limit
        rows = rng.choice(acgt[:3], size=(900, 12), p=[0.5, 0.3, 0.2])
    elif kind == "L300":        # rows compared from global memory
        rows = synth_keys(600, 300, 300, 13, sub_rate=3e-3)
    elif kind == "ragged":      # copies of one molecule cut to 30, 31 and 32 bases
        rows = synth_keys(900, 32, 32, 14, sub_rate=2e-2)
        return [bytes(r[:30 + i % 3]) for i, r in enumerate(rows)]
    elif kind == "L4":          # every 4-mer: d above the key length, empty segments
        rows = acgt[(np.arange(256)[:, None] >> (2 * np.arange(4))) & 3]
    elif kind == "U3000":       # several bins per pass
        rows = synth_keys(6000, 32, 32, 15, sub_rate=1.5e-2)
    elif kind == "crowd":       # ~440 distinct keys share their first half, among 400 random ones
        rows = rng.choice(acgt, size=(1300, 32))
        rows[:900] = rows[0]
        for r in rows[:900]:    # ... and differ from one second half in up to two bases
            r[rng.integers(16, 32, size=2)] = rng.choice(acgt, size=2)
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


def _collapsed(F, reads):
    """A context holding the unique table of `reads`, and its keys in row order."""
    raw = np.frombuffer(b"".join(reads), dtype=np.uint8)
    sizes = [len(r) for r in reads]
    ctx = F.Context(0)
    if min(sizes) == max(sizes):
        ctx.pack_keys(raw, None, sizes[0])
    else:
        ctx.pack_keys(raw, np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64))
    n_unique = ctx.collapse()
    first = ctx.unique_table(n_unique, labels=False, kept=False)[0]
    return ctx, [reads[int(i)] for i in first]


def _edges(ctx, d):
    e = np.empty((ctx.find_edges(d), 2), dtype=np.uint32)
    ctx.export_edges(e)
    found = sorted(map(tuple, e.tolist()))
    assert len(set(found)) == len(found), "an edge is listed twice"
    return found


@pytest.mark.parametrize("kind,d,pin,cap", [("L32", 1, None, None), ("L32", 1, "small", None), ("L64", 1, None, None),
                                            ("lowc12", 3, None, None), ("L300", 2, None, None),
                                            ("ragged", 2, None, None), ("L4", 5, None, None),
                                            ("U3000", 1, None, "1024")])
def test_edges_equal_brute_force(F, monkeypatch, kind, d, pin, cap):
    """pack_keys -> collapse -> find_edges -> export_edges over the shapes that reach each path of the kernel; the
    search is two launches (segment hashes + the small search) unless the edge buffer had to grow."""
    if pin:
        monkeypatch.setenv("FQD_EDGES", pin)
    if cap:
        monkeypatch.setenv("FQD_SMALL_CAP", cap)
    ctx, keys = _collapsed(F, _reads(kind))
    ctx.kernel_times(reset=True)
    found = _edges(ctx, d)
    route, kt = ctx.route(), ctx.kernel_times(reset=True)
    assert route["search_small"] and not route["search_sort"], route
    assert found == _brute(keys, d)
    assert kt["segment_hashes_kernel"][1] == 1 and kt["bucket_pairs_kernel"][1] == 1 + route["search_retried"], kt
    assert ctx.edge_stats()["edges"] == len(found)


def test_distance_zero_on_an_uncollapsed_table(F):
    """import_unique of rows with repeated keys, as the dissection of a caller's cluster does: every equal pair is an edge."""
    rng = np.random.default_rng(3)
    reads = [bytes(r) for r in rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=(40, 20))]
    reads = [reads[i] for i in rng.integers(0, 40, size=200)]
    ctx = F.Context(0)
    n = ctx.pack_keys(np.frombuffer(b"".join(reads), dtype=np.uint8), None, 20)
    recs, lens = np.empty(n * ctx.shape().stride_words, dtype=np.uint32), np.empty(n, dtype=np.uint32)
    ctx.export_packed(recs, lens, np.empty(n, dtype=np.uint32))
    ctx.import_unique(recs, lens, np.ones(n, dtype=np.uint32), np.arange(n, dtype=np.uint64), n)
    assert _edges(ctx, 0) == _brute(reads, 0)
    assert ctx.route()["search_small"]


@pytest.mark.parametrize("cap", [None, "64"])
def test_crowded_chain(F, monkeypatch, cap):
    """One segment value shared by ~440 keys: the wave-cooperative phase; with 64 items per workgroup the bin overflows
    and the search runs again on the sort path -- never an error."""
    if cap:
        monkeypatch.setenv("FQD_SMALL_CAP", cap)
    ctx, keys = _collapsed(F, _reads("crowd"))
    assert _edges(ctx, 1) == _brute(keys, 1)
    route = ctx.route()
    if cap:
        assert route["search_sort"] and route["search_retried"] and not route["search_small"], route
    else:
        assert route["search_small"] and not route["search_sort"], route


@pytest.mark.parametrize("d", [1, 2])
@pytest.mark.parametrize("method", METHODS)
def test_cluster_keys_takes_the_small_route(F, oracle, method, d):
    from fastqdedup_amd.synth import fixed_offsets, synth_keys
    n, L = 5000, 32
    raw = np.ascontiguousarray(synth_keys(n, L, 12, 21, sub_rate=5e-3)).reshape(-1)
    want = oracle.dedup(raw, fixed_offsets(n, L), max_distance=d, method=method)
    got = F.cluster_keys(raw, key_len=L, max_distance=d, method=method, context=F.Context(0))
    assert (got.n_unique, got.n_clusters) == (want["n_unique"], want["n_clusters"])
    assert np.array_equal(got.kept_read_ids, want["kept_read_ids"])
    assert got.route["search_small"], got.route


def test_dissection_of_a_cluster_takes_the_small_route(F, oracle):
    rng = np.random.default_rng(5)
    stem = rng.integers(0, 4, size=16)
    cluster = []
    for i in range(40):         # 40 distinct keys one substitution away from the stem
        key = stem.copy()
        key[i % 16] = (stem[i % 16] + 1 + i // 16) % 4
        cluster.append((int(rng.integers(1, 60)), bytes(np.frombuffer(b"ACGT", dtype=np.uint8)[key]).decode()))
    got = list(F.cluster_dissection_directional(cluster, 1))
    assert len(got) == len(set(got)) and set(got) == set(oracle.cluster_dissection_directional(cluster, 1))
    assert F.default_context().route()["search_small"]


def test_small_and_sorted_search_agree_on_one_table(F, monkeypatch):
    ctx, _ = _collapsed(F, _reads("U3000"))
    found = {}
    for mode in ("small", "sort"):
        monkeypatch.setenv("FQD_EDGES", mode)
        found[mode] = _edges(ctx, 2)
        assert ctx.route()["search_" + mode] and ctx.edge_stats()["edges"] == len(found[mode])
    assert found["small"] == found["sort"] and found["small"]
