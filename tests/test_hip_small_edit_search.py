"""The two-launch Levenshtein search of small unique tables (csrc/small_edit_search.hip, route bit
`search_small_edit`) against a plain all-pairs Levenshtein: the full integer DP table in numpy over the pairs of two
length classes (the CPU oracle's within_distance per pair for 300-nt keys). Edge sets must be equal. GPU only."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


@pytest.fixture(scope="module")
def F():
    import fastqdedup_amd
    return fastqdedup_amd


def _edited(rng, key, n_edits, syms=ACGT, indels=True):
    """`key` (uint8 array) after n_edits random substitutions, insertions or deletions, the key's ends included."""
    key = list(key)
    for _ in range(n_edits):
        op = rng.integers(0, 3 if indels else 1)
        at = int(rng.integers(0, len(key) + (op == 1)))
        if op == 0:
            key[at] = rng.choice(syms)
        elif op == 1:
            key.insert(at, rng.choice(syms))
        else:
            del key[at]
    return np.array(key, dtype=np.uint8)


def _family(rng, n, length, copies, d, syms=ACGT, indels=True):
    out = []
    for _ in range(n):
        stem = rng.choice(syms, size=length)
        out += [stem] + [_edited(rng, stem, int(rng.integers(1, d + 1)), syms, indels) for _ in range(copies)]
    return out


def _reads(kind):
    """(reads as a list of key bytes, d) of one case."""
    rng = np.random.default_rng(17)
    if kind == "own_class":     # one length: substitutions, and rotations by one base (an insertion + a deletion)
        rows = _family(rng, 70, 24, 2, 2, indels=False)
        rows += [np.roll(r, 1) for r in rows[::3]] + [np.roll(r, -1) for r in rows[1::3]]
        d = 2
    elif kind == "one_indel":   # 30 / 31 / 32 bases
        rows, d = [], 1
        for _ in range(110):
            stem = rng.choice(ACGT, size=32)
            mid = np.delete(stem, rng.integers(0, 32))
            rows += [stem, mid, np.delete(mid, rng.integers(0, 31)), _edited(rng, stem, 1, indels=False)]
    elif kind == "word_boundary":   # 62 .. 66 bases over ACGTN: segments across a 32-base word, shifts off either end
        rows, d = _family(rng, 60, 64, 3, 3, syms=np.frombuffer(b"ACGTN", dtype=np.uint8)), 3
    elif kind == "empty_segments":  # every string over AC of 1 .. 6 bases: d above the key length
        rows, d = [ACGT[(n >> np.arange(L)) & 1] for L in range(1, 7) for n in range(1 << L)], 3
    elif kind == "long_rows":   # rows compared from global memory
        rows, d = _family(rng, 50, 300, 2, 1), 2
    elif kind == "bins":        # 20 .. 22 bases
        rows, d = _family(rng, 400, 21, 2, 1), 2
    elif kind == "crowd":       # ~300 distinct keys share their first half
        stem = rng.choice(ACGT, size=16)
        rows, d = [np.concatenate([stem, r]) for r in _family(rng, 105, 16, 2, 2, indels=False)], 2
    elif kind == "repeats":     # rows with repeated keys, ragged
        rows, d = _family(rng, 30, 20, 2, 1), 1
        rows = [rows[i] for i in rng.integers(0, len(rows), size=200)]
    return [bytes(r) for r in rows], d


def _lev(a, b):
    """Levenshtein distances [len(a), len(b)] of the rows of a (n x la) and b (m x lb): the whole DP table, row by row."""
    (n, la), (m, lb) = a.shape, b.shape
    ramp = np.arange(lb + 1, dtype=np.int16)
    prev = np.broadcast_to(ramp, (n, m, lb + 1))
    for i in range(1, la + 1):
        best = np.minimum(prev[:, :, :-1] + (a[:, None, i - 1, None] != b[None, :, :]), prev[:, :, 1:] + 1)
        cur = np.concatenate([np.full((n, m, 1), i, dtype=np.int16), best], axis=2)
        prev = np.minimum.accumulate(cur - ramp, axis=2) + ramp       # insertions: cur[j] = min over k <= j of cur[k] + j - k
    return prev[:, :, lb]


def _brute(keys, d, oracle=None):
    """Sorted (i, j), i < j, of the keys within Levenshtein distance d."""
    if oracle is not None:
        strs = [k.decode() for k in keys]
        return sorted((i, j) for i in range(len(keys)) for j in range(i + 1, len(keys))
                      if abs(len(keys[i]) - len(keys[j])) <= d and oracle.within_distance(strs[i], strs[j], d, True))
    lens = np.array([len(k) for k in keys])
    rows = {L: (np.flatnonzero(lens == L), np.frombuffer(b"".join(k for k in keys if len(k) == L), dtype=np.uint8)
                .reshape(-1, L)) for L in np.unique(lens)}
    out = []
    for la, (ia, a) in rows.items():
        for lb, (ib, b) in rows.items():
            if la <= lb <= la + d:
                r, c = np.nonzero(_lev(a, b) <= d)
                out += [(int(i), int(j)) for i, j in zip(ia[r], ib[c]) if (i < j if la == lb else True)]
    return sorted((min(e), max(e)) for e in out)


def _table(F, reads, collapse=True):
    """A context holding the unique table of `reads` (or, uncollapsed, one row per read), and its keys in row order."""
    raw = np.frombuffer(b"".join(reads), dtype=np.uint8)
    sizes = [len(r) for r in reads]
    ctx = F.Context(0)
    if min(sizes) == max(sizes):
        n = ctx.pack_keys(raw, None, sizes[0])
    else:
        n = ctx.pack_keys(raw, np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64))
    if collapse:
        first = ctx.unique_table(ctx.collapse(), labels=False, kept=False)[0]
        return ctx, [reads[int(i)] for i in first]
    recs, lens = np.empty(n * ctx.shape().stride_words, dtype=np.uint32), np.empty(n, dtype=np.uint32)
    ctx.export_packed(recs, lens, np.empty(n, dtype=np.uint32))
    ctx.import_unique(recs, lens, np.ones(n, dtype=np.uint32), np.arange(n, dtype=np.uint64), n)
    return ctx, reads


def _edges(F, ctx, d):
    from fastqdedup_amd._lib import METRIC_EDIT
    e = np.empty((ctx.find_edges(d, METRIC_EDIT), 2), dtype=np.uint32)
    ctx.export_edges(e)
    found = sorted(map(tuple, e.tolist()))
    assert len(set(found)) == len(found), "an edge is listed twice"
    return found


@pytest.fixture(scope="module")
def crowd(F):
    reads, d = _reads("crowd")
    ctx, keys = _table(F, reads)
    return ctx, d, _brute(keys, d)


@pytest.mark.parametrize("kind,cap", [("own_class", None), ("one_indel", None), ("word_boundary", None),
                                      ("empty_segments", None), ("long_rows", None), ("bins", "256"), ("repeats", None)])
def test_edges_equal_all_pairs_levenshtein(F, oracle, monkeypatch, kind, cap):
    if cap:
        monkeypatch.setenv("FQD_SMALL_CAP", cap)
    reads, d = _reads(kind)
    ctx, keys = _table(F, reads, collapse=kind != "repeats")
    found = _edges(F, ctx, d)
    route = ctx.route()
    assert route["search_small_edit"] and route["search_edit"] and not route["search_retried"], route
    want = _brute(keys, d, oracle if kind == "long_rows" else None)
    assert found == want and want
    assert ctx.edge_stats()["edges"] == len(found)


@pytest.mark.parametrize("cap", [None, "64"])
def test_crowded_chain(F, monkeypatch, crowd, cap):
    """One segment value shared by ~300 keys: the wave-cooperative phase; with 64 items per workgroup the bin overflows
    and the search runs again the sorted way -- never an error."""
    if cap:
        monkeypatch.setenv("FQD_SMALL_CAP", cap)
    ctx, d, want = crowd
    assert _edges(F, ctx, d) == want and want
    route = ctx.route()
    assert route["search_edit"] and route["search_small_edit"] == (cap is None) and route["search_retried"] == (cap is not None), route


def test_small_and_sorted_search_agree_on_one_table(F, monkeypatch):
    reads, d = _reads("bins")
    ctx, _ = _table(F, reads)
    found = {}
    for mode in ("small", "sort"):
        monkeypatch.setenv("FQD_EDIT", mode)
        found[mode] = _edges(F, ctx, d)
        assert ctx.route()["search_small_edit"] == (mode == "small") and ctx.edge_stats()["edges"] == len(found[mode])
    assert found["small"] == found["sort"] and found["small"]


@pytest.fixture(scope="module")
def mixed_reads():
    rng = np.random.default_rng(23)
    reads = [bytes(r) for r in _family(rng, 500, 26, 5, 2)]
    return np.frombuffer(b"".join(reads), dtype=np.uint8), np.concatenate([[0], np.cumsum([len(r) for r in reads])]).astype(np.uint64)


@pytest.mark.parametrize("method", ("highest_count", "adjacency", "directional"))
def test_cluster_keys_takes_the_small_route(F, oracle, mixed_reads, method):
    raw, off = mixed_reads
    want = oracle.dedup(raw, off, max_distance=2, use_edit_distance=True, method=method)
    got = F.cluster_keys(raw, off, max_distance=2, use_edit_distance=True, method=method, context=F.Context(0))
    assert (got.n_unique, got.n_clusters) == (want["n_unique"], want["n_clusters"])
    assert np.array_equal(got.kept_read_ids, want["kept_read_ids"])
    assert got.route["search_small_edit"], got.route


def test_trie_pop_cluster(F, oracle):
    rng = np.random.default_rng(29)
    a, b = F.Trie(), oracle.Trie()
    for r in _family(rng, 40, 18, 4, 2):
        a.add_sequence(bytes(r).decode())
        b.add_sequence(bytes(r).decode())
    while b.number_of_sequences:
        ca, cb = a.pop_cluster(2, True), b.pop_cluster(2, True)
        assert sorted(ca) == sorted(cb) and ca[0] == cb[0]


def test_dissection_of_a_cluster_takes_the_small_route(F, oracle):
    rng = np.random.default_rng(31)
    stem = rng.choice(ACGT, size=16)
    keys = {bytes(_edited(rng, stem, 1)).decode() for _ in range(200)}
    cluster = [(int(rng.integers(1, 60)), k) for k in sorted(keys)[:40]]
    assert len(cluster) == 40
    got = list(F.cluster_dissection_directional(cluster, 2, True))
    assert len(got) == len(set(got)) and set(got) == set(oracle.cluster_dissection_directional(cluster, 2, True))
    assert F.default_context().route()["search_small_edit"]
