"""The sort-free collapse of small inputs (csrc/small_collapse.hip, route bit `collapse_small`) against a Python dict
over the key bytes: per distinct key the summed weight and the first position, compared with the unique table as a
mapping first holder -> count. Row order is compared between two jobs only: it must be the same. GPU only."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


@pytest.fixture(scope="module")
def F():
    import fastqdedup_amd
    return fastqdedup_amd


def _rows(a):
    return [bytes(r) for r in a]


def _case(kind):
    """(reads as a list of key bytes, weights or None, read ids or None) of one case."""
    from fastqdedup_amd.synth import synth_keys
    rng = np.random.default_rng(41)
    w = ids = None
    if kind in ("fixed32", "weights", "mask_0x3F"):
        reads = _rows(synth_keys(600 if kind == "mask_0x3F" else 3000, 32, 6, 11, copies=3 if kind == "mask_0x3F" else 8))
        if kind == "weights":
            w = rng.choice(np.array([0, 1, 1, 3], dtype=np.uint32), size=len(reads))
            w[[i for i, r in enumerate(reads) if r in (reads[0], reads[7])]] = 0      # two keys without any weight
            ids = np.arange(len(reads), dtype=np.uint64) * 3 + 11
    elif kind == "fixed100":
        reads = _rows(synth_keys(2000, 100, 12, 12))
    elif kind == "fixed300":
        reads = _rows(synth_keys(1500, 300, 12, 13))
    elif kind == "two_planes":
        reads = _rows(rng.choice(ACGT, size=(300, 12))[rng.integers(0, 300, size=2000)])
    elif kind == "ragged":          # 30 .. 32 bases; a third of the stems also with one and two trailing As
        stems = _rows(rng.choice(ACGT, size=(200, 30)))
        keys = stems + [s + b"A" for s in stems[::3]] + [s + b"AA" for s in stems[::3]] + _rows(rng.choice(ACGT, size=(100, 31)))
        reads = [keys[i] for i in rng.integers(0, len(keys), size=2500)]
    elif kind == "heavy":           # 20 000 copies of one key among 10 000 other reads
        reads = _rows(synth_keys(10000, 32, 8, 14))
        reads = [reads[i] if i >= 0 else reads[0] for i in rng.permutation(np.arange(-20000, 10000))]
    elif kind in ("distinct_40000", "distinct_2000", "distinct_3000"):
        # (40 nt: from 32 768 reads on, records of one uint4 with at most three key words belong to the LDS collapse)
        reads = list(dict.fromkeys(_rows(rng.choice(ACGT, size=(int(kind[9:]), 40)))))
    elif kind == "one":
        reads = [b"ACGTACGT"]
    elif kind == "two_equal":
        reads = [b"ACGTACGT"] * 2
    return reads, w, ids


def _want(reads, w=None, ids=None):
    """{first holder: summed weight} of the keys whose weights do not sum to 0."""
    first, count = {}, {}
    for i, r in enumerate(reads):
        first.setdefault(r, i if ids is None else int(ids[i]))
        count[r] = count.get(r, 0) + (1 if w is None else int(w[i]))
    return {first[r]: c for r, c in count.items() if c}


def _collapse(F, reads, w=None, ids=None):
    """(unique table as {first holder: count}, ClusterResult, head_flags_kernel launches) of one job on a new context."""
    sizes = [len(r) for r in reads]
    fixed = min(sizes) == max(sizes)
    off = None if fixed else np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    ctx = F.Context(0)
    got = F.cluster_keys(np.frombuffer(b"".join(reads), dtype=np.uint8), off, sizes[0] if fixed else 0, w, ids,
                         max_distance=1, context=ctx)
    sorted_launches = ctx.kernel_times()["head_flags_kernel"][1]
    first, counts, _, _ = ctx.unique_table(got.n_unique, labels=False, kept=False)
    assert len(set(first.tolist())) == got.n_unique
    return dict(zip(first.tolist(), counts.tolist())), got, sorted_launches


@pytest.mark.parametrize("kind,env,small", [
    ("fixed32", {}, True), ("fixed100", {}, True), ("fixed300", {}, True), ("two_planes", {}, True), ("ragged", {}, True),
    ("weights", {}, True), ("heavy", {}, True), ("distinct_40000", {}, True), ("one", {}, True), ("two_equal", {}, True),
    ("mask_0x3F", {"FQD_SMALL_HASH_MASK": "0x3F"}, True),            # distinct keys share slots: the collision list
    ("distinct_2000", {"FQD_SMALL_HASH_MASK": "0"}, False),          # ... which overflows,
    ("distinct_3000", {"FQD_SMALL_COLLAPSE_CAP": "64"}, False)])     # and so does the table: on to the sort path
def test_unique_table_equals_dict(F, monkeypatch, kind, env, small):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    reads, w, ids = _case(kind)
    want = _want(reads, w, ids)
    table, got, sorted_launches = _collapse(F, reads, w, ids)
    assert got.route["collapse_small"] == small and got.route["collapse_sort"] == (not small), got.route
    assert (sorted_launches == 0) == small
    assert got.n_counted == (len(reads) if w is None else int(w.sum()))
    assert table == want and want


def test_sort_pin_gives_the_same_table(F, monkeypatch):
    reads, w, ids = _case("weights")
    by_default, got, _ = _collapse(F, reads, w, ids)
    assert got.route["collapse_small"]
    monkeypatch.setenv("FQD_COLLAPSE", "sort")
    by_sort, got, _ = _collapse(F, reads, w, ids)
    assert got.route["collapse_sort"] and not got.route["collapse_small"], got.route
    assert by_sort == by_default == _want(reads, w, ids)


def test_two_jobs_number_their_rows_alike(F):
    """Callers number the keys by their rows: the rows of 8 bins come out in one order, job after job."""
    reads = _case("fixed32")[0]
    orders = []
    for job in range(3):
        ctx = F.Context(0)
        ctx.pack_keys(np.frombuffer(b"".join(reads), dtype=np.uint8), None, 32)
        n_unique = ctx.collapse()
        assert ctx.route()["collapse_small"]
        orders.append(ctx.unique_table(n_unique, labels=False, kept=False)[0].tolist())
    assert orders[0] == orders[1] == orders[2] and len(set(orders[0])) == len(_want(reads))


@pytest.mark.parametrize("method", ("highest_count", "adjacency", "directional"))
def test_cluster_keys_takes_the_small_route(F, oracle, method):
    from fastqdedup_amd.synth import fixed_offsets, synth_keys
    keys = synth_keys(5000, 32, 8, 15, sub_rate=5e-3).reshape(-1)
    want = oracle.dedup(keys, fixed_offsets(5000, 32), max_distance=1, method=method)
    got = F.cluster_keys(keys, key_len=32, max_distance=1, method=method, context=F.Context(0))
    assert (got.n_unique, got.n_clusters) == (want["n_unique"], want["n_clusters"])
    assert np.array_equal(got.kept_read_ids, want["kept_read_ids"])
    assert got.route["collapse_small"] and not got.route["collapse_sort"], got.route


def test_trie_fed_in_two_batches(F):
    """Both merges of the store (the second one of resident rows with new keys) take the small route."""
    reads = [r.decode() for r in _case("ragged")[0][:400]]
    trie = F.Trie()
    for r in reads[:250]:
        trie.add_sequence(r)
    assert trie.contains_sequence(reads[0]) and trie._store().route()["collapse_small"]      # (the first merge)
    for r in reads[150:]:
        trie.add_sequence(r)
    want = {}
    for r in reads[:250] + reads[150:]:
        want[r] = want.get(r, 0) + 1
    got = {}
    while trie.number_of_sequences:
        (count, key), = trie.pop_cluster(0)
        got[key] = count
    assert got == want
    route = trie._store().route()
    assert route["collapse_small"] and not route["collapse_sort"], route
