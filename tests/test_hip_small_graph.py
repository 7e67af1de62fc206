"""The one-launch graph stage of small unique tables (csrc/small_graph.hip, route bit `graph_small`): components,
dissection, kept flags and the kept-id list against the CPU oracle, a plain union-find, and the wide route
(FQD_GRAPH=wide) of the same library. GPU only."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

METHODS = ("highest_count", "adjacency", "directional")
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


@pytest.fixture(scope="module")
def F():
    import fastqdedup_amd
    return fastqdedup_amd


def _offsets(reads):
    return np.concatenate([[0], np.cumsum([len(r) for r in reads])]).astype(np.uint64)


def _case(kind):
    """(list of key bytes, weights or None, max_distance, use_edit_distance) of one case."""
    from fastqdedup_amd.synth import synth_keys
    rng = np.random.default_rng(5)
    w, d, edit = None, 1, False
    if kind in ("synth_d1", "synth_d2", "weights"):
        reads = [bytes(r) for r in synth_keys(5000, 32, 12, 21, sub_rate=5e-3)]
        d = 2 if kind == "synth_d2" else 1
        if kind == "weights":
            w = rng.choice(np.array([0, 0, 1, 1, 3], dtype=np.uint32), size=len(reads))
    elif kind == "with_n":
        reads = [bytes(r) for r in synth_keys(5000, 32, 12, 22, sub_rate=5e-3, n_rate=2e-2)]
    elif kind == "four_mers":        # one component of 256 keys
        reads = [bytes(ACGT[[(i >> 6) & 3, (i >> 4) & 3, (i >> 2) & 3, i & 3]]) for i in range(256)]
    elif kind in ("path_falling", "path_equal"):      # 301 keys in a path: hundreds of rounds; equal counts: rows compared
        reads = [b"A" * i + b"C" * (300 - i) for i in range(301)]
        w = np.arange(301, 0, -1, dtype=np.uint32) if kind == "path_falling" else np.full(301, 2, dtype=np.uint32)
    elif kind == "ragged_edit":      # 30 .. 32 bases, Levenshtein
        stems = [bytes(r) for r in rng.choice(ACGT, size=(300, 30))]
        keys = stems + [s + b"A" for s in stems[::3]] + [s + b"AC" for s in stems[::4]]
        reads = [keys[i] for i in rng.integers(0, len(keys), size=3000)]
        edit = True
    return reads, w, d, edit


@pytest.fixture(scope="module")
def wanted(oracle):
    """oracle.dedup of a case and method, computed once."""
    memo = {}

    def get(kind, method):
        if (kind, method) not in memo:
            reads, w, d, edit = _case(kind)
            memo[kind, method] = oracle.dedup(np.frombuffer(b"".join(reads), dtype=np.uint8), _offsets(reads), w,
                                              max_distance=d, use_edit_distance=edit, method=method)
        return memo[kind, method]
    return get


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("kind", ("synth_d1", "synth_d2", "four_mers", "path_falling", "path_equal", "weights", "with_n",
                                  "ragged_edit"))
def test_cluster_keys_against_the_oracle(F, wanted, kind, method):
    reads, w, d, edit = _case(kind)
    want = wanted(kind, method)
    ctx = F.Context(0)
    got = F.cluster_keys(np.frombuffer(b"".join(reads), dtype=np.uint8), _offsets(reads), weights=w, max_distance=d,
                         use_edit_distance=edit, method=method, context=ctx)
    assert (got.n_unique, got.n_clusters, got.n_kept) == (want["n_unique"], want["n_clusters"], len(want["kept_read_ids"]))
    assert np.array_equal(got.kept_read_ids, want["kept_read_ids"])
    assert got.route["graph_small"], got.route
    times = ctx.kernel_times()
    assert times["small_graph_kernel"][1] == 1 and times["uf_union_kernel"][1] == 0, times


def _staged(F, reads, method, d):
    ctx = F.Context(0)
    ctx.pack_keys(np.frombuffer(b"".join(reads), dtype=np.uint8), None, len(reads[0]))
    n_unique = ctx.collapse()
    uv = np.empty((ctx.find_edges(d), 2), dtype=np.uint32)
    n_clusters = ctx.components()
    small = ctx.route()["graph_small"]
    ctx.export_edges(uv)
    n_kept = ctx.dissect(F.core.METHODS[method])
    small = small and ctx.route()["graph_small"]
    _, _, labels, kept = ctx.unique_table(n_unique)
    return uv, n_clusters, labels, kept, ctx.kept_read_ids(n_kept), small


@pytest.mark.parametrize("method", METHODS)
def test_staged_calls(F, monkeypatch, method):
    reads = _case("synth_d2")[0]
    uv, n_clusters, labels, kept, ids, small = _staged(F, reads, method, 2)
    assert small and len(uv)
    parent = list(range(len(labels)))          # plain union-find: the smallest uid of every component

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for a, b in uv.tolist():
        a, b = find(a), find(b)
        parent[max(a, b)] = min(a, b)
    want = [find(x) for x in range(len(labels))]
    assert labels.tolist() == want and n_clusters == len(set(want))
    monkeypatch.setenv("FQD_GRAPH", "wide")
    _, wide_clusters, wide_labels, wide_kept, wide_ids, wide_small = _staged(F, reads, method, 2)
    assert not wide_small and wide_clusters == n_clusters
    assert np.array_equal(wide_labels, labels) and np.array_equal(wide_kept, kept) and np.array_equal(wide_ids, ids)


@pytest.mark.parametrize("method", METHODS)
def test_cluster_dissection_with_repeated_items(F, oracle, method):
    """A caller's list that repeats keys: an uncollapsed table, the relaxation sweeps for the directional method."""
    rng = np.random.default_rng(9)
    path = ["A" * i + "C" * (300 - i) for i in range(301)]
    cluster = [(1, s) for s in path] + [(int(rng.integers(1, 6)), path[i]) for i in rng.integers(0, 301, size=60)]
    name = "cluster_dissection_" + method
    assert list(getattr(F, name)(cluster, 1)) == list(getattr(oracle, name)(cluster, 1))
    assert F.core.default_context().route()["graph_small"]


@pytest.mark.parametrize("n,spread,env,small", [(5854, 1, None, True), (5855, 1, None, False), (4000, 70, None, False),
                                                (4000, 1, "wide", False), (8192, 1, "small", True),
                                                (8193, 1, "small", True)])     # (the pin: in LDS / best[] and states in global memory)
def test_boundaries_and_declines(F, oracle, monkeypatch, n, spread, env, small):
    if env:
        monkeypatch.setenv("FQD_GRAPH", env)
    rng = np.random.default_rng(3)
    # n distinct keys of 16 nt: distinct stems of 15, each ending in A and in C (pairs at distance 1)
    stems = rng.permutation(np.unique(rng.choice(ACGT, size=(n, 15)), axis=0))[: (n + 1) // 2]
    keys = rng.permutation(np.concatenate([np.c_[stems, np.full(len(stems), ord(c), dtype=np.uint8)] for c in "AC"])[:n])
    assert len(np.unique(keys, axis=0)) == n
    ids = np.arange(n, dtype=np.uint64) * spread                    # spread 70: ids over more than 2^18
    want = oracle.dedup(keys.reshape(-1), np.arange(n + 1, dtype=np.uint64) * 16, max_distance=1)
    got = F.cluster_keys(keys.reshape(-1), key_len=16, read_ids=ids if spread > 1 else None, max_distance=1,
                         context=F.Context(0))
    assert (got.n_unique, got.n_clusters) == (n, want["n_clusters"])
    assert np.array_equal(got.kept_read_ids, ids[want["kept_read_ids"]])
    assert got.route["graph_small"] == small, got.route
