"""Crowded buckets all pairs in tiles for the record shapes `gp_wide_tiles_kernel<K, QMAX>` adds
(csrc/group_tiles_wide.hip): any number of uint4 per record up to 16, one to four bit planes. The skewed model with a
ladder big enough to crowd a bucket, against the oracle's trie (`TrieNode_FindNearest`, `_triemodule.c:380-495`) on the
same bytes, with the route the job took asserted. GPU only."""
import functools
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SKEW = {"hot": 0.02, "ladder": 0.08, "lowc_every": 100}
METHODS = ("directional", "adjacency")


@pytest.fixture(scope="module")
def F():
    import fastqdedup_amd
    return fastqdedup_amd


@functools.lru_cache(maxsize=None)
def _reads(alphabet, L, n):
    """The bytes of one input: n reads, the fewer the longer the key (the oracle's trie walks the ladder too, its time
    grows with the ladder's square), and about one substitution per read at most, so that most of a ladder stays one
    family on 600-nt keys as well. "iupac9": every seventh column of the ACGNT input written in R, Y, K, M (a bijection per
    column: every Hamming distance is kept, nine symbols, four planes); "ac": G folded onto A and T onto C (one plane)."""
    from fastqdedup_amd.synth import synth_keys
    keys = synth_keys(n, L, 12, 300 + L, sub_rate=3e-3 if L <= 200 else 1e-3, n_rate=0 if alphabet == "ac" else 1e-4,
                      skew=SKEW)
    lut = np.arange(256, dtype=np.uint8)
    if alphabet == "iupac9":
        lut[list(b"ACGT")] = list(b"RYKM")
        keys[:, ::7] = lut[keys[:, ::7]]
    elif alphabet == "ac":
        lut[list(b"GT")] = list(b"AC")
        keys = lut[keys]
    raw = np.ascontiguousarray(keys).reshape(-1)
    raw.setflags(write=False)
    return raw


@functools.lru_cache(maxsize=None)
def _want(oracle, alphabet, L, n, d, method):
    from fastqdedup_amd.synth import fixed_offsets
    return oracle.dedup(_reads(alphabet, L, n), fixed_offsets(n, L), max_distance=d, method=method)


def _context(F, alphabet, L):
    ctx = F.Context(0)
    if alphabet == "ac":            # (two symbols are a subset of the default alphabet: the planes have to be said)
        present = np.zeros(128, dtype=np.uint8)
        present[list(b"AC")] = 1
        ctx.configure(present, L, False)
    return ctx


def _taken(got):
    return sorted(k for k, v in got.route.items() if v)


def _same(got, want, note):
    assert (got.n_unique, got.n_clusters, got.n_kept) == (want["n_unique"], want["n_clusters"],
                                                          len(want["kept_read_ids"])), (note, _taken(got))
    assert np.array_equal(got.kept_read_ids, want["kept_read_ids"]), note


# what each case pins: six uint4 (no power of two), K * W = 21 with three padding words | twelve uint4, above 128 bytes,
# in through the fine pieces' overflow and the sticky flag | fifteen uint4, W = 19 with a partial last word | the largest
# row, K * W = 63 of 64, d = 4 without fine pieces | K = 4 at four uint4 | K = 1 at one uint4 | L = 200 again with the
# crowding limit at 64: hundreds of buckets of 65 to 200 items -- single tiles, short last rows, no multiple of 128
@pytest.mark.parametrize("alphabet,L,n,d,env", [
    ("ACGNT", 200, 40_000, 2, {}),
    ("ACGNT", 500, 50_000, 1, {"FQD_GROUP_TILE_BUDGET": "0", "FQD_GROUP_CAND_BUDGET": "300000"}),
    ("ACGNT", 600, 30_000, 2, {}),
    ("ACGNT", 672, 20_000, 4, {}),
    ("iupac9", 100, 80_000, 2, {}),
    ("ac", 128, 80_000, 1, {}),
    ("ACGNT", 200, 40_000, 2, {"FQD_GROUP_CROWDED_LIMIT": "64"}),
])
def test_wide_and_odd_records_go_all_pairs_in_tiles(F, oracle, monkeypatch, alphabet, L, n, d, env):
    monkeypatch.setenv("FQD_EDGES", "grouped")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    raw = _reads(alphabet, L, n)
    ctx = _context(F, alphabet, L)
    for method in METHODS:          # (two jobs on one context: the second meets its sticky flags warm)
        got = F.cluster_keys(raw, key_len=L, max_distance=d, method=method, context=ctx)
        _same(got, _want(oracle, alphabet, L, n, d, method), (alphabet, L, d, method))
        assert got.route["search_tiles"] and not got.route["search_sort"], (method, _taken(got))


@pytest.mark.parametrize("d", [1, 2])
def test_wide_tiles_of_ragged_keys(F, oracle, monkeypatch, d):
    """Keys of 195 to 205 nt that share a 130-base stem by the thousand, with stems cut short and stems extended by A
    (code 0: equal rows of different lengths are different keys; a pair's segments are those of ITS length)."""
    rng = random.Random(60 + d)
    monkeypatch.setenv("FQD_EDGES", "grouped")
    monkeypatch.setenv("FQD_GROUP_TILE_BUDGET", "1000000000000")
    stem = "".join(rng.choice("ACGT") for _ in range(130))
    mols = [stem + "".join(rng.choice("ACGT") for _ in range(rng.randint(65, 75))) for _ in range(6000)]
    mols += ["".join(rng.choice("ACGT") for _ in range(rng.randint(195, 205))) for _ in range(6000)]
    strs = []
    for _ in range(60_000):
        m = list(rng.choice(mols))
        for _ in range(rng.choice((0, 0, 0, 1, 1, 2))):
            m[rng.randrange(len(m))] = rng.choice("ACGT")
        strs.append("".join(m))
    strs += [stem[:k] for k in range(120, 131)] * 2 + [stem + "A" * k for k in range(60, 76)]
    raw = np.frombuffer("".join(strs).encode(), dtype=np.uint8)
    off = np.concatenate([[0], np.cumsum([len(s) for s in strs])]).astype(np.uint64)
    ctx = F.Context(0)
    for method in METHODS:
        want = oracle.dedup(raw, off, max_distance=d, method=method)
        for job in range(2):
            got = F.cluster_keys(raw, off, max_distance=d, method=method, context=ctx)
            _same(got, want, (d, method, job))
    assert got.route["search_tiles"] and not got.route["search_sort"], _taken(got)


def test_rows_over_256_bytes_stay_off_the_tiles(F, oracle, monkeypatch):
    """The far side of the limit: 700-nt keys over ACGNT are rows of 68 words. Same result, no tiles, no error."""
    monkeypatch.setenv("FQD_EDGES", "grouped")
    raw = _reads("ACGNT", 700, 20_000)
    ctx = F.Context(0)
    for method in METHODS:
        got = F.cluster_keys(raw, key_len=700, max_distance=2, method=method, context=ctx)
        _same(got, _want(oracle, "ACGNT", 700, 20_000, 2, method), method)
        assert not got.route["search_tiles"], (method, _taken(got))
