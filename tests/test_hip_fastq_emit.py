"""The device-side FASTQ emit (csrc/fastq_emit.hip, fastq.DeviceEmit) against plain Python on the list of records:
the kept records as ``@name\\nseq\\n+\\nqual\\n``, byte for byte. No tolerances."""
import gzip
import io
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def F():
    import fastqdedup_amd
    return fastqdedup_amd


@pytest.fixture(scope="module")
def ctx(F):
    return F.Context(0)


def _rec(rng, i, length, mate=1, name=None):
    seq = "".join(rng.choice("ACGTN") for _ in range(length))
    q = "".join(chr(rng.choice([73, 73, 60, 45, 35])) for _ in range(length))
    return (name or f"r{i}/{mate} lane{mate}", seq, q)


def _sized(rng, i, size):
    """A record whose output is ``size`` bytes long (name + 2 * sequence + 6), sized through its name."""
    length = (size - 8) // 2
    return _rec(rng, i, length, name="abc"[: size - 6 - 2 * length])


def _text(recs, eol="\n", plus="+", tail="", strip=False):
    t = ("".join(f"@{n}{eol}{s}{eol}{plus}{eol}{q}{eol}" for n, s, q in recs) + tail).encode()
    return t[:-1] if strip else t


def _want(recs, keep):
    return b"".join(b"@%s\n%s\n+\n%s\n" % tuple(x.encode() for x in recs[i]) for i in keep if i < len(recs))


def _emit(F, ctx, tmp_path, texts, keep, **kw):
    paths = []
    for f, t in enumerate(texts):
        paths.append(str(tmp_path / f"in{f}.fastq"))
        open(paths[-1], "wb").write(t)
    outs = [io.BytesIO() for _ in texts]
    de = F.fastq.DeviceEmit(ctx, paths, outs, np.array(keep, dtype=np.uint64), **kw).run()
    return de, [o.getvalue() for o in outs]


def _shapes(rng):
    from fastqdedup_amd._lib import FASTQ_EMIT_TILE
    ragged = [_rec(rng, i, rng.randint(0, 301)) for i in range(700)]        # many tiles, spans off 16 bytes
    return {
        "one_record": ([_rec(rng, 0, 50)], {}),
        "empty_sequence": ([_rec(rng, 0, 20), ("e", "", ""), _rec(rng, 2, 20)], {}),
        "crlf": (ragged[:40], dict(eol="\r\n")),
        "plus_name": (ragged[:40], dict(plus="+name again")),
        "no_last_newline": (ragged[:9], dict(strip=True)),
        "trailing_blank_lines": (ragged[:9], dict(tail="\n\n")),
        "ragged_0_to_301": (ragged, {}),
        "record_longer_than_two_tiles": (ragged[:5] + [_sized(rng, 5, 2 * FASTQ_EMIT_TILE + 234)] + ragged[6:12], {}),
    }


PATTERNS = {
    "none": lambda n, rng: [],
    "all": lambda n, rng: list(range(n)),
    "first": lambda n, rng: [0],
    "last": lambda n, rng: [n - 1],
    "every_third": lambda n, rng: list(range(0, n, 3)),
    "random_half": lambda n, rng: sorted(rng.sample(range(n), n // 2)),
}


@pytest.mark.parametrize("pattern", list(PATTERNS))
@pytest.mark.parametrize("shape", ["one_record", "empty_sequence", "crlf", "plus_name", "no_last_newline",
                                   "trailing_blank_lines", "ragged_0_to_301", "record_longer_than_two_tiles"])
def test_record_shapes_and_keep_patterns(F, ctx, tmp_path, shape, pattern):
    recs, how = _shapes(random.Random(5))[shape]
    keep = PATTERNS[pattern](len(recs), random.Random(6))
    de, got = _emit(F, ctx, tmp_path, [_text(recs, **how)], keep)
    assert got == [_want(recs, keep)]
    assert (de.n, de.n_emitted) == (len(recs), len(keep))


@pytest.mark.parametrize("more", [0, 3])
@pytest.mark.parametrize("edge", ["ends_before", "ends_at", "ends_behind", "after_at", "in_name", "before_sequence",
                                  "in_plus_line", "in_quality", "on_last_newline"])
def test_tile_edges(F, ctx, tmp_path, edge, more):
    """One record whose output ends at T - 1, T and T + 1 bytes; then a second record that the tile's end cuts at byte
    ``cut`` of its output, once in each of its pieces."""
    from fastqdedup_amd._lib import FASTQ_EMIT_TILE as T
    rng = random.Random(len(edge) + more)
    second = _rec(rng, 1, 40, name="second")           # '@' 0, name 1-6, '\n' 7, sequence 8-47, "\n+\n" 48-50, quality 51-90, '\n' 91
    ends = {"ends_before": T - 1, "ends_at": T, "ends_behind": T + 1}
    cut = {"after_at": 1, "in_name": 4, "before_sequence": 7, "in_plus_line": 49, "in_quality": 70, "on_last_newline": 91}
    recs = [_sized(rng, 0, ends[edge])] if edge in ends else [_sized(rng, 0, T - cut[edge]), second]
    recs += [_rec(rng, i, 30 + i) for i in range(2, more + 2)]
    assert len(_want(recs[:1], [0])) == (ends[edge] if edge in ends else T - cut[edge])
    keep = list(range(len(recs)))
    assert _emit(F, ctx, tmp_path, [_text(recs)], keep)[1] == [_want(recs, keep)]


@pytest.mark.parametrize("block_bytes", [1999, 1 << 20])
@pytest.mark.parametrize("n_files", [1, 2, 3])
def test_files_blocks_and_chunks(F, ctx, tmp_path, n_files, block_bytes):
    """Files of unequal record counts, records that straddle blocks, chunks of 257 records; kept ids on both sides of
    the chunk ends and at or beyond the shortest file's record count."""
    rng = random.Random(n_files)
    files = [[_rec(rng, i, rng.randint(20, 90) // (f + 1), mate=f + 1) for i in range(900 + 40 * ((f + 1) % 3))]
             for f in range(n_files)]
    n = min(len(r) for r in files)
    edges = {0, 255, 256, 257, 258, 513, 514, 770, 771, n - 1, n, n + 5, 10 ** 6}
    keep = sorted(edges | set(rng.sample(range(n), 200)))
    de, got = _emit(F, ctx, tmp_path, [_text(r) for r in files], keep, block_bytes=block_bytes, chunk_records=257)
    for f, recs in enumerate(files):
        assert got[f] == _want(recs[:n], keep), f
    assert (de.n, de.n_emitted) == (n, sum(1 for i in keep if i < n))


def test_cursor_and_capacity_faults(F, ctx):
    import torch
    rng = random.Random(9)
    recs = [_rec(rng, i, 33 + i) for i in range(6)]
    want = _want(recs, [1, 2, 4])
    ctx.fastq_emit_begin(1)
    assert ctx.fastq_index(0, np.frombuffer(_text(recs), dtype=np.uint8), final=True).n_records == 6
    kept = torch.tensor([3, 11, 12, 14], dtype=torch.int64, device="cuda")
    buf = torch.full((len(want) + 32,), 0xAA, dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError, match="below base_id"):
        ctx.fastq_emit(6, 10, kept, 4, 0, [buf])                     # the cursor points at id 3, the chunk starts at 10
    with pytest.raises(ValueError, match="out_capacity is too small"):
        ctx.fastq_emit(6, 10, kept, 4, 1, [buf[: len(want) - 1]])
    assert bool((buf[len(want) - 1:] == 0xAA).all())
    info = ctx.fastq_emit(6, 10, kept, 4, 1, [buf[: len(want)]])
    assert (info.n_emitted, info.out_bytes[0], info.consumed[0]) == (3, len(want), len(_text(recs)))
    assert bytes(buf[: len(want)].cpu().numpy()) == want and bool((buf[len(want):] == 0xAA).all())


def test_command_line_same_output_on_all_routes(F, tmp_path, monkeypatch):
    rng = random.Random(8)
    mols = [("".join(rng.choice("ACGT") for _ in range(50)), "".join(rng.choice("ACGT") for _ in range(50)))
            for _ in range(200)]
    r1, r2 = [], []
    for i in range(1500):
        a, b = rng.choice(mols)
        r1.append((f"r{i}/1 lane1", a, "".join(chr(rng.choice([73, 73, 73, 40])) for _ in range(50))))
        r2.append((f"r{i}/2 lane2", b, "I" * 50))
    f1, f2 = str(tmp_path / "a.fastq.gz"), str(tmp_path / "b.fastq.gz")
    gzip.open(f1, "wb").write(_text(r1, plus="+r again"))
    gzip.open(f2, "wb").write(_text(r2, plus="+r again"))
    ctx, outs = F.core.default_context(), {}
    for ingest in ("device", "host"):
        for emit in ("device", "host"):
            monkeypatch.setenv("FQD_INGEST", ingest)
            monkeypatch.setenv("FQD_EMIT", emit)
            ctx.fastq_begin(2)
            o = [str(tmp_path / f"{ingest}_{emit}{k}.fastq") for k in (1, 2)]
            F.main([f1, f2, "-o", o[0], "-o", o[1], "-l", "4:20,::2", "-e", "0.01", "-q"])
            outs[ingest, emit] = [open(p, "rb").read() for p in o]
            assert ctx.fastq_stats()["records"] == (1500 if ingest == "device" else 0)
    assert all(v == outs["host", "host"] for v in outs.values()) and len(outs["host", "host"][0]) > 0
