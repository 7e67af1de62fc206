"""The device-side FASTQ ingest (csrc/fastq_ingest.hip, fastq.DeviceIngest) against plain Python on the list of
records: key bytes, offsets, weights, means bit for bit, discarded count, fixed-length report. No tolerances."""
import gzip
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NONE = slice(None)


@pytest.fixture(scope="module")
def F():
    import fastqdedup_amd
    return fastqdedup_amd


@pytest.fixture(scope="module")
def ctx(F):
    return F.Context(0)


def _rec(rng, i, length, mate=1, qual=None):
    seq = "".join(rng.choice("ACGTN") for _ in range(length))
    q = qual or "".join(chr(rng.choice([73, 73, 60, 45, 35])) for _ in range(length))
    return (f"r{i}/{mate} lane{mate}", seq, q)


def _text(recs, eol="\n", plus="+", tail=""):
    return ("".join(f"@{n}{eol}{s}{eol}{plus}{eol}{q}{eol}" for n, s, q in recs) + tail).encode()


def _ingest(F, ctx, tmp_path, texts, slices=None, thr=0.001, **kw):
    paths = []
    for f, t in enumerate(texts):
        paths.append(str(tmp_path / f"in{f}.fastq"))
        open(paths[-1], "wb").write(t)
    return F.fastq.DeviceIngest(ctx, paths, slices, threshold=thr, table=F.cli.SCORE_TO_ERROR_RATE,
                                want_means=True, **kw).run()


def _check(oracle, ing, files, slices=None, thr=0.001):
    """``files``: per file the list of (name, sequence, quality)."""
    n = min(len(r) for r in files)
    sl = slices or [NONE] * len(files)
    keys = ["".join(r[i][1][s] for r, s in zip(files, sl)) for i in range(n)]
    means = np.array([oracle.average_error_rate("".join(r[i][2][s] for r, s in zip(files, sl))) for i in range(n)])
    assert ing.n == n
    assert bytes(ing.keys[: ing.key_bytes].cpu().numpy()) == "".join(keys).encode()
    assert ing.offsets[: n + 1].cpu().tolist() == [0] + np.cumsum([len(k) for k in keys], dtype=np.int64).tolist()
    assert np.array_equal(ing.means[:n].cpu().numpy(), means, equal_nan=True)
    lens = {len(k) for k in keys}
    assert ing.key_len == (lens.pop() if len(lens) == 1 else 0)
    if thr < 1.0:
        want = [0 if m > thr else 1 for m in means]
        assert ing.weights[:n].cpu().tolist() == want
        assert ing.discarded == want.count(0)
    else:
        assert ing.weights is None and ing.discarded == 0


@pytest.mark.parametrize("first_end,more", [(-1, 0), (0, 0), (1, 0), (0, 3), (1, 3)])
def test_line_index_at_tile_edges(F, ctx, oracle, tmp_path, first_end, more):
    """Buffers of one line-index tile minus 1 / exactly / plus 1 byte; the first record's last newline as the last
    byte of a tile and as the first byte of the next."""
    from fastqdedup_amd._lib import FASTQ_LINE_TILE
    rng = random.Random(first_end * 7 + more)
    room = FASTQ_LINE_TILE + first_end - len(_text([("a", "", "")]))       # for the sequence and the quality string
    recs = [_rec(rng, 0, room // 2)] + [_rec(rng, i, 30 + i) for i in range(1, more + 1)]
    recs[0] = ("ab" if room % 2 else "a", recs[0][1], recs[0][2])
    text = _text(recs)
    assert len(_text(recs[:1])) == FASTQ_LINE_TILE + first_end
    _check(oracle, _ingest(F, ctx, tmp_path, [text]), [recs])


def test_more_tiles_than_one_scan_step(F, ctx, oracle, tmp_path):
    from fastqdedup_amd._lib import FASTQ_LINE_TILE, FASTQ_SCAN_STEP
    rng = random.Random(11)
    some = [_rec(rng, i, rng.randint(250, 301)) for i in range(64)]
    recs = some * ((FASTQ_SCAN_STEP + 2) * FASTQ_LINE_TILE // len(_text(some)) + 1)
    text = _text(recs)
    assert len(text) > (FASTQ_SCAN_STEP + 1) * FASTQ_LINE_TILE
    _check(oracle, _ingest(F, ctx, tmp_path, [text], block_bytes=len(text) + 1), [recs])


def _shapes(rng):
    from fastqdedup_amd._lib import FASTQ_IN_TILE
    ragged = [_rec(rng, i, rng.randint(0, 301)) for i in range(700)]     # several workgroups, key spans off 16 bytes
    return {
        "no_records": ([], {}),
        "one_record": ([_rec(rng, 0, 50)], {}),
        "empty_sequence": ([_rec(rng, 0, 20), ("e", "", ""), _rec(rng, 2, 20)], {}),
        "crlf": (ragged[:40], dict(eol="\r\n")),
        "plus_name": (ragged[:40], dict(plus="+name again")),
        "no_last_newline": (ragged[:9], dict(strip=True)),
        "trailing_blank_lines": (ragged[:9], dict(tail="\n\n")),
        "ragged_0_to_301": (ragged, {}),
        "record_larger_than_lds_tile": (ragged[:5] + [_rec(rng, 5, FASTQ_IN_TILE + 233)] + ragged[6:12], {}),
    }


@pytest.mark.parametrize("shape", ["no_records", "one_record", "empty_sequence", "crlf", "plus_name", "no_last_newline",
                                   "trailing_blank_lines", "ragged_0_to_301", "record_larger_than_lds_tile"])
def test_record_shapes(F, ctx, oracle, tmp_path, shape):
    recs, how = _shapes(random.Random(5))[shape]
    how = dict(how)
    text = _text(recs, **{k: v for k, v in how.items() if k != "strip"})
    _check(oracle, _ingest(F, ctx, tmp_path, [text[:-1] if how.get("strip") else text]), [recs])


@pytest.mark.parametrize("slc", [None, slice(16), slice(4, 20), slice(None, None, 2), slice(None, None, -1),
                                 slice(-8, None), slice(400, None)], ids=str)
@pytest.mark.parametrize("thr", [0.001, 1.0])
def test_slices_and_thresholds(F, ctx, oracle, tmp_path, slc, thr):
    rng = random.Random(21)
    r1 = [_rec(rng, i, rng.choice([0, 5, 19, 20, 33, 150, 301])) for i in range(300)]
    r2 = [_rec(rng, i, rng.choice([7, 16, 40]), mate=2) for i in range(300)]
    slices = None if slc is None else [slc, slice(None, None, 3)]
    _check(oracle, _ingest(F, ctx, tmp_path, [_text(r1), _text(r2)], slices, thr), [r1, r2], slices, thr)


@pytest.mark.parametrize("n_files", [1, 2, 3])
def test_files_blocks_and_chunks(F, ctx, oracle, tmp_path, monkeypatch, n_files):
    """Files of unequal record counts, records that straddle blocks, chunks of 257 records."""
    monkeypatch.setenv("FQD_FASTQ_BLOCK_BYTES", "1999")
    monkeypatch.setenv("FQD_FASTQ_CHUNK_RECORDS", "257")
    rng = random.Random(n_files)
    files = [[_rec(rng, i, rng.randint(20, 90) // (f + 1), mate=f + 1) for i in range(900 + 40 * ((f + 1) % 3))]
             for f in range(n_files)]
    slices = [slice(4, 60), slice(None, None, -2), None][:n_files]
    ing = _ingest(F, ctx, tmp_path, [_text(r) for r in files], slices)
    _check(oracle, ing, files, [s or NONE for s in slices])
    st = ctx.fastq_stats()
    assert (st["records"], st["key_bytes"], st["discarded"]) == (ing.n, ing.key_bytes, ing.discarded)
    assert st["chunks"] >= 4


def test_phred_byte_out_of_range(F, ctx, tmp_path):
    recs = [("a", "ACGT", "IIII"), ("b", "ACGT", "II I")]
    with pytest.raises(ValueError, match="outside the valid phred range"):
        _ingest(F, ctx, tmp_path, [_text(recs)])


@pytest.mark.parametrize("fault", ["no_at", "no_plus", "lengths", "truncated", "not_mates"])
def test_format_errors_match_the_host_route(F, tmp_path, monkeypatch, fault):
    """Each fault sits in the SECOND block; same exception class and text as FQD_INGEST=host."""
    rng = random.Random(4)
    r1 = [_rec(rng, i, 40) for i in range(60)]
    r2 = [_rec(rng, i, 40, mate=2) for i in range(60)]
    lines = _text(r1).decode().split("\n")
    k = 4 * 35
    if fault == "no_at":
        lines[k] = lines[k][1:]
    elif fault == "no_plus":
        lines[k + 2] = "-"
    elif fault == "lengths":
        lines[k + 3] = lines[k + 3][:-1]
    elif fault == "truncated":
        lines = lines[: k + 2] + [""]
    else:
        r2[35] = ("other/2", r2[35][1], r2[35][2])
    f1, f2 = str(tmp_path / "a.fastq"), str(tmp_path / "b.fastq")
    open(f1, "w").write("\n".join(lines))
    open(f2, "wb").write(_text(r2))
    monkeypatch.setenv("FQD_FASTQ_BLOCK_BYTES", "2048")
    seen = {}
    for route in ("host", "device"):
        monkeypatch.setenv("FQD_INGEST", route)
        with pytest.raises(F.fastq.FastqFormatError) as err:
            F.deduplicate_cluster([f1, f2], [str(tmp_path / "o1"), str(tmp_path / "o2")], None)
        seen[route] = (type(err.value), str(err.value))
    assert seen["device"] == seen["host"]


def test_command_line_same_output_on_both_routes(F, tmp_path, monkeypatch):
    rng = random.Random(8)
    mols = [("".join(rng.choice("ACGT") for _ in range(50)), "".join(rng.choice("ACGT") for _ in range(50)))
            for _ in range(200)]
    r1, r2 = [], []
    for i in range(1500):
        a, b = rng.choice(mols)
        r1.append(_rec(rng, i, 0)[:1] + (a, "".join(chr(rng.choice([73, 73, 73, 40])) for _ in range(50))))
        r2.append(_rec(rng, i, 0, mate=2)[:1] + (b, "I" * 50))
    f1, f2 = str(tmp_path / "a.fastq.gz"), str(tmp_path / "b.fastq.gz")
    gzip.open(f1, "wb").write(_text(r1))
    gzip.open(f2, "wb").write(_text(r2))
    ctx, outs = F.core.default_context(), {}
    for route in ("device", "host"):
        monkeypatch.setenv("FQD_INGEST", route)
        ctx.fastq_begin(2)
        o = [str(tmp_path / f"{route}{k}.fastq") for k in (1, 2)]
        F.main([f1, f2, "-o", o[0], "-o", o[1], "-l", "4:20,::2", "-e", "0.01", "-q"])
        outs[route] = [open(p, "rb").read() for p in o]
        assert ctx.fastq_stats()["records"] == (1500 if route == "device" else 0)
    assert outs["device"] == outs["host"] and len(outs["device"][0]) > 0
