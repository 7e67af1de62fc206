"""Writes an uncompressed synthetic paired FASTQ (R1, R2) from fastqdedup_amd/synth.py's read model: read i of
``synth_keys(n, 2 * length, umi, seed)`` is split into its two mates; qualities are a pure function of (seed, read,
position) too -- mostly 'I', one base in 16 lower, so a share of the reads fails the default quality gate.

    python tools/make_synth_fastq.py OUT_PREFIX [--pairs 2000000] [--length 100] [--seed 1001]

-> OUT_PREFIX_R1.fastq, OUT_PREFIX_R2.fastq (every record ``@r<9 digits>/<mate>\\nSEQ\\n+\\nQUAL\\n``)."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fastqdedup_amd.synth import stream_hash, synth_keys_range  # noqa: E402


def write_pair(prefix: str, pairs: int, length: int, seed: int, umi: int = 8, piece: int = 250_000):
    paths = [f"{prefix}_R{m}.fastq" for m in (1, 2)]
    outs = [open(p, "wb") for p in paths]
    seq0 = 14                                  # "@r" + 9 digits + "/" + mate + newline
    width = seq0 + length + 3 + length + 1
    for start in range(0, pairs, piece):
        count = min(piece, pairs - start)
        keys = synth_keys_range(pairs, start, count, 2 * length, umi, seed)
        idx = np.arange(start, start + count, dtype=np.uint64)
        at = idx[:, None] * np.uint64(length) + np.arange(length, dtype=np.uint64)
        for m, out in enumerate(outs):
            rec = np.empty((count, width), dtype=np.uint8)
            rec[:, 0], rec[:, 1], rec[:, 11], rec[:, 12], rec[:, 13] = ord("@"), ord("r"), ord("/"), ord("1") + m, 10
            for d in range(9):
                rec[:, 10 - d] = ord("0") + (idx // np.uint64(10 ** d)) % np.uint64(10)
            rec[:, seq0:seq0 + length] = keys[:, m * length:(m + 1) * length]
            rec[:, seq0 + length:seq0 + length + 3] = np.frombuffer(b"\n+\n", dtype=np.uint8)
            h = stream_hash(seed, 101 + m, at)
            low = (h & np.uint64(15)) == 0
            rec[:, seq0 + length + 3:width - 1] = np.where(low, 35 + (h >> np.uint64(8)) % np.uint64(30), 73)
            rec[:, width - 1] = 10
            out.write(rec.tobytes())
    for out in outs:
        out.close()
    return paths


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("prefix")
    ap.add_argument("--pairs", type=int, default=2_000_000)
    ap.add_argument("--length", type=int, default=100)
    ap.add_argument("--seed", type=int, default=1001)
    a = ap.parse_args()
    print(*write_pair(a.prefix, a.pairs, a.length, a.seed))
