"""Pass-1 wall time of the command line on both ingest routes (FQD_INGEST=host / device), measured alternately in
one process: from the call of ``deduplicate_cluster`` to its call of ``cluster_keys`` (not included; the device is
synchronised first). Then, in a run of its own, the ingest kernels' times and the gather kernel's bytes per second
beside ``Context.copy_bandwidth``. Input: tools/make_synth_fastq.py. Prints one JSON line.

    python tools/bench_ingest.py R1.fastq R2.fastq [--repeats 3] [-l 16,16]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fastqdedup_amd as F  # noqa: E402
from fastqdedup_amd import cli  # noqa: E402


class _Reached(Exception):
    pass


def pass1_seconds(files, slices, route, ctx, seen):
    def stop(keys, offsets=None, key_len=0, weights=None, **kw):
        ctx.synchronize()
        seen["t"] = time.perf_counter()
        seen["n"] = (keys.numel() if hasattr(keys, "numel") else keys.size) // key_len if key_len else len(offsets) - 1
        raise _Reached

    os.environ["FQD_INGEST"] = route
    real, cli.cluster_keys = cli.cluster_keys, stop
    t0 = time.perf_counter()
    try:
        cli.deduplicate_cluster(files, [os.devnull] * len(files), slices)
    except _Reached:
        pass
    finally:
        cli.cluster_keys = real
    return seen["t"] - t0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("fastq", nargs="+")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("-l", "--check-lengths")
    a = ap.parse_args()
    import torch
    slices = cli.length_string_to_slices(a.check_lengths) if a.check_lengths else None
    ctx, seen = F.core.default_context(), {}
    ctx.set_timing(False, ())
    out = {"files": a.fastq, "check_lengths": a.check_lengths, "host_s": [], "device_s": []}
    pass1_seconds(a.fastq, slices, "device", ctx, seen)          # warm-up: code objects, page-locked blocks, file cache
    for _ in range(a.repeats):
        for route in ("host", "device"):
            out[route + "_s"].append(round(pass1_seconds(a.fastq, slices, route, ctx, seen), 4))
    out["records"] = seen["n"]
    ingest = [k for k in ctx.KERNELS if k.startswith("fastq_")]
    ctx.set_timing(False, ingest)
    ctx.kernel_times(reset=True)
    pass1_seconds(a.fastq, slices, "device", ctx, seen)
    kt = ctx.kernel_times(reset=True)
    out["kernel_ms"] = {k: [round(kt[k][0], 4), kt[k][1]] for k in ingest}
    moved = sum(os.path.getsize(p) for p in a.fastq) + ctx.fastq_stats()["key_bytes"]    # bytes staged + key bytes written
    out["gather_gbs"] = round(moved / (kt["fastq_gather_kernel"][0] * 1e-3) / 1e9, 1)
    src = torch.empty(256 << 20, dtype=torch.uint8, device="cuda")
    out["copy_gbs"] = round(ctx.copy_bandwidth(src, torch.empty_like(src)), 1)
    print(json.dumps(out))
