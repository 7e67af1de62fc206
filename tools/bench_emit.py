"""Pass-2 wall time of the command line on both emit routes (FQD_EMIT=host / device), measured alternately in one
process: from ``deduplicate_cluster``'s "Found ... distinct reads" log line to its return, outputs uncompressed into
os.devnull. Then, in a run of its own, the emit kernels' times and the copy kernel's bytes per second (bytes read
from the kept records + bytes written) beside ``Context.copy_bandwidth`` -- for the kept reads of the run and, through
``fastq.DeviceEmit`` alone, with every record kept. Input: tools/make_synth_fastq.py;
``--plus-name DIR`` first writes copies whose third lines repeat the name (the form SRA dumps have) into DIR and
measures those. gzip output is bound by zlib on the host and is not measured here. Prints one JSON line.

    python tools/bench_emit.py R1.fastq R2.fastq [--repeats 3] [-l 16,16] [--plus-name DIR]"""
import argparse
import json
import logging
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fastqdedup_amd as F  # noqa: E402
from fastqdedup_amd import cli  # noqa: E402


class _FoundAt(logging.Handler):
    """Notes when the line that ends the clustering is logged: pass 2 starts there."""

    def __init__(self):
        super().__init__(logging.INFO)
        self.t = None

    def emit(self, record):
        if record.getMessage().startswith("Found "):
            self.t = time.perf_counter()


class _Count:
    def __init__(self):
        self.n = 0

    def write(self, b):
        self.n += len(b)

    def close(self):
        pass


def plus_name_copy(path: str, folder: str) -> str:
    """The file with every '+' line turned into '+name' (records of one width, as make_synth_fastq.py writes them)."""
    buf = np.fromfile(path, dtype=np.uint8)
    nl = np.flatnonzero(buf[:4096] == 10)[:4]
    width, name_end, plus = int(nl[3]) + 1, int(nl[0]), int(nl[1]) + 1
    rec = buf.reshape(-1, width)
    out = os.path.join(folder, "plus_" + os.path.basename(path))
    np.concatenate([rec[:, : plus + 1], rec[:, 1:name_end], rec[:, plus + 1:]], axis=1).tofile(out)
    return out


def pass2_seconds(files, slices, route, found):
    os.environ["FQD_EMIT"] = route
    found.t = None
    cli.deduplicate_cluster(files, [os.devnull] * len(files), slices)
    return time.perf_counter() - found.t


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("fastq", nargs="+")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("-l", "--check-lengths")
    ap.add_argument("--plus-name")
    a = ap.parse_args()
    import torch
    files = [plus_name_copy(p, a.plus_name) for p in a.fastq] if a.plus_name else a.fastq
    slices = cli.length_string_to_slices(a.check_lengths) if a.check_lengths else None
    ctx, found = F.core.default_context(), _FoundAt()
    logger = logging.getLogger("fastqdedup")
    logger.setLevel(logging.INFO)
    logger.addHandler(found)
    logger.propagate = False
    ctx.set_timing(False, ())
    out = {"files": files, "check_lengths": a.check_lengths, "host_s": [], "device_s": []}
    pass2_seconds(files, slices, "device", found)          # warm-up: code objects, page-locked blocks, file cache
    for _ in range(a.repeats):
        for route in ("host", "device"):
            out[route + "_s"].append(round(pass2_seconds(files, slices, route, found), 4))
    for route in ("host", "device"):
        out[route + "_spread_s"] = round(max(out[route + "_s"]) - min(out[route + "_s"]), 4)
    out["ratio_of_medians"] = round(float(np.median(out["host_s"]) / np.median(out["device_s"])), 2)
    # one more device pass with the emit kernels timed and the output counted
    emit = [k for k in ctx.KERNELS if k.startswith("fastq_emit_")]
    ctx.set_timing(False, emit)
    ctx.kernel_times(reset=True)
    sinks, seen = [], {}
    real_open, real_emit = cli.fastq.open_write, cli.fastq.DeviceEmit

    class _Emit(real_emit):
        def run(self):
            seen["emit"] = super().run()
            return seen["emit"]

    cli.fastq.open_write = lambda path: sinks.append(_Count()) or sinks[-1]
    cli.fastq.DeviceEmit = _Emit
    try:
        pass2_seconds(files, slices, "device", found)
    finally:
        cli.fastq.open_write, cli.fastq.DeviceEmit = real_open, real_emit
    kt = ctx.kernel_times(reset=True)
    out["kernel_ms"] = {k: [round(kt[k][0], 4), kt[k][1]] for k in emit}
    written = sum(s.n for s in sinks)
    out["records"], out["kept"], out["bytes_written"] = seen["emit"].n, seen["emit"].n_emitted, written
    moved = 2 * written - 6 * seen["emit"].n_emitted * len(files)     # of a record's output all but "@\n\n+\n\n" is read
    out["copy_kernel_gbs"] = round(moved / (kt["fastq_emit_copy_kernel"][0] * 1e-3) / 1e9, 1)
    # the other end of the kept share: every record kept, through DeviceEmit itself
    sinks = [_Count() for _ in files]
    t0 = time.perf_counter()
    every = real_emit(ctx, files, sinks, torch.arange(seen["emit"].n, dtype=torch.int64, device="cuda")).run()
    out["all_kept_s"] = round(time.perf_counter() - t0, 4)
    kt = ctx.kernel_times(reset=True)
    out["all_kept_kernel_ms"] = {k: [round(kt[k][0], 4), kt[k][1]] for k in emit}
    moved = 2 * sum(s.n for s in sinks) - 6 * every.n_emitted * len(files)
    out["all_kept_copy_kernel_gbs"] = round(moved / (kt["fastq_emit_copy_kernel"][0] * 1e-3) / 1e9, 1)
    src = torch.empty(256 << 20, dtype=torch.uint8, device="cuda")
    out["copy_gbs"] = round(ctx.copy_bandwidth(src, torch.empty_like(src)), 1)
    print(json.dumps(out))
