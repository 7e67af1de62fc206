"""``cluster_keys`` on a warm context, keys resident in HBM, under the skewed model with its ladder, at key shapes whose
crowded buckets take ``gp_wide_tiles_kernel`` (csrc/group_tiles_wide.hip): the host time of a call (it ends in a
read-back, i.e. a device synchronise) -- ``--warmup`` jobs, then the median and the spread of ``--repeats`` -- the search
stage from the context's stage timer, and the pair-kernel slot of one more job with the kernel timers on. One JSON line
per shape with the route the last job took. One library per process: run it once per build
(``FQD_LIB_VARIANT=name``, tools/ab_variants.sh), alternating, for an A/B.

    python tools/bench_wide_tiles.py [--shapes 10000000x200x2,5000000x600x2] [--warmup 2] [--repeats 5]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fastqdedup_amd as F  # noqa: E402
from fastqdedup_amd.synth import SKEW  # noqa: E402

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="10000000x200x2,5000000x600x2", help="reads x key length x distance")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    for shape in a.shapes.split(","):
        n, L, d = map(int, shape.split("x"))
        ctx = F.Context(0)
        keys = torch.empty(n * L, dtype=torch.uint8, device="cuda:0")
        ctx.synth_keys(keys, n, 0, n, L, 12, 4242, skew=SKEW)
        ctx.set_timing(True, ())
        times, search = [], []
        for job in range(a.warmup + a.repeats):
            t0 = time.perf_counter()
            got = F.cluster_keys(keys, key_len=L, max_distance=d, method="directional", context=ctx)
            if job >= a.warmup:
                times.append(time.perf_counter() - t0)
                search.append(got.stage_ms["edges"])
        ctx.set_timing(True, ("bucket_pairs_kernel",))
        ctx.kernel_times(reset=True)
        F.cluster_keys(keys, key_len=L, max_distance=d, method="directional", context=ctx)
        pairs_ms, pairs_launches = ctx.kernel_times()["bucket_pairs_kernel"]
        print(json.dumps({
            "lib": os.environ.get("FQD_LIB_VARIANT", "this"), "n": n, "L": L, "d": d,
            "n_unique": got.n_unique, "n_edges": got.n_edges, "n_kept": got.n_kept,
            "job_ms": round(statistics.median(times) * 1e3, 2), "job_ms_min_max": [round(min(times) * 1e3, 2), round(max(times) * 1e3, 2)],
            "search_ms": round(statistics.median(search), 2), "search_ms_min_max": [round(min(search), 2), round(max(search), 2)],
            "pair_slot_ms": round(pairs_ms, 2), "pair_slot_launches": pairs_launches,
            "route": sorted(k for k, v in got.route.items() if v)}), flush=True)
        del keys, ctx
