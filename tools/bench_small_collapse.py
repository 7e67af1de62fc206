"""``Context.collapse()`` of small inputs on the LDS-table route (FQD_COLLAPSE=small, the default under 65 536 reads)
and on the sort path (=sort),
measured alternately on one warm context: the median host time of a call (it ends in the read-back, i.e. a device
synchronise) over ``--repeats`` calls per route, then the launches ``kernel_times()`` saw in one call per route.
Shapes: n reads of L nt, once duplicate-heavy (``synth_keys`` with a 6-nt UMI) and once all distinct. Prints one JSON
line per shape.

    python tools/bench_small_collapse.py [--repeats 300] [--shapes 1000x32,16000x32,60000x32,16000x300]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fastqdedup_amd as F  # noqa: E402
from fastqdedup_amd.synth import synth_keys  # noqa: E402


def pin(route):
    os.environ["FQD_COLLAPSE"] = route


def timed(ctx, route, calls):
    pin(route)
    out = []
    for _ in range(calls):
        t0 = time.perf_counter()
        ctx.collapse()
        out.append(time.perf_counter() - t0)
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=300)
    ap.add_argument("--shapes", default="1000x32,16000x32,60000x32,16000x300")
    a = ap.parse_args()
    rng = np.random.default_rng(7)
    for shape in a.shapes.split(","):
        n, L = map(int, shape.split("x"))
        for kind in ("duplicates", "distinct"):
            keys = synth_keys(n, L, 6, 21, copies=8) if kind == "duplicates" else \
                rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=(n, L))
            ctx = F.Context(0)
            ctx.set_timing(False, ())
            ctx.pack_keys(np.ascontiguousarray(keys).reshape(-1), None, L)
            row = {"n": n, "L": L, "reads": kind}
            unique = {}
            for route in ("small", "sort"):              # warm-up: code objects, buffers
                unique[route] = timed(ctx, route, 5) and ctx.collapse()
            assert unique["small"] == unique["sort"]
            row["n_unique"] = unique["small"]
            times = {"small": [], "sort": []}
            for _ in range(6):                           # alternating blocks
                for route in times:
                    times[route] += timed(ctx, route, a.repeats // 6)
            for route, t in times.items():
                row[route + "_us"] = round(statistics.median(t) * 1e6, 1)
                row[route + "_us_p10_p90"] = [round(float(q) * 1e6, 1) for q in np.percentile(t, [10, 90])]
            ctx.set_timing(False, None)
            for route in times:
                ctx.kernel_times(reset=True)
                timed(ctx, route, 1)
                row[route + "_timed_launches"] = {k: v[1] for k, v in ctx.kernel_times().items() if v[1]}
            print(json.dumps(row), flush=True)
    os.environ.pop("FQD_COLLAPSE", None)
