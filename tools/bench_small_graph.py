"""``Context.components()`` + ``Context.dissect()`` of small unique tables on the one-launch route (FQD_GRAPH=small,
the default up to 8 192 keys) and on the wide route (=wide), measured alternately on one warm context per shape: the
host time of the two calls (each ends in a read-back) and the device time ``stage_times()`` reports for them, median
and 10th-90th percentile over ``--repeats`` pairs of calls per route and method. Then 1 000 back-to-back
``cluster_dissection_*`` calls on a 64-key cluster (24 nt, d = 1), five alternating samples per route. Prints one JSON
line per measurement.

    python tools/bench_small_graph.py [--repeats 120] [--shapes 1000x32x1,8000x32x1,8000x300x2] [--calls 1000]"""
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

METHODS = ("highest_count", "adjacency", "directional")


def timed(ctx, route, method, calls):
    """[(host seconds, device ms)] of `calls` runs of components + dissect."""
    os.environ["FQD_GRAPH"] = route
    out = []
    for _ in range(calls):
        t0 = time.perf_counter()
        ctx.components()
        ctx.dissect(F.core.METHODS[method])
        host = time.perf_counter() - t0
        ms = ctx.stage_times()[0]
        out.append((host, ms["components"] + ms["dissect"]))
    return out


def summary(values, scale, digits):
    return [round(statistics.median(values) * scale, digits)] + [round(float(q) * scale, digits) for q in np.percentile(values, [10, 90])]


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=120)
    ap.add_argument("--shapes", default="1000x32x1,8000x32x1,8000x300x2")
    ap.add_argument("--calls", type=int, default=1000)
    a = ap.parse_args()
    for shape in a.shapes.split(","):
        n, L, d = map(int, shape.split("x"))
        # (copies = 1: about as many unique keys as reads; a substitution rate that leaves edges)
        keys = synth_keys(n, L, 12, 21, copies=1, sub_rate=5e-3)
        ctx = F.Context(0)
        ctx.set_timing(True, ())
        ctx.pack_keys(np.ascontiguousarray(keys).reshape(-1), None, L)
        n_unique = ctx.collapse()
        n_edges = ctx.find_edges(d)
        for method in METHODS:
            row = {"U": n_unique, "L": L, "d": d, "edges": n_edges, "method": method}
            kept = {}
            for route in ("small", "wide"):              # warm-up: code objects, buffers
                timed(ctx, route, method, 5)
                kept[route] = ctx.unique_table(n_unique)[3].tobytes()
                row[route + "_took_small"] = ctx.route()["graph_small"]
            assert kept["small"] == kept["wide"]
            times = {"small": [], "wide": []}
            for _ in range(6):                           # alternating blocks
                for route in times:
                    times[route] += timed(ctx, route, method, max(1, a.repeats // 6))
            for route, t in times.items():
                row[route + "_host_us"] = summary([h for h, _ in t], 1e6, 1)
                row[route + "_device_us"] = summary([m for _, m in t], 1e3, 1)
            print(json.dumps(row), flush=True)
    rng = np.random.default_rng(7)
    stem = rng.choice(list("ACGT"), size=24)
    cluster = []
    for i in range(64):                                  # a molecule and its one-substitution variants, 24 nt
        s = stem.copy()
        if i:
            s[rng.integers(24)] = rng.choice(list("ACGT"))
        cluster.append((int(rng.integers(1, 9)) if i else 40, "".join(s)))
    for name in ("cluster_dissection_directional", "cluster_dissection_adjacency"):
        fn = getattr(F, name)
        samples = {"small": [], "wide": []}
        for route in samples:
            os.environ["FQD_GRAPH"] = route
            list(fn(cluster, 1))
        for _ in range(5):
            for route in samples:
                os.environ["FQD_GRAPH"] = route
                t0 = time.perf_counter()
                for _ in range(a.calls):
                    list(fn(cluster, 1))
                samples[route].append(time.perf_counter() - t0)
        print(json.dumps({"call": name, "calls": a.calls, "items": len(cluster),
                          **{r + "_s": [round(statistics.median(t), 4), round(min(t), 4), round(max(t), 4)]
                             for r, t in samples.items()}}), flush=True)
    os.environ.pop("FQD_GRAPH", None)
