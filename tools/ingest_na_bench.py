"""Streaming ingest rate under the NaN policies (vampomi_set_meth_na), next to
the plain load of tools/ingest_bench.py: one marker-major fp64 file of the given
shape, loaded `reps` times under pass and under fatal, then, after `frac` of
every marker's entries have been overwritten with NaN in place (random rows,
fixed seed), `reps` times under mean.  Rates are the FILE's bytes per second of
wall clock around read_methylation_data (ingest and marker statistics).

    python tools/ingest_na_bench.py [--N 100000] [--M 25000] [--path F] [--threads 8] [--reps 3]
        [--frac 0.005] [--policies pass,fatal,mean] [--reuse] [--leave]

--policies: which loads to run, in that order (pass alone for a library without
the entry points, named by VAMPOMI_LIB); --reuse: load the file at --path as it
is instead of writing it (and plant nothing: a file left by an earlier run with
mean already holds its NaNs); --leave: do not remove it.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402,F401

import vampomi_amd as va  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--N", type=int, default=100000)
ap.add_argument("--M", type=int, default=25000)
ap.add_argument("--path", default=os.path.join(os.environ.get("TMPDIR", "/tmp"), "vampomi_ingest_na.bin"))
ap.add_argument("--threads", type=int, default=8)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--frac", type=float, default=0.005)
ap.add_argument("--policies", default="pass,fatal,mean")
ap.add_argument("--reuse", action="store_true")
ap.add_argument("--leave", action="store_true")
a = ap.parse_args()
N, M = a.N, a.M
gb = 8.0 * N * M / 1e9
os.environ["VAMPOMI_IO_THREADS"] = str(a.threads)
res = {"N": N, "M": M, "GB": round(gb, 2), "threads": a.threads, "frac": a.frac, "runs": []}
if not a.reuse:
    t0 = time.perf_counter()
    with va.Data(N, M) as d:
        d.generate(5, va.GEN_METH)
        with open(a.path, "wb") as f:
            step = max(1, (1 << 30) // (8 * N))
            for i0 in range(0, M, step):
                f.write(d.get_meth_data(i0, min(step, M - i0)).astype("<f8").tobytes())
    res["write_s"] = round(time.perf_counter() - t0, 1)
probe = sorted({0, M // 2, M - 1})  # the markers whose rows are compared
per = max(1, int(round(a.frac * N)))  # NaNs per marker
planted = 0


def plant():
    """`per` distinct random rows of every marker become NaN, in place."""
    global planted
    t0 = time.perf_counter()
    rng = np.random.default_rng(9)
    mm = np.memmap(a.path, dtype="<f8", mode="r+", shape=(M, N))
    step = max(1, (1 << 28) // (8 * N))
    for i0 in range(0, M, step):
        nc = min(step, M - i0)
        rows = np.stack([rng.choice(N, per, replace=False) for _ in range(nc)])
        mm[i0 + np.arange(nc)[:, None], rows] = np.nan
    del mm  # (no flush: the loads read the page cache, which already holds the new bytes)
    planted = per * M
    res["plant_s"] = round(time.perf_counter() - t0, 1)
    res["planted"] = planted


def one(policy):
    kw = {} if policy == "pass" else {"meth_na": policy}
    with va.Data(N, M, **kw) as d:
        t0 = time.perf_counter()
        d.read_methylation_data(a.path)
        el = time.perf_counter() - t0
        got = np.concatenate([d.get_meth_data(i, 1) for i in probe])
        stats = d.missing_stats() if hasattr(d, "missing_stats") and policy != "pass" else None
    run = {"load": policy, "s": round(el, 3), "GB/s": round(gb / el, 2)}
    if policy == "mean":  # filled: no NaN left, the counts are the planted ones
        run["missing"] = stats["missing"]
        run["ok"] = bool(not np.isnan(got).any() and stats["missing"] == (planted or stats["missing"]) and
                         stats["markers_masked"] == 0)
    elif policy == "fatal":  # a clean file: stored as the plain load stores it (after a pass load)
        run["ok"] = bool(stats["missing"] == 0 and (ref is None or np.array_equal(got, ref)))
    res["runs"].append(run)
    print(json.dumps(run), flush=True)
    return got


ref = None
policies = a.policies.split(",")
for policy in policies:
    if policy == "mean" and not a.reuse:
        plant()
    for _ in range(a.reps):
        got = one(policy)
        if policy == "pass" and ref is None:
            ref = got
if not a.leave:
    os.remove(a.path)
for policy in policies:
    v = [r["GB/s"] for r in res["runs"] if r["load"] == policy]
    res.setdefault("summary", []).append({"load": policy, "GB/s": v, "median": sorted(v)[len(v) // 2],
                                          "spread": round(max(v) - min(v), 2)})
print(json.dumps(res))
