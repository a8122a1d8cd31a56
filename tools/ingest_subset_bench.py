"""Streaming ingest rate with a row subset (vampomi_set_row_subset), next to the
plain load of tools/ingest_bench.py: one marker-major fp64 file of the given
shape, loaded `reps` times plainly and `reps` times at each keep fraction
(every k-th row spread evenly, rows 0 and N - 1 kept), each load checked bit for
bit against the plain one's rows.  Rates are the FILE's bytes per second: a
subset load reads and stages all of them.

    python tools/ingest_subset_bench.py [--N 100000] [--M 25000] [--path F] [--threads 8] [--reps 3]
        [--keep 1.0,0.9,0.5] [--plain-only] [--reuse] [--leave]

--plain-only: no subset loads (a library without the entry point, named by
VAMPOMI_LIB, for a comparison of the plain path); --reuse: load the file at
--path as it is instead of writing it; --leave: do not remove it.
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
ap.add_argument("--path", default=os.path.join(os.environ.get("TMPDIR", "/tmp"), "vampomi_ingest_subset.bin"))
ap.add_argument("--threads", type=int, default=8)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--keep", default="1.0,0.9,0.5")
ap.add_argument("--plain-only", action="store_true")
ap.add_argument("--reuse", action="store_true")
ap.add_argument("--leave", action="store_true")
a = ap.parse_args()
N, M = a.N, a.M
gb = 8.0 * N * M / 1e9
os.environ["VAMPOMI_IO_THREADS"] = str(a.threads)
res = {"N": N, "M": M, "GB": round(gb, 2), "threads": a.threads, "runs": []}
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
ref = None


def one(kind, keep, rows):
    global ref
    with va.Data(N, M, **({} if rows is None else {"rows": rows})) as d:
        t0 = time.perf_counter()
        d.read_methylation_data(a.path)
        el = time.perf_counter() - t0
        got = np.concatenate([d.get_meth_data(i, 1) for i in probe])
        mave = d.get_mave()
    if rows is None:
        if ref is None:
            ref = got
        ok = bool(np.array_equal(got, ref))
    else:
        ok = bool(np.array_equal(got, ref[:, rows]))
        if len(rows) == N:
            ok = ok and bool(np.array_equal(mave, ref_mave))
    run = {"load": kind, "keep": keep, "n": N if rows is None else len(rows), "s": round(el, 3),
           "GB/s": round(gb / el, 2), "bitwise": ok}
    res["runs"].append(run)
    print(json.dumps(run), flush=True)
    return mave


ref_mave = None
for _ in range(a.reps):
    ref_mave = one("plain", None, None)
if not a.plain_only:
    for frac in [float(x) for x in a.keep.split(",")]:
        n = max(2, min(N, int(round(frac * N))))
        rows = np.unique(np.round(np.linspace(0, N - 1, n)).astype(np.int64))
        for _ in range(a.reps):
            one("subset", frac, rows)
if not a.leave:
    os.remove(a.path)
for kind, keep in sorted({(r["load"], r["keep"]) for r in res["runs"]}, key=lambda t: (t[0], -(t[1] or 2))):
    v = [r["GB/s"] for r in res["runs"] if (r["load"], r["keep"]) == (kind, keep)]
    res.setdefault("summary", []).append({"load": kind, "keep": keep, "GB/s": v, "median": sorted(v)[len(v) // 2],
                                          "spread": round(max(v) - min(v), 2)})
print(json.dumps(res))
