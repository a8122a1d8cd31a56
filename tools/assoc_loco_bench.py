"""The leave-one-chromosome-out test against assoc_loo of the same context, in
the same process, per storage, on one GPU.

    python tools/assoc_loco_bench.py [--N 100000] [--M 62500] [--storages f64,f32,u16] [--G 24] [--reps 7]
        [--loop-reps 1] [--out FILE.json]

For each storage the generated methylation-like shard (GEN_METH) is made once
and one phenotype is simulated on it.  Per label layout ("blocks": G
contiguous blocks; "robin": marker j has label j mod G): the median wall time
of `reps` calls of assoc_loco and of assoc_loo (each ends in a device
synchronise), after one untimed call of each; with timing on, the device time
of the two passes of each call (stats.ax, stats.loo: the segmented A.x and the
marker pass against the parent's A.x and loo passes); and the wall time of the
G-call loop that the test replaces (the estimate zeroed inside a label, then
assoc_loo, per label; `loop-reps` rounds).  The marker pass is compared bit for
bit with the marginal test against R[c] for three labels.  The read ceiling of
the same shard (vampomi_dev_read_ceiling) is printed with them.  One JSON line
per (storage, layout), one summary line at the end.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

import vampomi_amd as va  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--N", type=int, default=100000)
ap.add_argument("--M", type=int, default=62500)
ap.add_argument("--storages", default="f64,f32,u16")
ap.add_argument("--G", type=int, default=24)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--loop-reps", type=int, default=1)
ap.add_argument("--out", default="")
a = ap.parse_args()
N, M, G = a.N, a.M, a.G
ESIZE = {"f64": 8, "f32": 4, "u16": 2}


def median(v):
    return sorted(v)[len(v) // 2]


def timed(fn, reps):
    fn()  # untimed: first launches load code objects, first calls allocate workspaces
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return round(median(out), 3), round(min(out), 3), round(max(out), 3)


def pass_ms(d, fn):
    """Device time of the A.x and association launches of one fn() (every launch timed)."""
    d.set_timing(True, 1)
    d.reset_stats()
    fn()
    s = d.stats()
    d.set_timing(False)
    return round(s.ax.ms_timed, 3), round(s.loo.ms_timed, 3), s.a_passes_exec


def layouts():
    blocks = (np.arange(M, dtype=np.int64) * G // M).astype(np.int32)
    robin = (np.arange(M) % G).astype(np.int32)
    return {"blocks": blocks, "robin": robin}


res = {"N": N, "M": M, "G": G, "reps": a.reps, "runs": []}
for storage in a.storages.split(","):
    with va.Data(N, M, storage=storage) as d:
        d.generate(9, va.GEN_METH)
        beta = d.simulate_phen(10, lam=0.05, h2=0.5)
        est = (beta * 0.9 + np.random.default_rng(1).normal(size=M) * 1e-3) / np.sqrt(N)
        ceil = d.read_ceiling()
        print(json.dumps({"storage": storage, "read_ceiling_GBs": round(ceil["GBs"], 1),
                          "read_ceiling_us": round(ceil["us_med"], 1)}), flush=True)
        t_loo = timed(lambda: d.assoc_loo(est), a.reps)
        k_loo = pass_ms(d, lambda: d.assoc_loo(est))
        for name, lab in layouts().items():
            t_loco = timed(lambda: d.assoc_loco(est, lab, G=G), a.reps)
            k_loco = pass_ms(d, lambda: d.assoc_loco(est, lab, G=G))

            def loop():
                for c in range(G):
                    d.assoc_loo(np.where(lab == c, 0.0, est))

            t_loop = timed(loop, a.loop_reps)
            p, st, R = d.assoc_loco(est, lab, G=G, resid=True)
            same = True
            for c in (0, G // 2, G - 1):
                pm, sm = d.assoc_loo_multi(R[c][None], None, standardize=False)
                idx = lab == c
                same = same and bool(np.array_equal(st[idx], sm[0][idx]) and np.array_equal(p[idx], pm[0][idx]))
            gb = ESIZE[storage] * N * M / 1e9
            run = {"storage": storage, "labels": name, "loco_ms": t_loco[0], "loco_min_max": list(t_loco[1:]),
                   "loo_ms": t_loo[0], "loo_min_max": list(t_loo[1:]), "loco_over_loo": round(t_loco[0] / t_loo[0], 3),
                   "loop_ms": t_loop[0], "loop_over_loco": round(t_loop[0] / t_loco[0], 2),
                   "seg_ax_ms": k_loco[0], "ax_ms": k_loo[0], "seg_ax_over_ax": round(k_loco[0] / k_loo[0], 3),
                   "loco_pass_ms": k_loco[1], "loo_pass_ms": k_loo[1],
                   "loco_pass_over_loo_pass": round(k_loco[1] / k_loo[1], 3), "passes": k_loco[2],
                   "seg_ax_TBs": round(gb / k_loco[0], 2), "loco_pass_TBs": round(gb / k_loco[1], 2),
                   "marker_pass_bitwise": same}
            res["runs"].append(run)
            print(json.dumps(run), flush=True)
        res.setdefault("ceiling", {})[storage] = ceil
print(json.dumps(res))
if a.out:
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
