"""Association tests for T phenotypes: vampomi_assoc_loo_multi against T calls
of set_phen + assoc_loo in the same process, per storage, on one GPU.

    python tools/assoc_multi_bench.py [--N 100000] [--M 62500] [--storages f64,f32,u16] [--T 1,2,3,4,8,16]
        [--reps 7] [--out FILE.json]

For each storage the generated methylation-like shard (GEN_METH) is made once;
the phenotypes are simulated on it.  Per T: the median wall time of `reps`
calls of assoc_loo_multi (each ends in a device synchronise) and of `reps`
rounds of the T single calls, after one untimed call of each; then, with
timing on, the device time of the association launches alone (stats.loo) for
both.  The blocks are compared bit for bit with the single calls at every T.
The read ceiling of the same shard (vampomi_dev_read_ceiling) is printed with
them.  One JSON line per (storage, T), one summary line at the end.
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
ap.add_argument("--T", default="1,2,3,4,8,16")
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--out", default="")
a = ap.parse_args()
N, M = a.N, a.M
Ts = [int(t) for t in a.T.split(",")]
ESIZE = {"f64": 8, "f32": 4, "u16": 2}


def median(v):
    return sorted(v)[len(v) // 2]


def timed(fn, reps):
    fn()  # untimed: first launches load code objects
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return median(out), min(out), max(out)


def loo_ms(d, fn):
    """Device time of the association launches of one fn() (every launch timed)."""
    d.set_timing(True, 1)
    d.reset_stats()
    fn()
    s = d.stats()
    d.set_timing(False)
    return s.loo.ms_timed, s.loo.launches, s.ax.ms_timed


res = {"N": N, "M": M, "reps": a.reps, "runs": []}
for storage in a.storages.split(","):
    with va.Data(N, M, storage=storage) as d:
        d.generate(9, va.GEN_METH)
        Y, E = [], []
        rng = np.random.default_rng(1)
        for t in range(max(Ts)):
            beta = d.simulate_phen(10 + t, lam=0.05, h2=0.5)
            Y.append(d.get_phen())
            E.append((beta * 0.9 + rng.normal(size=M) * 1e-3) / np.sqrt(N))
        Y, E = np.stack(Y), np.stack(E)
        ceil = d.read_ceiling()
        print(json.dumps({"storage": storage, "read_ceiling_GBs": round(ceil["GBs"], 1),
                          "read_ceiling_us": round(ceil["us_med"], 1), "kernels": [d.kernel_name(2, k) for k in (1, 2, 3, 4)]}), flush=True)
        for T in Ts:
            Yt, Et = np.ascontiguousarray(Y[:T]), np.ascontiguousarray(E[:T])
            got = {}

            def multi():
                got["m"] = d.assoc_loo_multi(Yt, Et, standardize=False)

            def loop():
                ps = []
                for t in range(T):
                    d.set_phen(Yt[t], standardize=False)
                    ps.append(d.assoc_loo(Et[t])[0])
                got["s"] = np.stack(ps)

            tm, tl = timed(multi, a.reps), timed(loop, a.reps)
            km, kl = loo_ms(d, multi), loo_ms(d, loop)
            run = {"storage": storage, "T": T, "multi_ms": round(tm[0], 3), "multi_min_max": [round(tm[1], 3), round(tm[2], 3)],
                   "loop_ms": round(tl[0], 3), "loop_min_max": [round(tl[1], 3), round(tl[2], 3)],
                   "speedup": round(tl[0] / tm[0], 3), "multi_loo_ms": round(km[0], 3), "multi_loo_launches": km[1],
                   "loop_loo_ms": round(kl[0], 3), "multi_ax_ms": round(km[2], 3), "loop_ax_ms": round(kl[2], 3),
                   "loo_ms_per_phen": round(km[0] / T, 3), "loo_ratio_to_single": round(km[0] / T / (kl[0] / T), 3),
                   "loo_TBs_per_launch": round(ESIZE[storage] * N * M / (km[0] / km[1] * 1e-3) / 1e12, 2),
                   "bitwise": bool(np.array_equal(got["m"][0], got["s"]))}
            res["runs"].append(run)
            print(json.dumps(run), flush=True)
        res.setdefault("ceiling", {})[storage] = ceil
print(json.dumps(res))
if a.out:
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
