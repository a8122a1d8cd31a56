#!/usr/bin/env python3
"""What storing X on a coarser grid costs the algorithm, on the CPU oracle.

    python tools/quant_cost.py [--N 301] [--Mt 500] [--its 8] [--seed 11]

Runs oracle.pyoracle.vamp_infere on the methylation-like generator's matrix and
on the same matrix as a narrow storage holds it (u16: k * 2^-16 with
k = min(65535, rint(x * 65536)); f32: rounded to float), and prints: the share
of entries changed, the largest change, the norm-relative move of x1_hat per
iteration, and whether every CG / Onsager count is identical.  No device.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import pyoracle as O  # noqa: E402


def stored(X, storage):
    if storage == "u16":
        return np.minimum(65535, np.rint(X * 65536)) / 65536
    return X.astype(np.float32).astype(np.float64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=301)
    ap.add_argument("--Mt", type=int, default=500)
    ap.add_argument("--its", type=int, default=8)
    ap.add_argument("--seed", type=int, default=11)
    a = ap.parse_args()
    X = O.generate_markers(a.seed, 1, a.N, 0, a.Mt)
    rng = np.random.default_rng(a.seed)
    beta = np.zeros(a.Mt)
    idx = rng.choice(a.Mt, 50, replace=False)
    beta[idx] = rng.normal(0, np.sqrt(0.8 / 50), 50)
    y = O.standardize_phen(X.T @ beta + rng.normal(0, np.sqrt(0.2), a.N))
    ref = O.vamp_infere(X, y, a.Mt, true_signal=beta, max_iter=a.its, stop_criteria_thr=0.0)
    print(f"methylation-like generator, N = {a.N}, Mt = {a.Mt}, {ref['iterations']} iterations")
    for storage in ("f32", "u16"):
        W = stored(X, storage)
        r = O.vamp_infere(W, y, a.Mt, true_signal=beta, max_iter=a.its, stop_criteria_thr=0.0)
        moves = [np.linalg.norm(r["x1_hist"][k] - ref["x1_hist"][k]) / max(np.linalg.norm(ref["x1_hist"][k]), 1e-300)
                 for k in range(min(r["iterations"], ref["iterations"]))]  # (an all-zero first estimate: 0)
        same = (r["iterations"] == ref["iterations"] and r["cg_iters"].tolist() == ref["cg_iters"].tolist()
                and r["ons_iters"].tolist() == ref["ons_iters"].tolist())
        print(f"{storage}: entries changed {np.mean(W != X):.4f}, max abs change {np.abs(W - X).max():.3e}, "
              f"clamped {int(np.count_nonzero(np.rint(X * 65536) > 65535)) if storage == 'u16' else 0}")
        print("     x1_hat move per iteration: " + " ".join(f"{m:.2e}" for m in moves))
        print(f"     CG / Onsager counts identical: {same}  (cg {r['cg_iters'].tolist()} vs {ref['cg_iters'].tolist()}; "
              f"onsager {r['ons_iters'].tolist()} vs {ref['ons_iters'].tolist()})")


if __name__ == "__main__":
    main()
