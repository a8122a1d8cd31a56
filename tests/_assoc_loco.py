"""Helpers of tests/test_gpu_assoc_loco.py and tests/test_assoc_loco.py: the
shapes and label sets of the leave-one-chromosome-out tests, the oracle's
references (made once per case and left unchanged), and the bars, which are
those of tests/_assoc_multi.py."""
import numpy as np

import _assoc_multi as H
from oracle import pyoracle as O

# (N, Mt, generator kind): the two shapes of the single-phenotype tests, and
# one whose N = 1101 spans three row tiles of the segmented A.x (512 rows; the
# last tile ragged, N odd) and whose 700 markers give a label more than one
# chunk of 256 columns under the "g1" and "blocks" label sets
SHAPES = [(301, 257, 0), (1001, 517, 1), (1101, 700, 1)]
STORAGES = {SHAPES[0]: ("f64", "f32"), SHAPES[1]: ("f64", "f32", "u16"), SHAPES[2]: ("f64", "u16")}
LABELSETS = ("g5", "blocks", "g1", "g64")


def labels(name, Mt):
    """(labels int32 (Mt), G)."""
    if name == "g5":
        # label 2 unused, label 1 one marker, the first 7 markers label 0, the
        # rest spread at random over labels 0, 3 and 4 (not contiguous)
        rng = np.random.default_rng(5)
        lab = rng.choice(np.array([0, 3, 4]), size=Mt)
        lab[:7] = 0
        lab[Mt // 2] = 1
        return lab.astype(np.int32), 5
    if name == "blocks":  # three contiguous blocks of about 1/2, 1/3 and 1/6
        lab = np.zeros(Mt, dtype=np.int32)
        lab[Mt // 2:] = 1
        lab[Mt // 2 + Mt // 3:] = 2
        return lab, 3
    if name == "g1":
        return np.zeros(Mt, dtype=np.int32), 1
    if name == "g64":  # round robin, rotated so that label 0 does not start the file
        return ((np.arange(Mt) + 11) % 64).astype(np.int32), 64
    raise KeyError(name)


def problem(N, Mt, kind):
    """X (Mt, N), y (N) standardised, est (Mt): tests/_assoc_multi.py's first phenotype."""
    X, Y, E = H.problem(N, Mt, kind, T=1)
    return X, Y[0], E[0]


def zeroed(est, lab, c):
    e = est.copy()
    e[lab == c] = 0.0
    return e


def oracle_refs(X, y, est, lab, G):
    """What the oracle says about the test on the matrix X (as stored) and the
    phenotype y (as the context holds it): per label c the residual
    y - A (x1 zeroed inside c), the p-values and sums of assoc_loo with that
    estimate and their order spread, all taken at the markers of c; and
    scale = ||y|| + sum_c ||z_c||, the residual bar's norm."""
    Mt, N = X.shape
    mave, msig = O.marker_stats(X)
    x1 = est * np.sqrt(N)
    R = np.zeros((G, N))
    p, st, spread = np.zeros(Mt), np.zeros((Mt, 5)), np.zeros(Mt)
    scale = np.linalg.norm(y)
    for c in range(G):
        idx = lab == c
        R[c] = y - O.ax(X, mave, msig, zeroed(x1, lab, c))
        scale += np.linalg.norm(O.ax(X, mave, msig, np.where(idx, x1, 0.0)))
        if idx.any():
            ez = zeroed(est, lab, c)
            po, sto = O.assoc_loo(X, y, ez)
            p[idx], st[idx] = po[idx], sto[idx]
            spread[idx] = H.order_spread(X, y, ez, po)[idx]
    return {"R": R, "p": p, "st": st, "spread": spread, "scale": scale}


def check_resid(R, ref, scale, what=""):
    """||R[c] - ref_c||_2 <= 1e-12 (||y||_2 + sum ||z_c||_2): ten times the
    1e-13 bar of an A.x, for the G + 1 products in y_c.  Returns the largest
    ratio seen."""
    worst = 0.0
    for c in range(len(ref)):
        err = np.linalg.norm(R[c] - ref[c]) / scale
        worst = max(worst, err)
        assert err <= 1e-12, (what, c, err)
    return worst


def check_against_oracle(p, st, ref, N, centred=None):
    """The bars of tests/_assoc_multi.py: sums 1e-13, p-value function 1e-12,
    p-values 1e-10 or 10x the order spread of the zeroed estimate.

    centred (an adjusted context only): {0: sum |X_j| per marker, 3: sum |y_c|
    per marker}.  The adjustment projects the intercept out of every column and
    of y, so sum X and sum y are zero in exact arithmetic and what any
    summation order returns for them is its own rounding noise (about 1e-15
    here): the oracle's two orders differ from each other by more than 1e-13
    of such a sum.  check_loo's bar on these two sums is then taken against the
    norm of the summed magnitudes, which is the same number wherever the terms
    do not cancel (every plain context: X >= 0); the other three sums, the
    p-value function and the p-values keep check_loo's bars as they are."""
    H.check_pfun(p, st, N)
    if centred is None:
        H.check_loo(p, st, ref["p"], ref["st"], ref["spread"])
        return
    for q in range(5):
        den = np.linalg.norm(centred[q]) if q in centred else np.linalg.norm(ref["st"][:, q])
        assert np.linalg.norm(st[:, q] - ref["st"][:, q]) < 1e-13 * den, q
    tol = np.maximum(1e-10, 10 * ref["spread"])
    ok = np.abs(p - ref["p"]) <= tol * ref["p"] + 1e-300
    assert ok.all(), (p[~ok][:5], ref["p"][~ok][:5], ref["spread"][~ok][:5])


def differs(p, q):
    """at least one marker's p-value differs by more than 1e-3 relative"""
    return bool(np.any(np.abs(p - q) > 1e-3 * np.abs(q)))
