"""The planted problem of the degenerate-marker tests: a methylation-like
matrix (values in [0, 1], so it loads into every storage) whose columns at the
places where the kernels' structure changes are constant, all but constant, or
copies of one another.

A constant column is what compute_markers_statistics (src/data.cpp:233-283)
gives msig = 1 for, when the centred sum of squares is exactly 0; every operator
then relies on (x - mave) being an exact zero.  For a DYADIC constant (a
multiple of 2^-16 here) every sum of the column is exact in fp64 at these N, so
the reference's answers are exact and independent of the summation order:
mave = c, msig = 1, (A^T u)_m = 0, x1_hat_m = 0.  A non-dyadic constant (0.3,
0.7) is not defined in the reference itself: its mean is an ulp
off c in a direction that depends on the order of the sum.
"""
import numpy as np

from oracle import pyoracle as O

DYADIC = (0.0, 1.0, 0.5, 0.25, 65535 / 65536)
NONDYADIC = (0.3, 0.7)
TINY = 2.0 ** -30
TEAM_N = 12000  # from here on the one-pass operator runs on teams (tests/test_gpu_tiny.py)


def planted(N, Mt, seed=3, nondyadic=False, team=None):
    """(X (Mt, N), idx): O.generate_markers(seed, 1, N, 0, Mt) with planted columns.

    idx maps each class to its column indices (ascending int64 arrays):
      "const"      dyadic constants, values idx["const_val"] cycling DYADIC: column
                   0; column Mt - 1 (the one out-of-range lanes are clamped to);
                   4-8 (a stats_kernel block); 16-24 (the widest G of atx_kernel
                   and loo_kernel); 28-36 (across an 8-boundary); with `team`
                   (default: N >= TEAM_N) also 64-128, at least two per team
                   member at T = 32 with interleaved teams
      "single"     all 0 but one entry (idx["single_row"], idx["single_val"]): 1.0
                   at row 0, 127, 128 (the lane stride) and N - 1 (next to the pad
                   row of an odd N), 2^-30 at row 1 (msig ~ 1e9 sqrt(N))
      "dup"        three equal columns: one generator column at 50, copied to 61
                   (another position of another 8-group) and into the last,
                   partly filled 8-group
      "nondyadic"  with nondyadic=True, 0.3 at 45 and 0.7 at 46 (f64 storage only)
      "plain"      everything else, as generated
    """
    if team is None:
        team = N >= TEAM_N
    assert N > 129 and Mt >= (138 if team else 74), (N, Mt)
    X = O.generate_markers(seed, 1, N, 0, Mt)
    const = [0, Mt - 1] + list(range(4, 8)) + list(range(16, 24)) + list(range(28, 36))
    if team:
        const += list(range(64, 128))
    const = np.array(sorted(const), dtype=np.int64)
    cval = np.array([DYADIC[i % len(DYADIC)] for i in range(len(const))])
    X[const] = cval[:, None]

    single = np.arange(40, 45, dtype=np.int64)
    srow = np.array([0, 127, 128, N - 1, 1], dtype=np.int64)
    sval = np.array([1.0, 1.0, 1.0, 1.0, TINY])
    X[single] = 0.0
    X[single, srow] = sval

    last = (Mt - 1) // 8 * 8 + 1  # position 1 of the last 8-group (Mt - 1 itself is a constant)
    assert (128 if team else 62) <= last < Mt - 1, (Mt, last)
    dup = np.array([50, 61, last], dtype=np.int64)
    X[dup[1:]] = X[dup[0]]

    nd = np.array([45, 46], dtype=np.int64) if nondyadic else np.zeros(0, dtype=np.int64)
    if nondyadic:
        X[nd] = np.array(NONDYADIC)[:, None]

    used = np.concatenate([const, single, dup, nd])
    assert len(np.unique(used)) == len(used)
    idx = {"const": const, "const_val": cval, "single": single, "single_row": srow, "single_val": sval,
           "dup": dup, "nondyadic": nd, "nondyadic_val": np.array(NONDYADIC[:len(nd)]),
           "plain": np.setdiff1d(np.arange(Mt, dtype=np.int64), used)}
    return X, idx


def phen(X, seed=3, binary=False):
    """(y, beta): a standardised (or, thresholded, 0/1) phenotype from fixed-order
    arithmetic (tests/_data.py: phen_from_markers); an effect drawn on a constant
    column adds nothing to it."""
    from _data import phen_from_markers

    y, beta = phen_from_markers(X, seed)
    return ((y > 0).astype(np.float64) if binary else y), beta


def nan_aware_pfun(p, st, N):
    """tests/test_gpu_assoc.py's _check_pfun where the oracle's p-value function
    of the device's own sums is finite, and NaN exactly where it is NaN."""
    pf = np.array([O.reg1d_pval(*s, N) for s in st])
    assert np.array_equal(np.isnan(p), np.isnan(pf)), (np.nonzero(np.isnan(p) != np.isnan(pf))[0][:8])
    ok = ~np.isnan(pf)
    assert np.all(np.abs(p[ok] - pf[ok]) <= 1e-12 * pf[ok] + 1e-300)
