"""What the CPU oracle alone does with degenerate markers (tests/_degenerate.py),
so that tests/test_gpu_degenerate.py has a sound reference; no GPU.

* Dyadic constant columns: msig == 1, mave == c, (A^T u)_m == 0 and x1_hat_m == 0
  at every iteration, exactly, for the linear and the probit model; the LOO
  p-value is NaN there (s2x = 0) and finite everywhere else.
* Non-dyadic constants (0.3, 0.7) are NOT defined by the reference: the
  sequential sum puts the mean an ulp off c, msig becomes ~1e14 and the column a
  constant +-sqrt((N-1)/N) whose sign is an accident of rounding; a run moves by
  far more than rounding against the same matrix with those columns at 0.25.
  This is why the GPU tests ask for no parity there.
* The Student-t tail at |t| = inf and where t * t overflows.
"""
import math

import numpy as np
import pytest

import _degenerate as D
from oracle import pyoracle as O

N0, MT0 = 301, 517


def _rel(a, b):
    return np.linalg.norm(a - b) / np.linalg.norm(b)


@pytest.fixture(scope="module")
def prob():
    X, idx = D.planted(N0, MT0)
    return X, idx, O.marker_stats(X)


def test_planted_layout():
    for N, Mt in ((301, 517), (4099, 333), (12001, 300), (20001, 160)):
        X, idx = D.planted(N, Mt, nondyadic=True)
        c = idx["const"]
        assert X.shape == (Mt, N) and X.min() >= 0 and X.max() <= 1
        assert c[0] == 0 and c[-1] == Mt - 1 and {4, 7, 16, 23, 28, 35} <= set(c.tolist())
        assert ({64, 127} <= set(c.tolist())) == (N >= D.TEAM_N)
        assert np.array_equal(X[c], np.broadcast_to(idx["const_val"][:, None], (len(c), N)))
        assert set(idx["const_val"].tolist()) == set(D.DYADIC)
        for m, r, v in zip(idx["single"], idx["single_row"], idx["single_val"]):
            assert X[m, r] == v and np.count_nonzero(X[m]) == 1
        assert sorted(idx["single_row"].tolist()) == [0, 1, 127, 128, N - 1]
        d = idx["dup"]
        assert np.array_equal(X[d[0]], X[d[1]]) and np.array_equal(X[d[0]], X[d[2]]) and np.ptp(X[d[0]]) > 0
        assert len({int(m) % 8 for m in d}) == 3 and d[2] >= (Mt - 1) // 8 * 8
        assert np.array_equal(X[idx["nondyadic"]][:, 0], D.NONDYADIC)
        g = O.generate_markers(3, 1, N, 0, Mt)
        assert np.array_equal(X[idx["plain"]], g[idx["plain"]])
        assert sum(len(idx[k]) for k in ("const", "single", "dup", "nondyadic", "plain")) == Mt


@pytest.mark.parametrize("alpha", [1.0, 0.7])
def test_oracle_statistics_of_dyadic_constants(alpha):
    X, idx = D.planted(N0, MT0)
    mave, msig = O.marker_stats(X, alpha)
    c = idx["const"]
    assert np.array_equal(mave[c], idx["const_val"]) and np.all(msig[c] == 1.0)
    d = idx["dup"]
    assert mave[d[0]] == mave[d[1]] == mave[d[2]] and msig[d[0]] == msig[d[1]] == msig[d[2]]
    rest = np.setdiff1d(np.arange(MT0), c)
    assert np.all(msig[rest] != 1.0) and np.all(np.isfinite(msig))
    s = idx["single"][4]  # the 2^-30 entry: 1 / msig^2 = 2^-60 / N
    if alpha == 1.0:
        assert abs(msig[s] / (2.0 ** 30 * math.sqrt(N0)) - 1) < 1e-14


def test_oracle_operators_at_dyadic_constants(prob):
    X, idx, (mave, msig) = prob
    rng = np.random.default_rng(1)
    u, x = rng.normal(size=N0), rng.normal(size=MT0)
    c = idx["const"]
    assert np.all(O.atx(X, mave, msig, u)[c] == 0.0)
    x2 = x.copy()
    x2[c] *= 1e30
    assert np.array_equal(O.ax(X, mave, msig, x), O.ax(X, mave, msig, x2))
    t = O.atx(X, mave, msig, u)[idx["dup"]]
    assert t[0] == t[1] == t[2]


@pytest.mark.parametrize("model,its", [("linear", 8), ("bin_class", 4)])
def test_oracle_run_keeps_constants_at_zero(prob, model, its):
    X, idx, _ = prob
    y, beta = D.phen(X, binary=model == "bin_class")
    ref = O.vamp_infere(X, y, MT0, true_signal=beta, max_iter=its, stop_criteria_thr=0.0, model=model)
    assert ref["iterations"] == its
    assert np.all(ref["x1_hist"][:, idx["const"]] == 0.0)
    assert np.all(np.isfinite(ref["x1_hist"])) and np.any(ref["x1_hist"][-1] != 0.0)


def test_oracle_loo_is_nan_exactly_at_the_constants(prob):
    X, idx, _ = prob
    y, beta = D.phen(X)
    po, sto = O.assoc_loo(X, y, beta * 0.9 / math.sqrt(N0))
    mask = np.zeros(MT0, dtype=bool)
    mask[idx["const"]] = True
    assert np.array_equal(np.isnan(po), mask)
    assert np.all(np.isfinite(sto)) and np.all((po[~mask] >= 0) & (po[~mask] <= 1))
    d = idx["dup"]
    assert np.array_equal(sto[d[0]], sto[d[1]]) and np.array_equal(sto[d[0]], sto[d[2]]) and po[d[0]] == po[d[2]]


@pytest.mark.parametrize("N", [301, 1000, 4099])
def test_oracle_nondyadic_constants_are_not_constant_to_it(N):
    for c in D.NONDYADIC:
        mave, msig = O.marker_stats(np.full((1, N), c))
        e = (c - mave[0]) * msig[0]
        print(f"N={N} c={c}: mave - c = {mave[0] - c:.3e}, msig = {msig[0]:.3e}, e = {e:+.6f}")
        assert msig[0] != 1.0 and msig[0] > 1e12
        assert abs(abs(e) - math.sqrt((N - 1) / N)) <= N * 2.0 ** -53 * abs(e)


@pytest.mark.parametrize("N,Mt", [(301, 517), (1000, 333)])
def test_oracle_run_moves_with_nondyadic_constants(N, Mt):
    """The oracle's 8-iteration run with columns of 0.3 and 0.7 against the same
    matrix with those columns at 0.25: measured 6e-5 to 9e-3 norm-relative in
    x1_hat (a rounding-level change would be ~1e-13)."""
    X, idx = D.planted(N, Mt, nondyadic=True)
    y, beta = D.phen(D.planted(N, Mt)[0])  # one phenotype for both runs
    kw = dict(true_signal=beta, max_iter=8, stop_criteria_thr=0.0)
    a = O.vamp_infere(X, y, Mt, **kw)
    X2 = X.copy()
    X2[idx["nondyadic"]] = 0.25
    b = O.vamp_infere(X2, y, Mt, **kw)
    assert np.all(b["x1_hist"][:, idx["nondyadic"]] == 0.0)
    gap = max(_rel(a["x1_hist"][k], b["x1_hist"][k]) for k in range(1, 8))
    print(f"N={N} Mt={Mt}: x1_hat moves by {gap:.3e}; cg {a['cg_iters'].tolist()} vs {b['cg_iters'].tolist()}")
    assert gap > 1e-6


T_BELOW, T_ABOVE = (1e150, 1.3e154), (1.4e154, 1e160, 1e300)


@pytest.mark.parametrize("df", [1, 2, 3, 30, 299])
def test_t_tail_at_infinite_and_overflowing_t(df):
    """0.5 * I_x(df/2, 1/2), x = df / (df + t^2), in mpmath: to 1e-9 while t * t is
    finite (tests/test_mixture_refs.py's agreement); from where it overflows,
    0 <= p <= the true value (Boost's complemented cdf returns 0 there, its
    z = df / (df + inf) being 0); at inf exactly 0, both tails finite."""
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 60

    def ref(t):
        x = mp.mpf(df) / (mp.mpf(df) + mp.mpf(t) ** 2)
        return float(mp.betainc(mp.mpf(df) / 2, mp.mpf(1) / 2, 0, x, regularized=True) / 2)

    for t in T_BELOW:
        assert math.isfinite(t * t)
        got, want = O.t_sf(t, df), ref(t)
        assert abs(got - want) <= 1e-9 * want, (df, t, got, want)
        assert O.t_sf(-t, df) == 1.0 - got
    for t in T_ABOVE:
        assert math.isinf(t * t)
        got, want = O.t_sf(t, df), ref(t)
        assert 0.0 <= got <= want * (1 + 1e-9), (df, t, got, want)
        assert O.t_sf(-t, df) == 1.0 - got
    assert O.t_sf(math.inf, df) == 0.0 and O.t_sf(-math.inf, df) == 1.0
    assert math.isnan(O.t_sf(math.nan, df))


@pytest.mark.parametrize("N", [64, 301, 4099])
def test_oracle_p_is_zero_where_y_is_a_column(N):
    """y_mark = +-X[m] (est = 0): rxy = +-1 exactly, t = inf, p = 0."""
    X = O.generate_markers(3, 1, N, 0, 40)
    for m, sign in ((7, 1.0), (33, -1.0)):
        po, _ = O.assoc_loo(X, sign * X[m], np.zeros(40))
        assert po[m] == 0.0
        assert np.all(np.isfinite(po)) and np.all(np.delete(po, m) > 0)
