"""The references of the large-mixture and element-wise GPU tests, checked on
the CPU before a GPU is involved (tests/_mix.py holds them):

* the oracle's g1 / g1d against the spike-and-slab posterior in mpmath over
  the whole (L, gam1) grid of tests/test_gpu_mixture.py, at 4x the measured
  worst cases |g - ref| <= 1.3e-14 |r| and |gd - ref| <= 1.3e-12 (both at
  gam1 = 1e-6).  The relative error of g itself reaches 1e-8 where the spike
  dominates (the formula's cancellation y + sigma pkd / pk): never the bar;
* updatePrior on r1 and on r1 reversed gives the same L and agrees to 1e-13,
  so no merge decision of the GPU test's inputs is borderline;
* the small-sample p-values of the designed markers: finite, and within 1e-9
  of mpmath's incomplete beta function of the same sums (the conditioning of
  1 - rxy^2 at t = 1e3);
* the oracle's assoc_se gives exact zeros in the strongly negative tail."""
import math

import numpy as np
import pytest

import _mix
from oracle import pyoracle as O


def test_mix_shapes():
    for L in (2, 13, 16, 24, 64):
        probs, vars_ = _mix.mix(L)
        assert len(probs) == len(vars_) == L and vars_[0] == 0.0 and vars_[-1] == (1e-3 if L == 2 else 1.0)
        assert abs(sum(probs) - 1.0) < L * 2.0 ** -52 and probs[0] == 0.99
        assert list(vars_) == sorted(vars_)
    assert _mix.mix(13, 8.0)[1][-1] == 8.0
    assert _mix.mix(13)[1][1] == 1e-6


def test_denoise_reference_is_a_posterior():
    """The mpmath reference against brute-force quadrature of the posterior
    (one slab, one wide mixture): it is the model's, not the code's."""
    import mpmath as mp

    for L, gam1, r in ((2, 35.0, 0.07), (13, 1.0, -1.9)):
        probs, vars_s = _mix.denoise_mix(L)
        (E, V), = _mix.denoise_ref([r], gam1, probs, vars_s)
        with mp.workdps(30):
            s = 1 / mp.mpf(gam1)

            def lik(x):
                return mp.exp(-(r - x) ** 2 / (2 * s))

            # the spike is a point mass at 0; the slabs are integrated piecewise around 0 and r
            num1 = num2 = mp.mpf(0)  # (x and x^2 vanish at the spike)
            den = probs[0] * lik(0)
            for p, v in zip(probs[1:], vars_s[1:]):
                sd = mp.sqrt(v)

                def f(x, k, p=p, v=v):
                    return p * mp.npdf(x, 0, mp.sqrt(v)) * lik(x) * x ** k

                pts = sorted({-12 * sd, 0, mp.mpf(r), 12 * sd, mp.mpf(r) - 12 * mp.sqrt(s), mp.mpf(r) + 12 * mp.sqrt(s)})
                den += mp.quad(lambda x: f(x, 0), pts)
                num1 += mp.quad(lambda x: f(x, 1), pts)
                num2 += mp.quad(lambda x: f(x, 2), pts)
            Eq = num1 / den
            Vq = num2 / den - Eq * Eq
            assert abs(E - Eq) <= 1e-12 * abs(Eq), (L, gam1, r)
            assert abs(V - gam1 * Vq) <= 1e-10 * abs(gam1 * Vq), (L, gam1, r)


@pytest.mark.parametrize("L", _mix.DENOISE_LS)
def test_oracle_denoiser_against_mpmath(L):
    worst_g = worst_gd = 0.0
    for gam1 in _mix.DENOISE_GAM1:
        grp = _mix.denoise_group(L, gam1)
        go, gdo = grp["oracle"]
        assert np.all(np.isfinite(go)) and np.all(np.isfinite(gdo)), gam1
        eg, ed = grp["oracle_errs"]
        print(f"L={L} gam1={gam1:g}: oracle max|g-ref|/|r| = {eg:.3e}, max|gd-ref| = {ed:.3e}")
        if gam1 >= 1e10:  # |sigma| < 1e-10: g = r, gd = 1 by the code's shortcut, which is not the model
            assert np.array_equal(go, grp["r1"]) and np.all(gdo == 1.0)
            continue
        worst_g, worst_gd = max(worst_g, eg), max(worst_gd, ed)
        assert eg <= 4 * 1.3e-14, gam1
        assert ed <= 4 * 1.3e-12, gam1
    assert worst_g > 0 and worst_gd > 0


@pytest.mark.parametrize("M", [m for m in _mix.PRIOR_MS if m <= 2100])
def test_update_prior_order_of_r1(M):
    r1 = _mix.prior_r1(M)
    for L, em, lv, mg in _mix.prior_cases(M):
        p, v = _mix.oracle_prior(r1, L, em, lv, mg)
        pr, vr = _mix.oracle_prior(r1[::-1].copy(), L, em, lv, mg)
        assert np.all(np.isfinite(p)) and np.all(np.isfinite(v)), (L, em, lv, mg)
        assert len(p) == len(pr), (L, em, lv, mg)
        assert np.allclose(p, pr, rtol=1e-13, atol=0) and np.allclose(v, vr, rtol=1e-13, atol=0), (L, em, lv, mg)
        if mg == 0.0:
            assert len(p) == L


@pytest.mark.parametrize("N", _mix.PVAL_NS)
def test_small_sample_pvalues_against_mpmath(N):
    X, y = _mix.pval_problem(N)
    po, sto = O.assoc_loo(X, y, np.zeros(_mix.PVAL_MT))
    assert np.all(np.isfinite(po)) and np.all((po >= 0) & (po <= 1))
    nt = len(_mix.PVAL_TS)
    df = N - 2
    # the designed markers reach their targets: t from the sums, to the sums' rounding
    for k, t in enumerate(_mix.PVAL_TS):
        sx, sxx, sxy, sy, syy = sto[k]
        rxy = (sxy - sx * sy / N) / math.sqrt((sxx - sx * sx / N) * (syy - sy * sy / N))
        assert abs(rxy - t / math.sqrt(df + t * t)) < 1e-12, (k, t)
    pm = np.array([_mix.pval_mp(s, N) for s in sto[:nt]])
    gap = np.abs(po[:nt] - pm) / pm
    print(f"N={N}: p from {po[:nt].min():.3e}, oracle vs mpmath {gap.max():.3e}")
    assert np.all(gap <= 1e-9), gap.max()
    assert po[0] > 0.99 and np.all(np.diff(po[:nt]) < 0)  # t = 0 first, then increasing |t|


def test_oracle_se_tails():
    r1 = _mix.se_r1()
    po = O.assoc_se(r1, _mix.SE_GAM1, _mix.SE_N)
    sd = math.sqrt(1.0 / (_mix.SE_GAM1 * _mix.SE_N))
    z = r1 / sd
    assert np.all(np.isfinite(po))
    assert np.all(po[z < -9] == 0.0)  # 1 - erfc(.)/2 with erfc = 2 to the last bit
    assert np.all(po[np.abs(r1) <= 1e-300] == 0.5)
    pos = r1 > 1e-300
    pm = _mix.se_mp(r1[pos])
    assert np.all(po[pos] > 0) and po[pos].min() < 1e-280
    assert np.all(np.abs(po[pos] - pm) <= 4 * 2.0 ** -52 * pm)  # glibc's erfc: < 1 ulp, and the halving is exact
