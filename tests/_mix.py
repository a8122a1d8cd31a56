"""Shared inputs and high-precision references of the large-mixture and
element-wise tests (tests/test_mixture_refs.py on the CPU,
tests/test_gpu_mixture.py and the mix* cases of the option, sharded, corner
and association tests on the GPU).

mix(L): the standard L-component spike-and-slab (1 <= L <= 64 is what the
ABI accepts): probs = [0.99, 0.01/(L-1) ...], vars = [0, geomspace(1e-6, 1,
L-1)]; mix(2) has the one slab 1e-3.

The denoiser's reference is written from the model, not from the code: for
x ~ sum_k p_k N(0, v_k) and r = x + N(0, s), s = 1/gam1, the posterior weights
are w_k ~ p_k N(r; 0, v_k + s), and
    E[x|r]        = sum_k w_k r v_k / (v_k + s)
    gam1 Var[x|r] = gam1 (sum_k w_k (v_k s / (v_k + s) + (r v_k / (v_k + s))^2) - E[x|r]^2)
(d E[x|r] / d r = Var[x|r] / s, which is what vamp::g1d returns), in mpmath
at 50 digits with the log-weights normalised by their maximum."""
from __future__ import annotations

import functools
import json
import math
import os

import numpy as np

from oracle import pyoracle as O

N_SMALL = 8  # samples of the contexts that only carry an M-vector (variances are scaled by it)


def mix(L: int, scale: float = 1.0):
    """(probs, vars * scale) of the standard L-component mixture, as tuples."""
    if L < 2:
        raise ValueError("mix(L) needs a spike and at least one slab")
    slabs = [1e-3] if L == 2 else np.geomspace(1e-6, 1.0, L - 1).tolist()
    probs = [0.99] + [0.01 / (L - 1)] * (L - 1)
    return tuple(probs), tuple(v * scale for v in [0.0] + slabs)


def mix_kw(L: int, **kw) -> dict:
    """mix(L) as the vars / probs options of a run (unscaled variances)."""
    probs, vars_ = mix(L)
    return dict(vars=vars_, probs=probs, **kw)


def record(kind: str, **fields) -> None:
    """One JSON line of measured figures appended to $VAMPOMI_MIXTURE_FIGURES
    (profiles/mixture_tests.md is written from them); nothing without it."""
    f = os.environ.get("VAMPOMI_MIXTURE_FIGURES")
    if f:
        with open(f, "a") as fh:
            fh.write(json.dumps(dict(kind=kind, **fields)) + "\n")


# ---------------------------------------------------------------------------
# vampomi_update_prior on its own
# ---------------------------------------------------------------------------
PRIOR_LS = (2, 11, 12, 13, 24, 64)
PRIOR_MS = (1, 63, 65, 255, 257, 2100, 524289)
PRIOR_SETTINGS = ((1, 1, 0.0), (3, 1, 0.5), (4, 0, 0.0))  # (EM_max_iter, learn_vars, merge_vars_thr)
PRIOR_GAM1 = 35.0


def prior_r1(M: int) -> np.ndarray:
    """6/7 of the entries 0.02 N(0,1), 1/7 0.4 N(0,1) (test_update_prior_entry_point's shape)."""
    rng = np.random.default_rng(1000 + M)
    big = M // 7
    return np.concatenate([rng.normal(size=M - big) * 0.02, rng.normal(size=big) * 0.4])


def prior_cases(M: int):
    """(L, EM_max_iter, learn_vars, merge) of one M: the cross product up to
    M = 2100, the widest mixture and the first beyond the register slabs above."""
    Ls = PRIOR_LS if M <= 2100 else (64, 13)
    return [(L, em, lv, mg) for L in Ls for em, lv, mg in PRIOR_SETTINGS]


def oracle_prior(r1, L, em, lv, mg):
    probs, vars_s = mix(L, N_SMALL)
    return O.update_prior(r1, PRIOR_GAM1, probs, vars_s, N_SMALL, EM_max_iter=em, learn_vars=lv, merge_vars_thr=mg)


# ---------------------------------------------------------------------------
# vampomi_denoise, element-wise
# ---------------------------------------------------------------------------
DENOISE_LS = (2, 10, 13, 64)
DENOISE_GAM1 = (1e-6, 1e-3, 1.0, 35.0, 1e3, 1e6, 1e9, 1e11)
DENOISE_M = 96
DENOISE_FLOOR = 8 * 2.0 ** -53
RED_L, RED_GAM1 = 13, 35.0
RED_MS = (1, 63, 64, 65, 255, 256, 257, 511, 512, 513, 524287, 524289)


def denoise_mix(L: int):
    """(probs, scaled vars): L = 10 is the default mixture of the options."""
    if L == 10:
        return tuple(O.DEFAULT_PROBS), tuple(v * N_SMALL for v in O.DEFAULT_VARS)
    return mix(L, N_SMALL)


def denoise_r1(L: int, gam1: float, M: int = DENOISE_M) -> np.ndarray:
    """[+0, -0, 1e-300, 1e-8], +-geomspace(1e-3, 40, 25) standard deviations of
    the widest component's r, then seeded normals at the noise's scale (where
    the spike and the narrow slabs compete), M entries (the first M of them)."""
    _, vars_s = denoise_mix(L)
    g = np.geomspace(1e-3, 40.0, 25) * math.sqrt(max(vars_s) + 1.0 / gam1)
    head = np.concatenate([[0.0, -0.0, 1e-300, 1e-8], g, -g])
    rng = np.random.default_rng(int(L * 100 + round(math.log10(gam1))))
    fill = rng.normal(size=max(M - len(head), 0)) * math.sqrt(1.0 / gam1)
    return np.concatenate([head, fill])[:M]


def denoise_ref(r1, gam1: float, probs, vars_s):
    """[(E[x|r], gam1 Var[x|r])] as mpmath numbers at 50 digits, per element."""
    import mpmath as mp

    out = []
    with mp.workdps(50):
        s = 1 / mp.mpf(gam1)
        p = [mp.mpf(float(q)) for q in probs]
        v = [mp.mpf(float(q)) for q in vars_s]
        lp = [mp.log(q) for q in p]
        lv = [mp.log(vk + s) / 2 for vk in v]
        for r in r1:
            r = mp.mpf(float(r))
            lw = [lp[k] - lv[k] - r * r / (2 * (v[k] + s)) for k in range(len(p))]
            top = max(lw)
            w = [mp.exp(q - top) for q in lw]
            W = mp.fsum(w)
            mk = [r * vk / (vk + s) for vk in v]
            E = mp.fsum(w[k] * mk[k] for k in range(len(p))) / W
            E2 = mp.fsum(w[k] * (v[k] * s / (v[k] + s) + mk[k] * mk[k]) for k in range(len(p))) / W
            out.append((E, mp.mpf(gam1) * (E2 - E * E)))
    return out


def denoise_errs(r1, g, gd, ref):
    """(largest |g - ref| / |r| over r != 0, largest |gd - ref|) as floats."""
    import mpmath as mp

    eg, ed = mp.mpf(0), mp.mpf(0)
    with mp.workdps(50):
        for r, a, b, (E, V) in zip(r1, g, gd, ref):
            if r != 0:
                eg = max(eg, abs(mp.mpf(float(a)) - E) / abs(mp.mpf(float(r))))
            ed = max(ed, abs(mp.mpf(float(b)) - V))
    return float(eg), float(ed)


def oracle_denoise(r1, gam1, probs, vars_s):
    return (np.array([O.g1(float(t), gam1, probs, vars_s) for t in r1]),
            np.array([O.g1d(float(t), gam1, probs, vars_s) for t in r1]))


@functools.lru_cache(maxsize=None)
def denoise_group(L: int, gam1: float):
    """One (L, gam1) group: r1, the mixture, the mpmath reference and the
    oracle's own largest errors against it (part of the reference)."""
    probs, vars_s = denoise_mix(L)
    r1 = denoise_r1(L, gam1)
    ref = denoise_ref(r1, gam1, probs, vars_s)
    go, gdo = oracle_denoise(r1, gam1, probs, vars_s)
    return dict(r1=r1, probs=probs, vars=vars_s, ref=ref, oracle=(go, gdo), oracle_errs=denoise_errs(r1, go, gdo, ref))


def red_r1(M: int) -> np.ndarray:
    """Reduction-size inputs: the group's head (as far as M goes), then normals."""
    return denoise_r1(RED_L, RED_GAM1, M)


def red_sample(M: int) -> np.ndarray:
    """Every index up to M = 20000; above, every 1021st plus the first and last 300."""
    if M <= 20000:
        return np.arange(M)
    return np.unique(np.concatenate([np.arange(300), np.arange(0, M, 1021), np.arange(M - 300, M)]))


# ---------------------------------------------------------------------------
# small-sample p-values
# ---------------------------------------------------------------------------
PVAL_NS = (3, 4, 5, 9, 32, 61, 62, 63, 64)  # df = 1, 2, 3, 7, 30, 59, 60, 61, 62
PVAL_TS = tuple([0.0, 1e-3, 0.5, 2.0, 2.999, 3.0, 3.001, 6.0] + np.geomspace(10.0, 1e3, 8).tolist())
PVAL_MT = 64


def pval_problem(N: int):
    """(X (64, N), y): one designed marker per target |t| in PVAL_TS,
    x = 0.5 + 0.1 (c y^ + s e^) with y^ the centred unit phenotype, e^ a seeded
    unit vector orthogonal to y^ and to the ones, c = t / sqrt(df + t^2),
    s = sqrt(df / (df + t^2)); generated markers fill up to Mt = 64."""
    from _data import make_problem

    X, y, _ = make_problem(N, PVAL_MT, seed=21)
    X = X.copy()
    one = np.ones(N) / math.sqrt(N)
    yh = y - y.mean()
    yh /= np.linalg.norm(yh)
    e = np.random.default_rng(500 + N).normal(size=N)
    for _ in range(2):
        e -= (e @ one) * one
        e -= (e @ yh) * yh
    e /= np.linalg.norm(e)
    df = N - 2
    for k, t in enumerate(PVAL_TS):
        c, s = t / math.sqrt(df + t * t), math.sqrt(df / (df + t * t))
        X[k] = 0.5 + 0.1 * (c * yh + s * e)
    return X, y


def pval_mp(sums, n: int) -> float:
    """linear_reg1d_pvals of the five sums (doubles, taken as exact) in mpmath:
    p = I_x(df/2, 1/2) with x = df / (df + t^2) = 1 - rxy^2."""
    import mpmath as mp

    with mp.workdps(50):
        sx, sxx, sxy, sy, syy = (mp.mpf(float(q)) for q in sums)
        s2y = (syy - sy * sy / n) / (n - 1)
        s2x = (sxx - sx * sx / n) / (n - 1)
        cxy = (sxy - sx * sy / n) / (n - 1)
        r2 = cxy * cxy / (s2x * s2y)
        return float(mp.betainc(mp.mpf(n - 2) / 2, mp.mpf(1) / 2, 0, 1 - r2, regularized=True))


# ---------------------------------------------------------------------------
# assoc_se tails
# ---------------------------------------------------------------------------
SE_N, SE_GAM1 = 1000, 2.5


def se_r1() -> np.ndarray:
    sd = math.sqrt(1.0 / (SE_GAM1 * SE_N))
    return np.concatenate([np.linspace(-36.0, 36.0, 145) * sd, [0.0, -0.0, 1e-300, -1e-300]])


def se_mp(r1) -> np.ndarray:
    """erfc / 2 of the double argument the code forms (upper tail, r1 > 0), in mpmath, as floats."""
    import mpmath as mp

    sd = math.sqrt(1.0 / (SE_GAM1 * SE_N))
    with mp.workdps(50):
        return np.array([float(mp.erfc(mp.mpf(-((0.0 - float(t)) / sd) / math.sqrt(2.0))) / 2) for t in r1])
