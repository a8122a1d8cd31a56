"""numpy restatement of the reference's covariate path, the checker of
tests/test_covariates.py and tests/test_gpu_covariates.py:

* data::read_covariates, src/data.cpp:159-227 (parse + standardisation);
* vamp::Newton_method_cov, grad_cov, mlogL_probit, src/vamp_probit.cpp:490-617,
  with a trace of every decision the loop takes;
* g1_bin_class / g1d_bin_class with m_cov, src/vamp_probit.cpp:469-488.

erfcx is the oracle's restatement of the reference's (oracle.pyoracle.erfcx,
src/utilities.cpp:293-363).  Tables are (N, C) arrays, one row per sample, as
the reference's Z[i][j]."""
from __future__ import annotations

import math
import re

import numpy as np

from oracle import pyoracle as O

K0 = 2.0 / math.sqrt(2 * math.pi)
SQRT2 = math.sqrt(2.0)
FATAL = "FATAL: number of covariates = %d does not match to the specified number of covariates = %d"


class CovFormatError(ValueError):
    pass


def erfcx(x: np.ndarray) -> np.ndarray:
    return np.array([O.erfcx(float(v)) for v in np.ravel(x)]).reshape(np.shape(x))


_erfc = np.vectorize(math.erfc, otypes=[float])


def normal_cdf(x):  # src/utilities.cpp normal_cdf: 0.5 * erfc(-x * M_SQRT1_2)
    return 0.5 * _erfc(-np.asarray(x, dtype=float) * math.sqrt(0.5))


# ---- data::read_covariates ----------------------------------------------------
def standardize(Z: np.ndarray) -> np.ndarray:
    """src/data.cpp:205-226: long double mean and population deviation per column."""
    Z = np.asarray(Z, dtype=np.float64)
    N, C = Z.shape
    out = np.empty_like(Z)
    for j in range(C):
        col = Z[:, j].astype(np.longdouble)
        cavg = np.longdouble(0.0)
        for v in col:
            cavg += v
        cavg = cavg / np.longdouble(float(N))
        csig = np.longdouble(0.0)
        for v in col:
            csig += (v - cavg) * (v - cavg)
        csig = np.sqrt(csig / np.longdouble(float(N)))
        if csig < 0.00000001:
            out[:, j] = 0.0
        else:
            out[:, j] = ((col - cavg) / csig).astype(np.float64)
    return out


def parse_covariates(path: str, N: int, C: int, standardize_: bool = True) -> np.ndarray:
    """(N, C) table of the file (src/data.cpp:166-197): header skipped, "\\s+"
    token split (a leading blank run gives an empty first token), two IDs
    skipped, exactly C numbers per row, N rows."""
    rows = []
    with open(path, newline="") as f:
        text = f.read()
    lines = text.split("\n")
    if lines and lines[-1] == "":
        lines.pop()  # std::getline: no empty line after a final newline
    for i, line in enumerate(lines):
        if i == 0:
            continue
        tok = re.split(r"[ \t\r\n\v\f]+", line)
        if len(tok) > 1 and tok[-1] == "":
            tok.pop()  # sregex_token_iterator(-1): no trailing empty token
        entries = tok[2:]
        if len(entries) != C:
            raise CovFormatError(FATAL % (len(entries), C))
        rows.append([float(t) for t in entries])
    if len(rows) != N:
        raise CovFormatError("covariate rows (%d) != N (%d)" % (len(rows), N))
    Z = np.array(rows, dtype=np.float64).reshape(N, C)
    return standardize(Z) if standardize_ else Z


# ---- the Newton quantities (:536-551, :490-523) ---------------------------------
def _lam(Z, y, gg, eta):
    g = gg + Z @ eta
    s = 2 * y - 1
    arg = s * g
    ratio = K0 / erfcx(-arg / SQRT2)
    lam = ratio * s
    return g, arg, lam


def mlogl(Z, y, gg, eta) -> float:
    s = 2 * y - 1
    arg = s * (gg + Z @ eta)
    return float(-np.sum(np.log(normal_cdf(arg))) / len(y))


def cov_eval(Z, y, gg, eta):
    """H (C, C), rhs (C), mlogL at eta."""
    Z = np.asarray(Z, dtype=np.float64)
    gg = np.zeros(len(y)) if gg is None else np.asarray(gg, dtype=np.float64)
    g, arg, lam = _lam(Z, y, gg, eta)
    w = lam * (lam + g)
    H = Z.T @ (Z * w[:, None])
    rhs = Z.T @ lam
    return H, rhs, float(-np.sum(np.log(normal_cdf(arg))) / len(y))


# ---- boost::numeric::ublas lu_factorize / lu_substitute ---------------------------
def lu_factorize(A: np.ndarray):
    A = A.copy()
    n = A.shape[0]
    pm = list(range(n))
    singular = 0
    for i in range(n):
        ip, t = i, 0.0
        for r in range(i, n):
            u = abs(A[r, i])
            if u > t:
                ip, t = r, u
        if A[ip, i] != 0.0:
            if ip != i:
                pm[i] = ip
                A[[i, ip]] = A[[ip, i]]
            inv = 1.0 / A[i, i]
            for r in range(i + 1, n):
                A[r, i] *= inv
        elif singular == 0:
            singular = i + 1
        for r in range(i + 1, n):
            for k in range(i + 1, n):
                A[r, k] -= A[r, i] * A[i, k]
    return A, pm, singular


def lu_substitute(A, pm, b):
    b = np.array(b, dtype=np.float64)
    n = len(b)
    for i in range(n):
        if pm[i] != i:
            b[i], b[pm[i]] = b[pm[i]], b[i]
    for i in range(n):
        t = b[i]
        if t != 0.0:
            for r in range(i + 1, n):
                b[r] -= A[r, i] * t
    for i in range(n - 1, -1, -1):
        b[i] /= A[i, i]
        t = b[i]
        if t != 0.0:
            for r in range(i):
                b[r] -= A[r, i] * t
    return b


def _dot(a, b):
    s = 0.0
    for x, v in zip(a, b):
        s += float(x) * float(v)
    return s


# ---- vamp::Newton_method_cov (:525-617) ------------------------------------------
def newton(Z, y, gg=None, eta0=None):
    """Returns (eta, trace).  trace["iters"]: outer iterations run;
    trace["final"]: index of the iteration whose step was discarded (the
    rel_err stop or a zero step), else None; per iteration: backtracks, rel_err,
    ls_margins (cur - (init + d.grad/2) of every line-search evaluation) and
    mono_margin (mlogL after - before the step; None where the loop broke first).
    A step that is exactly zero ends the loop at once (the reference would
    repeat the same iteration to the same eta)."""
    Z = np.asarray(Z, dtype=np.float64)
    N, C = Z.shape
    gg = np.zeros(N) if gg is None else np.asarray(gg, dtype=np.float64)
    eta = np.zeros(C) if eta0 is None else np.array(eta0, dtype=np.float64)
    tr = {"backtracks": [], "rel_err": [], "ls_margins": [], "mono_margin": [], "final": None}
    it = 0
    while it <= 500:
        H, rhs, init_val = cov_eval(Z, y, gg, eta)
        grad = -rhs / N
        A, pm, sing = lu_factorize(H)
        step = lu_substitute(A, pm, rhs) if sing == 0 else np.zeros(C)
        norm_eta = math.sqrt(_dot(eta, eta))
        if not np.any(step != 0.0):
            tr["backtracks"].append(0)
            tr["rel_err"].append(1.0 if norm_eta == 0 else 0.0)
            tr["ls_margins"].append([])
            tr["mono_margin"].append(None)
            tr["final"] = it
            it += 1
            break
        scale, bt, margins = 1.0, 0, []
        for _ in range(1, 300):
            displ = scale * step
            eta_new = eta + displ
            curr_val = mlogl(Z, y, gg, eta_new)
            margins.append(curr_val - (init_val + _dot(displ, grad) / 2))
            if curr_val <= init_val + _dot(displ, grad) / 2:
                break
            scale *= 0.9
            bt += 1
        diff = eta - eta_new
        rel = 1.0 if norm_eta == 0 else math.sqrt(_dot(diff, diff)) / norm_eta
        tr["backtracks"].append(bt)
        tr["rel_err"].append(rel)
        tr["ls_margins"].append(margins)
        if rel < 1e-4:
            tr["mono_margin"].append(None)
            tr["final"] = it
            it += 1
            break
        eta = eta_new
        tr["mono_margin"].append(curr_val - init_val)
        if curr_val > init_val:
            it += 1
            break
        it += 1
    tr["iters"] = min(it, 501)
    return eta, tr


def trace_is_safe(tr, margin=1e-10, band=0.05):
    """The borderline decisions of a trace are far from their thresholds: every
    line-search and monotonicity margin of a non-final iteration is at least
    `margin` in absolute value, and no rel_err lies within `band` of 1e-4."""
    for k in range(tr["iters"]):
        if abs(tr["rel_err"][k] / 1e-4 - 1.0) <= band:
            return False
        if k == tr["final"]:
            continue
        if any(abs(m) < margin for m in tr["ls_margins"][k]):
            return False
        mm = tr["mono_margin"][k]
        if mm is not None and abs(mm) < margin:
            return False
    return True


def probit_problem(N, C, seed, effect=0.5, noise=1.3):
    """Standardised Gaussian covariates (N, C), effects ~ effect, liability noise `noise`: (Z, y, eff)."""
    rng = np.random.default_rng(seed)
    Z = standardize(rng.standard_normal((N, C)))
    eff = effect * rng.standard_normal(C)
    y = (Z @ eff + noise * rng.standard_normal(N) > 0).astype(np.float64)
    return Z, y, eff


# ---- g1_bin_class / g1d_bin_class with m_cov (:469-488), probit_var = 1 -----------
def g1_bin_cov(p, tau1, y, m):
    sq = math.sqrt(1.0 + 1.0 / tau1)
    c = (p + m) / sq
    s = 2 * y - 1
    ratio = K0 / erfcx(-s * c / SQRT2)
    return p + s * ratio / tau1 / sq


def g1d_bin_cov(p, tau1, y, m):
    sq = math.sqrt(1.0 + 1.0 / tau1)
    c = (p + m) / sq
    s = 2 * y - 1
    ratio = K0 / erfcx(-s * c / SQRT2)
    return 1 - ratio / (1 + tau1 * 1.0) * (s * c + ratio)


def beta1_of(g1d_sum: float, N: int) -> float:
    """beta1 of an iteration (src/vamp_probit.cpp:226-236): the sum of g1d,
    set to N - 1 when it reaches N, over N."""
    b = float(g1d_sum)
    if b >= N:
        b = N - 1.0
    return b / N
