"""Helpers of tests/test_gpu_assoc_multi.py: problems with several phenotypes
on one design, the reference loop (set_phen + assoc_loo per phenotype), the
association tests' bars restated from tests/test_gpu_assoc.py, and the
command-line runs."""
import os
import subprocess
import time

import numpy as np

from conftest import relerr
from _data import make_problem, phen_from_markers
from oracle import pyoracle as O

TMAX = 9  # phenotypes per problem: two full chunks of four and a remainder


def estimate(beta, N, scale=0.9, seed=0):
    """tests/test_gpu_assoc.py's _estimate: what an _it_K.bin holds."""
    rng = np.random.default_rng(seed)
    return (beta * scale + rng.normal(size=beta.shape) * 1e-3) / np.sqrt(N)


_problems = {}


def problem(N, Mt, kind, T=TMAX):
    """X (Mt, N), Y (T, N) standardised phenotypes of different seeds on X,
    est (T, Mt) their estimates; made once per shape and left unchanged."""
    key = (N, Mt, kind, T)
    if key not in _problems:
        X, y0, b0 = make_problem(N, Mt, kind=kind)
        ys, es = [y0], [estimate(b0, N)]
        for t in range(1, T):
            y, beta = phen_from_markers(X, seed=10 + t, lam=0.1 + 0.02 * t, h2=0.8 - 0.05 * t)
            ys.append(y)
            es.append(estimate(beta, N, seed=t))
        X.setflags(write=False)
        Y, E = np.stack(ys), np.stack(es)
        Y.setflags(write=False)
        E.setflags(write=False)
        _problems[key] = (X, Y, E)
    return _problems[key]


def single_loop(d, Y, est, standardize):
    """The parent path: per phenotype set_phen + assoc_loo on the context d
    (est: (T, M), this context's slices).  (pvals (T, M), stats (T, M, 5))"""
    pv, st = [], []
    for t in range(len(Y)):
        d.set_phen(Y[t], standardize=standardize)
        p, s = d.assoc_loo(est[t])
        pv.append(p.copy())
        st.append(s.copy())
    return np.stack(pv), np.stack(st)


def loo_bytes(d, esize, KT):
    """The algorithmic bytes of one association pass that serves KT phenotypes."""
    return esize * d.N * d.M + 8 * d.N * KT + 8 * d.M * 6 * KT


# ---- the bars of tests/test_gpu_assoc.py ----
def order_spread(X, y, est, po):
    """|p(oracle sums) - p(pairwise sums)| / p per marker (numpy restatement)."""
    N = X.shape[1]
    mave, msig = O.marker_stats(X)
    x1 = est * np.sqrt(N)
    ymod = y - O.ax(X, mave, msig, x1)
    ym = ymod[None, :] + X / np.sqrt(N) * x1[:, None]
    sums = np.stack([X.sum(1), (X * X).sum(1), (X * ym).sum(1), ym.sum(1), (ym * ym).sum(1)], axis=1)
    pp = np.array([O.reg1d_pval(*s, N) for s in sums])
    return np.abs(pp - po) / np.maximum(po, 1e-300)


def check_loo(p, st, po, sto, spread):
    for q in range(5):
        assert relerr(st[:, q], sto[:, q]) < 1e-13, q
    tol = np.maximum(1e-10, 10 * spread)
    ok = np.abs(p - po) <= tol * po + 1e-300
    assert ok.all(), (p[~ok][:5], po[~ok][:5], spread[~ok][:5])


def check_pfun(p, st, N):
    pf = np.array([O.reg1d_pval(*s, N) for s in st])
    assert np.all(np.abs(p - pf) <= 1e-12 * pf + 1e-300)


# ---- the command line ----
def write_inputs(tmp, X, Y, est, na=None):
    """ex.bin, y<t>.phen (na: {t: rows written as NA}), e<t>_it_7.bin and the
    trait file; returns (meth, phen paths, estimate paths, trait file)."""
    Xp = os.path.join(tmp, "ex.bin")
    X.astype("<f8").tofile(Xp)
    phen, ests = [], []
    for t in range(len(Y)):
        phen.append(os.path.join(tmp, "y%d.phen" % t))
        with open(phen[-1], "w") as f:
            for i, v in enumerate(Y[t]):
                f.write("%d %d %s\n" % (i, i, "NA" if na and i in na.get(t, ()) else "%0.10f" % v))
        ests.append(os.path.join(tmp, "e%d_it_7.bin" % t))
        est[t].astype("<f8").tofile(ests[-1])
    tf = os.path.join(tmp, "traits.txt")
    with open(tf, "w") as f:
        f.write("# name phenotype estimate\n")
        for t in range(len(Y)):
            f.write("trait%d %s %s\n" % (t, phen[t], ests[t]))
    return Xp, phen, ests, tf


def launch(cmd, P, tmp, tag):
    """P processes of cmd (ranks 0..P-1) through the shm communicator, as
    tests/test_gpu_cli_ranks.py starts them; (Popen objects, log paths)."""
    rdzv = os.path.join(tmp, f".{tag}.rdzv")
    procs, logs = [], []
    for r in range(P):
        env = dict(os.environ, VAMPOMI_RANK=str(r), VAMPOMI_NRANKS=str(P), VAMPOMI_COMM="shm", VAMPOMI_RDZV=rdzv,
                   VAMPOMI_COLL_TIMEOUT_S="60", VAMPOMI_COMM_INIT_TIMEOUT_S="60", VAMPOMI_RUN_ID=f"{tag}-{os.getpid()}")
        log = os.path.join(tmp, f"{tag}_rank{r}.log")
        logs.append(log)
        with open(log, "w") as fh:
            procs.append(subprocess.Popen(cmd, stdout=fh, stderr=subprocess.STDOUT, env=env))
    return procs, logs


def wait(procs, timeout):
    deadline = time.monotonic() + timeout
    rcs = []
    for p in procs:
        try:
            rcs.append(p.wait(max(0.1, deadline - time.monotonic())))
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
    return rcs
