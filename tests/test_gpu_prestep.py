"""The pre-step (pcg.cpp): an operator slot whose own system has
stopped forms T1 = A^T A b and U1 = A T1 of the NEXT iteration's Onsager
right-hand side b; that iteration composes its Onsager solve's first CG step
from them without a pass over X and carries the second step in the head-start
pass, so it takes 1 + max(k1, k2 - 2) passes instead of 1 + max(k1, k2 - 1).

Every step is still the reference's up to re-association (A^T A is applied to
b instead of b/diag, and <d,p> is summed in another order), so the runs with
the pre-step forced on (vampomi_dev_set_variant(ctx, 7, 1)) and off agree in
every integer count and within the bars test_headstart uses for the same kind
of change; the executed passes follow the slot rule exactly."""
import functools

import numpy as np
import pytest

from conftest import relerr
from _data import make_problem

pytestmark = pytest.mark.gpu

va = pytest.importorskip("vampomi_amd")
from oracle import pyoracle as O  # noqa: E402  (checker)


@functools.lru_cache(maxsize=None)
def _problem(N, Mt, kind=0, seed=3, h2=0.8):
    if kind == "tail":  # tests/test_gpu_tail.py's problem (its stop criterion fires)
        return make_problem(N, Mt)
    X = O.generate_markers(seed, kind, N, 0, Mt)
    rng = np.random.default_rng(seed)
    nc = max(1, Mt // 10)
    beta = np.zeros(Mt)
    idx = rng.choice(Mt, nc, replace=False)
    beta[idx] = rng.normal(0, np.sqrt(h2 / nc), nc)
    mave, msig = O.marker_stats(X)
    g = ((X - mave[:, None]) * msig[:, None]).T @ beta
    y = O.standardize_phen(g + rng.normal(0, np.sqrt(1 - h2), N))
    return X, y, beta


@functools.lru_cache(maxsize=None)
def _oracle(N, Mt, kind, **kw):
    X, y, beta = _problem(N, Mt, kind)
    return O.vamp_infere(X, y, Mt, true_signal=beta, **kw)


def _gpu(N, Mt, kind, prestep, op_variant=None, **kw):
    """One run; prestep: the value of variant 7 (None: the default)."""
    X, y, beta = _problem(N, Mt, kind)
    with va.Data(N, Mt) as d:
        d.load_meth(X)
        if prestep is not None:
            d.set_variant(7, prestep)
        if op_variant is not None:
            d.set_variant(3, op_variant)
        d.set_phen(y, standardize=False)
        v = va.Vamp(d, va.VampOptions(**kw), true_signal=beta)
        x1 = v.infere(keep_hist=True)
        s = v.summary()
        n = s["iterations"]
        s["x1_hist"] = v.x1_hist[:n, : d.M].copy()
        s["r1_hist"] = v.r1_hist[:n, : d.M].copy()
        s["x1_final"] = x1
        s["made"], s["used"] = d.prestep_counts()
    return s


def _simulate(cg, ons, max_iter, prestep=True):
    """The schedule's executed passes over X and the pre-steps made / used,
    from the run's own CG (k1) and Onsager (k2) step counts.

    Iteration 1 has no head start: one A.x pass, then max(k1, k2) steps.  From
    iteration 2 on the head-start pass carries the Onsager solve's step 1, or
    its step 2 when the previous iteration made a pre-step (J = 1: step 1 is
    composed), and max(k1, k2 - 1 - J) regular steps follow.  A regular step
    has a free slot when one system has stopped and the other has not: an
    iteration makes a pre-step iff its systems do not stop together (and a
    next iteration exists to use it)."""
    passes = made = used = 0
    have = False
    for i, (k1, k2) in enumerate(zip(cg, ons)):
        head = i > 0
        J = 1 if (head and have and prestep) else 0
        used += J
        rest = k2 - (1 + J if head else 0)  # the Onsager solve's regular steps
        passes += 1 + max(k1, rest)
        have = prestep and i + 1 < max_iter and (rest <= 0 or rest != k1)
        made += 1 if have else 0
    return passes, made, used


def _assert_close(a, b):
    """On against off: the bars of test_headstart."""
    assert a["iterations"] == b["iterations"]
    assert a["cg_iters"] == b["cg_iters"] and a["ons_iters"] == b["ons_iters"] and a["L"] == b["L"]
    errs = [max(relerr(a["x1_hist"][k], b["x1_hist"][k]), relerr(a["r1_hist"][k], b["r1_hist"][k]))
            for k in range(a["iterations"])]
    print("pre-step on vs off, max rel err per iteration:", ["%.1e" % e for e in errs])
    assert max(errs) <= 1e-11
    assert np.allclose(np.array(a["params"]), np.array(b["params"]), rtol=1e-11, atol=0)
    assert np.allclose(np.array(a["metrics"]), np.array(b["metrics"]), rtol=1e-10, atol=1e-13, equal_nan=True)
    assert a["a_passes_ref"] == b["a_passes_ref"]


def _assert_parity(s, ref, tol=1e-10):
    assert s["iterations"] == ref["iterations"]
    assert s["cg_iters"] == ref["cg_iters"].tolist()
    assert s["ons_iters"] == ref["ons_iters"].tolist()
    assert s["L"] == ref["L"].tolist()
    for k in range(s["iterations"]):
        assert relerr(s["x1_hist"][k], ref["x1_hist"][k]) <= tol, f"x1 it {k + 1}"
        assert relerr(s["r1_hist"][k], ref["r1_hist"][k]) <= tol, f"r1 it {k + 1}"
    assert np.allclose(np.array(s["params"]), ref["params"], rtol=1e-9, atol=0)
    assert np.allclose(np.array(s["metrics"]), ref["metrics"], rtol=1e-9, atol=1e-12, equal_nan=True)


def _assert_schedule(s, max_iter, prestep=True):
    passes, made, used = _simulate(s["cg_iters"], s["ons_iters"], max_iter, prestep)
    print("passes", s["a_passes_exec"] - 1, "simulated", passes, "made/used", s["made"], s["used"], "simulated",
          made, used, "k1", s["cg_iters"], "k2", s["ons_iters"])
    assert s["a_passes_exec"] == 1 + passes  # + A^T y
    assert (s["made"], s["used"]) == (made, used)


BITWISE = ("x1_hist", "r1_hist", "x1_final", "params", "metrics")


def _assert_bitwise(a, b):
    for k in ("iterations", "cg_iters", "ons_iters", "L", "a_passes_exec", "made", "used"):
        assert a[k] == b[k], k
    for k in BITWISE:
        np.testing.assert_array_equal(np.asarray(a[k]), np.asarray(b[k]), err_msg=k)


@pytest.mark.parametrize("N,Mt,its,kind,opv", [(1000, 2000, 30, 0, None), (4099, 3001, 12, 1, None),
                                                (301, 517, 12, 0, None),
                                                (3000, 2000, 10, 1, 1000 + 2 * 100 + 2),
                                                (3000, 2000, 10, 0, 1000 + 4 * 100 + 4),
                                                (1000, 2000, 6, 0, 1000 + 1 * 100 + 0)])
def test_prestep_on_against_off(N, Mt, its, kind, opv):
    """Forced on against off: the same counts, values within rounding, the
    oracle's parity bar, and the slot rule's passes with at least one use."""
    kw = dict(max_iter=its, stop_criteria_thr=0.0)
    a = _gpu(N, Mt, kind, 1, opv, **kw)
    b = _gpu(N, Mt, kind, 0, opv, **kw)
    _assert_close(a, b)
    _assert_schedule(a, its)
    _assert_schedule(b, its, prestep=False)
    assert a["used"] >= 1
    assert a["a_passes_exec"] <= b["a_passes_exec"]  # (a use saves a pass where the Onsager solve was the longer one)
    _assert_parity(a, _oracle(N, Mt, kind, **kw))


def test_prestep_cg_limits():
    """CG_max_iter 1, 2, 3: the composed step and the head-start pass count
    towards the Onsager solve's limit as its own steps do."""
    N, Mt = 800, 1500
    for cgmax in (1, 2, 3):
        kw = dict(max_iter=5, stop_criteria_thr=0.0, CG_max_iter=cgmax)
        a = _gpu(N, Mt, 0, 1, **kw)
        b = _gpu(N, Mt, 0, 0, **kw)
        assert a["cg_iters"] == b["cg_iters"] and a["ons_iters"] == b["ons_iters"], cgmax
        assert max(a["ons_iters"]) <= cgmax and max(a["cg_iters"]) <= cgmax
        for k in range(5):
            assert relerr(a["x1_hist"][k], b["x1_hist"][k]) <= 1e-11, (cgmax, k)
            assert relerr(a["r1_hist"][k], b["r1_hist"][k]) <= 1e-11, (cgmax, k)
        _assert_schedule(a, 5)
        assert a["used"] >= 1, cgmax
        _assert_parity(a, _oracle(N, Mt, 0, **kw))


def test_prestep_early_stop():
    """The stop criterion fires after an iteration that made a pre-step:
    nothing uses it, and the results are the off run's."""
    N, Mt = 1500, 3001  # (the oracle stops this one at iteration 13 of 40)
    kw = dict(max_iter=40, stop_criteria_thr=1e-2)
    a = _gpu(N, Mt, "tail", 1, **kw)
    b = _gpu(N, Mt, "tail", 0, **kw)
    assert a["iterations"] < 40
    _assert_close(a, b)
    _assert_schedule(a, 40)
    assert a["used"] >= 1 and a["made"] == a["used"] + 1  # the last iteration's was never used
    _assert_parity(a, _oracle(N, Mt, "tail", **kw))


def test_prestep_repeatable(monkeypatch):
    """Two forced-on runs are bitwise equal, and so is one with the start
    queued ahead off (tests/test_gpu_tail.py's switch)."""
    N, Mt = 1000, 2000
    kw = dict(max_iter=12, stop_criteria_thr=0.0)
    a = _gpu(N, Mt, 0, 1, **kw)
    b = _gpu(N, Mt, 0, 1, **kw)
    _assert_bitwise(a, b)
    monkeypatch.setenv("VAMPOMI_PRE_AHEAD", "0")
    c = _gpu(N, Mt, 0, 1, **kw)
    _assert_bitwise(a, c)
    assert a["used"] >= 1


def test_default_unchanged_below_the_gate():
    """Below the size gate the default schedule is the one without the
    pre-step, bit for bit."""
    N, Mt = 1000, 2000
    kw = dict(max_iter=8, stop_criteria_thr=0.0)
    a = _gpu(N, Mt, 0, None, **kw)
    b = _gpu(N, Mt, 0, 0, **kw)
    _assert_bitwise(a, b)
    assert (a["made"], a["used"]) == (0, 0)
