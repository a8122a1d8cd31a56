"""The leave-one-chromosome-out association test (vampomi_assoc_loco, DESIGN.md
§4.16) on the GPU.

Two contracts.  The marker pass: a marker's five sums and p-value are, bit for
bit, those of the plain marginal test against y_c (assoc_loo_multi of R[c]
without an estimate), c the marker's label.  The residuals: R[c] is y - A (x1
zeroed inside c) to 1e-12 (||y|| + sum ||z_c||), against the oracle and
against the engine's own A.x.  End to end the p-values meet the bars of
tests/_assoc_multi.py against the oracle's assoc_loo with the estimate zeroed
inside the label.  Every case runs once on the device (run()); the tests read
what it kept.

Shapes (tests/_assoc_loco.py): 301 x 257 (f64, f32), 1001 x 517 (f64, f32,
u16), and 1101 x 700 (f64, u16), whose N spans three row tiles of the
segmented A.x and whose labels hold up to three chunks."""
import ctypes as C
import os
import threading
import time

import numpy as np
import pytest

import _assoc_loco as L
import _assoc_multi as H

pytestmark = pytest.mark.gpu

va = pytest.importorskip("vampomi_amd")
from oracle import pyoracle as O  # noqa: E402  (checker)

CASES = [(s, st, ls) for s in L.SHAPES for st in L.STORAGES[s] for ls in L.LABELSETS]
IDS = ["%dx%d-%s-%s" % (s[0], s[1], st, ls) for s, st, ls in CASES]

_runs = {}


def measure(d, est, lab, G):
    """One context's answers: the call (twice), the marginal tests against every
    R[c], the engine's own A.x of every zeroed vector, the two other tests."""
    N = d.N
    out = {"X": d.get_meth_data(), "y": d.get_phen()}
    d.reset_stats()
    p, st, R = d.assoc_loco(est, lab, G=G, resid=True)
    s = d.stats()
    out.update(p=p.copy(), st=st.copy(), R=R.copy(), passes=s.a_passes_exec, ax_launches=s.ax.launches,
               loo_launches=s.loo.launches)
    p2, st2, R2 = d.assoc_loco(est, lab, G=G, resid=True)
    out["again"] = (p2.copy(), st2.copy(), R2.copy())
    out["marginal"] = [d.assoc_loo_multi(R[c][None], None, standardize=False) for c in range(G)]
    x1 = est * np.sqrt(N)
    out["own_ax"] = np.stack([out["y"] - d.Ax(L.zeroed(x1, lab, c)) for c in range(G)])
    out["p_loo"] = d.assoc_loo(est)[0].copy()
    p0, s0 = d.assoc_loo(np.zeros(d.M))
    out["p_marg"], out["st_marg"] = p0.copy(), s0.copy()
    d.reset_stats()
    pn, sn = d.assoc_loco(None, lab, G=G)
    s = d.stats()
    out["none"] = (pn.copy(), sn.copy(), s.a_passes_exec, s.ax.launches)
    out["y_after"] = d.get_phen()
    return out


def run(case):
    if case not in _runs:
        (N, Mt, kind), storage, ls = case
        X, y, est = L.problem(N, Mt, kind)
        lab, G = L.labels(ls, Mt)
        with va.Data(N, Mt, storage=storage) as d:
            d.load_meth(X)
            d.set_phen(y, standardize=False)
            out = measure(d, est, lab, G)
        out.update(est=est, lab=lab, G=G, N=N)
        out["ref"] = L.oracle_refs(out["X"], out["y"], est, lab, G)
        _runs[case] = out
    return _runs[case]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_marker_pass_is_the_marginal_test_against_the_label_residual_bitwise(case):
    r = run(case)
    seen = np.zeros(len(r["lab"]), dtype=bool)
    for c in range(r["G"]):
        idx = r["lab"] == c
        pm, sm = r["marginal"][c]
        assert np.array_equal(r["st"][idx], sm[0][idx]), c
        assert np.array_equal(r["p"][idx], pm[0][idx]), c
        seen |= idx
    assert seen.all() and np.all(np.isfinite(r["p"])) and np.all((r["p"] >= 0) & (r["p"] <= 1))
    assert np.array_equal(r["y_after"], r["y"])  # the context's own phenotype is unchanged


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_residuals_against_the_oracle_and_the_engines_own_ax(case):
    r = run(case)
    a = L.check_resid(r["R"], r["ref"]["R"], r["ref"]["scale"], "oracle")
    b = L.check_resid(r["R"], r["own_ax"], r["ref"]["scale"], "own A.x")
    print("residual error / scale: oracle %.2e, own A.x %.2e" % (a, b))
    if r["G"] > 1:  # an unused label's residual is y - z, a label's own effect stays in
        assert not np.array_equal(r["R"][0], r["R"][1])


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_end_to_end_against_the_oracle(case):
    r = run(case)
    L.check_against_oracle(r["p"], r["st"], r["ref"], r["N"])


@pytest.mark.parametrize("case", [c for c in CASES if c[2] == "g5"], ids=[i for i in IDS if i.endswith("g5")])
def test_it_is_a_different_test(case):
    """Neither assoc_loo(est) nor the marginal test: at least one p-value more
    than 1e-3 (relative) away from each (the oracle alone shows the same,
    tests/test_assoc_loco.py)."""
    r = run(case)
    assert L.differs(r["p"], r["p_loo"]) and L.differs(r["p"], r["p_marg"])


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_no_estimate_is_the_marginal_test_in_one_pass(case):
    r = run(case)
    pn, sn, passes, ax = r["none"]
    assert passes == 1 and ax == 0
    assert np.array_equal(sn, r["st_marg"]) and np.array_equal(pn, r["p_marg"])


@pytest.mark.parametrize("case", [c for c in CASES if c[2] in ("g5", "g64")],
                         ids=[i for i in IDS if i.endswith(("g5", "g64"))])
def test_two_passes_whatever_g(case):
    r = run(case)
    assert (r["passes"], r["ax_launches"], r["loo_launches"]) == (2, 1, 1)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_two_calls_give_equal_bits(case):
    r = run(case)
    p2, st2, R2 = r["again"]
    assert np.array_equal(p2, r["p"]) and np.array_equal(st2, r["st"]) and np.array_equal(R2, r["R"])


# ---- loopback ranks ----
def _run_ranks(monkeypatch, P, N, Mt, fn, timeout=100):
    """fn(rank, data) on P loopback rank threads (tests/test_gpu_assoc_multi.py's)."""
    monkeypatch.setenv("VAMPOMI_COMM", "loopback")
    cid = os.urandom(va.UNIQUE_ID_BYTES)
    res, errs = [None] * P, []

    def work(r):
        try:
            with va.Data(N, Mt, rank=r, nranks=P, comm_id=cid, device=0) as d:
                res[r] = fn(r, d)
        except BaseException as e:  # noqa: BLE001 - reported below
            errs.append((r, e))

    th = [threading.Thread(target=work, args=(r,), daemon=True) for r in range(P)]
    [t.start() for t in th]
    deadline = time.monotonic() + timeout
    [t.join(max(0.0, deadline - time.monotonic())) for t in th]
    stuck = [r for r, t in enumerate(th) if t.is_alive()]
    assert not stuck, f"ranks {stuck} stuck in a collective; errors of the others: {errs}"
    assert not errs, errs
    return res


RANK_SHAPE = (1001, 517, 1)


def rank_labels(Mt):
    """G = 4: label 0 only among the first 60 markers (absent from the last
    rank of 2 and of 3), label 3 unused, labels 1 and 2 at random everywhere."""
    rng = np.random.default_rng(8)
    lab = rng.integers(1, 3, size=Mt)
    lab[rng.choice(60, 25, replace=False)] = 0
    return lab.astype(np.int32), 4


_one_rank = {}


def one_rank():
    if not _one_rank:
        N, Mt, kind = RANK_SHAPE
        X, y, est = L.problem(N, Mt, kind)
        lab, G = rank_labels(Mt)
        with va.Data(N, Mt) as d:
            d.load_meth(X)
            d.set_phen(y, standardize=False)
            p, st, R = d.assoc_loco(est, lab, G=G, resid=True)
        _one_rank.update(p=p.copy(), st=st.copy(), R=R.copy(), ref=L.oracle_refs(X, y, est, lab, G))
    return _one_rank


@pytest.mark.parametrize("P", [2, 3])
def test_ranks(monkeypatch, P):
    N, Mt, kind = RANK_SHAPE
    X, y, est = L.problem(N, Mt, kind)
    lab, G = rank_labels(Mt)
    one = one_rank()

    def fn(r, d):
        sl = slice(d.S, d.S + d.M)
        d.load_meth(X[sl])
        d.set_phen(y, standardize=False)
        p, st, R = d.assoc_loco(est[sl], lab[sl], G=G, resid=True)
        marg = [d.assoc_loo_multi(R[c][None], None, standardize=False) for c in range(G)]
        return d.S, d.M, p.copy(), st.copy(), R.copy(), marg

    res = _run_ranks(monkeypatch, P, N, Mt, fn)
    sizes = [r[1] for r in res]
    assert len(set(sizes)) > 1  # uneven shards
    assert not np.any(lab[res[-1][0]:] == 0) and all(np.any(lab[r[0]:r[0] + r[1]] == 1) for r in res)
    for S, M, p, st, R, marg in res:
        ll = lab[S:S + M]
        for c in range(G):  # the marker-pass contract on every rank
            idx = ll == c
            assert np.array_equal(st[idx], marg[c][1][0][idx]) and np.array_equal(p[idx], marg[c][0][0][idx])
        assert np.array_equal(R, res[0][4])  # the same on every rank
        L.check_resid(R, one["R"], one["ref"]["scale"], "one rank")
        L.check_resid(R, one["ref"]["R"], one["ref"]["scale"], "oracle")
    p = np.concatenate([r[2] for r in res])
    st = np.concatenate([r[3] for r in res])
    L.check_against_oracle(p, st, one["ref"], N)
    H.check_loo(p, st, one["p"], one["st"], one["ref"]["spread"])  # against the one-rank run, the same bars


# ---- other contexts ----
@pytest.mark.parametrize("what", ["adjust", "meth_na", "rows"])
def test_adjusted_mean_filled_and_subset_contexts(what):
    N, Mt, kind = L.SHAPES[0]
    X, y, est = L.problem(N, Mt, 1)
    lab, G = L.labels("g5", Mt)
    rng = np.random.default_rng(4)
    kw, yin = {}, y * 1.5 + 0.25
    if what == "adjust":
        kw["adjust"] = rng.normal(size=(N, 3))
    elif what == "meth_na":
        X = X.copy()
        X[rng.integers(0, Mt, 400), rng.integers(0, N, 400)] = np.nan
        kw["meth_na"] = "mean"
    else:
        kw["rows"] = np.sort(rng.choice(N, 257, replace=False))
        yin = yin[kw["rows"]]
    with va.Data(N, Mt, **kw) as d:
        d.load_meth(X)
        d.set_phen(yin, standardize=True)
        r = measure(d, est, lab, G)
        n = d.N
    ref = L.oracle_refs(r["X"], r["y"], est, lab, G)
    L.check_resid(r["R"], ref["R"], ref["scale"], "oracle")
    L.check_resid(r["R"], r["own_ax"], ref["scale"], "own A.x")
    centred = None
    if what == "adjust":  # sum X and sum y are zero but for rounding: see check_against_oracle
        centred = {0: np.abs(r["X"]).sum(axis=1), 3: np.abs(ref["R"]).sum(axis=1)[lab]}
    L.check_against_oracle(r["p"], r["st"], ref, n, centred)
    if what != "adjust":  # (an adjusted context projects assoc_loo_multi's phenotype again: other bits)
        for c in range(G):
            idx = lab == c
            assert np.array_equal(r["st"][idx], r["marginal"][c][1][0][idx])


# ---- errors ----
def test_argument_and_state_errors_leave_the_context_usable():
    N, Mt, kind = L.SHAPES[0]
    X, y, est = L.problem(N, Mt, kind)
    lab, G = L.labels("g5", Mt)
    lib = va.load()
    dp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    e64 = np.ascontiguousarray(est)
    with va.Data(N, Mt) as d:
        with pytest.raises(va.VampomiError) as e:
            d.assoc_loco(est, lab, G=G)
        assert e.value.status == 6  # no matrix
        d.load_meth(X)
        with pytest.raises(va.VampomiError) as e:
            d.assoc_loco(est, lab, G=G)
        assert e.value.status == 6  # no phenotype
        d.set_phen(y, standardize=False)
        good = d.assoc_loco(est, lab, G=G)
        assert lib.vampomi_assoc_loco(d.ctx, dp(e64), None, G, None, None, None, 0) == 1  # null labels
        for g in (0, -1, 65):
            assert lib.vampomi_assoc_loco(d.ctx, dp(e64), dp(lab), g, None, None, None, 0) == 1, g
        for bad in (-1, G):
            lb = lab.copy()
            lb[Mt - 1] = bad
            with pytest.raises(va.VampomiError) as e:
                d.assoc_loco(est, lb, G=G)
            assert e.value.status == 1 and "marker %d" % (Mt - 1) in str(e.value)
        again = d.assoc_loco(est, lab, G=G)
        assert np.array_equal(again[0], good[0]) and np.array_equal(again[1], good[1])
        p64, _ = d.assoc_loco(est, ((np.arange(Mt) + 11) % 64).astype(np.int32), G=64)  # the workspaces grow
        assert np.all(np.isfinite(p64))


# ---- the command line ----
def _write_inputs(tmp, X, y, est, names):
    Xp, _, ests, _ = H.write_inputs(tmp, X, y[None], est[None])
    lf = os.path.join(tmp, "labels.txt")
    with open(lf, "w") as f:
        f.write("\n".join(names) + "\n")
    return Xp, os.path.join(tmp, "y0.phen"), ests[0], lf


@pytest.mark.parametrize("mode", ["one_process", "two_processes", "bin_class"])
def test_cli_writes_the_api_p_values(tmp_path, monkeypatch, mode):
    N, Mt, kind = 301, 500, 1
    X, y, est = L.problem(N, Mt, kind)
    if mode == "bin_class":  # cases and controls, left raw by the run
        y = (y > np.median(y)).astype(np.float64)
    lab, G = L.labels("g5", Mt)
    names = ["chr%d" % c if c else "X" for c in lab]  # first appearance: X (0), then the others in file order
    tmp = str(tmp_path)
    Xp, phen, ef, lf = _write_inputs(tmp, X, y, est, names)
    flab, fnames = va.read_labels(lf, Mt)
    P = 2 if mode == "two_processes" else 1
    cmd = [va.CLI_PATH, "--meth-file", Xp, "--N", str(N), "--Mt", str(Mt), "--run-mode", "association_test",
           "--pval-method", "loco", "--loco-file", lf, "--phen-file", phen, "--estimate-file", ef, "--out-dir", tmp,
           "--out-name", "run"] + (["--model", "bin_class"] if mode == "bin_class" else [])
    procs, logs = H.launch(cmd, P, tmp, "loco")
    assert H.wait(procs, 120) == [0] * P, [open(lg).read()[-2000:] for lg in logs]
    got = np.fromfile(os.path.join(tmp, "run_it_7_pval_loco.bin"), dtype="<f8")
    assert got.shape == (Mt,)
    txt = open(logs[0]).read()
    counts = np.bincount(flab, minlength=len(fnames))
    assert "INFO   : LOCO: %d segments (%s)" % (len(fnames), " ".join(
        "%s:%d" % (n, k) for n, k in zip(fnames, counts))) in txt
    e = np.fromfile(ef, dtype="<f8")

    def api(d, sl):
        d.load_meth(X[sl])
        d.read_phen(phen, standardize=mode != "bin_class")
        return d.assoc_loco(e[sl], flab[sl], G=len(fnames))[0].copy()

    if P == 1:
        with va.Data(N, Mt) as d:
            want = api(d, slice(0, Mt))
    else:
        want = np.concatenate(_run_ranks(monkeypatch, P, N, Mt, lambda r, d: api(d, slice(d.S, d.S + d.M))))
    assert got.tobytes() == want.tobytes()
    assert np.all((got >= 0) & (got <= 1))
