"""The schedule and the bits of every branch of pcg_run (pcg.cpp), pinned.

tests/golden/pcg_schedule.json holds, for each case below, what one run
queued (the launches of every A.x / A^T.u / operator class and of the
collectives, the host waits, the executed passes), what it counted (CG and
Onsager steps, pre-steps made and used) and a SHA-256 of the float64 bytes of
its x1_hat and r1 histories.  tests/golden/make_pcg_schedule.py recorded it
with the commit before pcg_run was split into its phases; a change to the
host side of the solve that queues anything differently, or moves one bit of
a result, fails here.  The fixture is never regenerated to make this pass.

The cases are the smallest shapes at which each branch is live: the two-pass
form (batch_rhs 0-3) and the one-pass form with the whole-column operator
(4) at 301 x 517; the team operator with the pre-step on and off and with the
head start off; T = 1; CG_max_iter 1 and 2; probit with and without A r0
given; vampomi_pcg cold, warm and with the Onsager stop; two loopback ranks
with the decisions folded, not folded, and <d,p> riding in the all-reduce."""
import functools
import hashlib
import json
import os

import numpy as np
import pytest

from _data import make_problem
from test_gpu_sharded import run_ranks

pytestmark = pytest.mark.gpu

va = pytest.importorskip("vampomi_amd")

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pcg_schedule.json")
TEAM2 = 1000 + 2 * 100 + 2  # operator variant: teams of 2
T1 = 1000 + 1 * 100 + 0     # operator variant: T = 1


def _vamp_case(N, Mt, its, kind=0, variants=(), model="linear", **opts):
    return dict(run="vamp", N=N, Mt=Mt, kind=kind, variants=variants, model=model,
                opts=dict(max_iter=its, stop_criteria_thr=0.0, **opts))


CASES = {
    **{f"linear_batch_rhs{b}": _vamp_case(301, 517, 6, batch_rhs=b) for b in range(5)},
    "team_prestep_on": _vamp_case(3000, 2000, 10, kind=1, variants=((3, TEAM2), (7, 1))),
    "team_prestep_off": _vamp_case(3000, 2000, 10, kind=1, variants=((3, TEAM2), (7, 0))),
    "team_headstart_off": _vamp_case(3000, 2000, 10, kind=1, variants=((3, TEAM2), (5, 0))),
    "t1_prestep_on": _vamp_case(1000, 2000, 6, variants=((3, T1), (7, 1))),
    "cg_max_iter1": _vamp_case(800, 1500, 5, variants=((5, 1),), CG_max_iter=1),
    "cg_max_iter2": _vamp_case(800, 1500, 5, variants=((5, 1),), CG_max_iter=2),
    "probit_batch_rhs1": _vamp_case(64, 128, 10, model="bin_class", batch_rhs=1),
    "probit_batch_rhs4": _vamp_case(64, 128, 10, model="bin_class", batch_rhs=4),
    "pcg_cold": dict(run="pcg", N=301, Mt=517, warm=False, onsager=False),
    "pcg_warm": dict(run="pcg", N=301, Mt=517, warm=True, onsager=False),
    "pcg_onsager": dict(run="pcg", N=301, Mt=517, warm=False, onsager=True),
    "ranks2_fold_on": dict(_vamp_case(3000, 2000, 6, kind=1, variants=((3, TEAM2),), batch_rhs=4), ranks=2,
                           env={"VAMPOMI_CG_FOLD": "1"}),
    "ranks2_fold_off": dict(_vamp_case(3000, 2000, 6, kind=1, variants=((3, TEAM2),), batch_rhs=4), ranks=2,
                            env={"VAMPOMI_CG_FOLD": "0"}),
    "ranks2_batch_rhs3": dict(_vamp_case(3000, 2000, 6, kind=1, variants=((3, TEAM2),), batch_rhs=3), ranks=2),
}


@functools.lru_cache(maxsize=None)
def _problem(N, Mt, kind, binary):
    X, y, beta = make_problem(N, Mt, kind=kind)
    return X, ((y > 0).astype(np.float64) if binary else y), beta


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype=np.float64).tobytes()).hexdigest()


def _stats(d):
    st = d.stats()
    out = {f"{cls}_k": [getattr(st, cls + "_k")[k].launches for k in range(4)] for cls in ("ax", "atx", "op")}
    out.update(coll=st.coll.launches, host_syncs=st.host_syncs, a_passes_exec=st.a_passes_exec)
    return out


def _run_vamp(d, case):
    X, y, beta = _problem(case["N"], case["Mt"], case["kind"], case["model"] == "bin_class")
    d.load_meth(X[d.S:d.S + d.M])
    for which, value in case["variants"]:
        d.set_variant(which, value)
    d.set_phen(y, standardize=False)
    v = va.Vamp(d, va.VampOptions(model=case["model"], **case["opts"]), true_signal=beta[d.S:d.S + d.M])
    if case.get("step_after_stop"):
        _run_stepwise(d, v)
    else:
        v.infere(keep_hist=True)
    s = v.summary()
    n = s["iterations"]
    out = _stats(d)
    out.update(cg_iters=s["cg_iters"], ons_iters=s["ons_iters"], prestep_counts=list(d.prestep_counts()))
    if case.get("tail"):  # what the iteration's tail forms (tests/test_gpu_vamp_schedule.py)
        out.update(iterations=n, L=s["L"], params=_sha(s["params"]), metrics=_sha(s["metrics"]))
    return out, v.x1_hist[:n, :d.M].copy(), v.r1_hist[:n, :d.M].copy()


def _run_stepwise(d, v):
    """The run through the step-wise API; once it has stopped, one more step
    reports stopped and queues, waits for and counts nothing."""
    def counters():
        return dict(_stats(d), iterations=v.iterations_run, a_passes=v.a_passes, prestep=d.prestep_counts())

    v.begin(keep_hist=True)
    while not v.step():
        pass
    before = counters()
    assert v.step() is True
    assert counters() == before
    v.end()


def _run_pcg(d, case):
    """vampomi_pcg on exactly representable vectors (no generator in between)."""
    Mt = case["Mt"]
    X, _, _ = _problem(case["N"], Mt, 0, False)
    d.load_meth(X)
    i = np.arange(Mt)
    v = ((i * 37) % 101 - 50) / 64.0
    mu0 = ((i * 53) % 89 - 44) / 1024.0 if case["warm"] else None
    mu, it = d.pcg(v, 1.7, 0.4, mu0=mu0, onsager=case["onsager"], tol=1e-9, max_iter=200)
    out = _stats(d)
    out.update(cg_iters=[it], mu=_sha(mu))
    return out


def run_case(name, monkeypatch, cases=None):
    """What the fixture holds for one case (of CASES, or of cases), from one run."""
    case = (CASES if cases is None else cases)[name]
    for k, val in case.get("env", {}).items():
        if val is None:
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, val)
    if case["run"] == "pcg":
        with va.Data(case["N"], case["Mt"]) as d:
            return _run_pcg(d, case)
    if case.get("ranks", 1) == 1:
        with va.Data(case["N"], case["Mt"]) as d:
            out, x1, r1 = _run_vamp(d, case)
    else:  # rank 0's schedule, the gathered histories
        parts = run_ranks(monkeypatch, case["ranks"], case["N"], case["Mt"], lambda r, d: _run_vamp(d, case))
        out = parts[0][0]
        x1, r1 = (np.concatenate([p[j] for p in parts], axis=1) for j in (1, 2))
    out.update(x1_hist=_sha(x1), r1_hist=_sha(r1))
    return out


@functools.lru_cache(maxsize=None)
def _fixture():
    with open(FIXTURE) as f:
        return json.load(f)


@pytest.mark.parametrize("name", sorted(CASES))
def test_pcg_schedule_and_bits(monkeypatch, name):
    want = _fixture()[name]
    got = run_case(name, monkeypatch)
    print(name, json.dumps(got))
    assert sorted(got) == sorted(want)
    for key in sorted(want):
        assert got[key] == want[key], (name, key)


def test_fixture_covers_the_branches():
    """The recorded schedules show each branch live: the operator ran where the
    one-pass form is meant, pre-steps were made and used where forced on and
    none elsewhere, and the solves were cut at CG_max_iter."""
    f = _fixture()
    assert sorted(f) == sorted(CASES)
    assert sum(f["linear_batch_rhs4"]["op_k"]) > 0 and sum(f["linear_batch_rhs3"]["op_k"]) == 0
    for name in ("team_prestep_on", "t1_prestep_on"):
        assert min(f[name]["prestep_counts"]) >= 1, name
    for name in ("team_prestep_off", "team_headstart_off", "linear_batch_rhs4", "ranks2_fold_on"):
        assert f[name]["prestep_counts"] == [0, 0], name
    assert f["team_prestep_on"]["a_passes_exec"] < f["team_prestep_off"]["a_passes_exec"]
    assert f["team_prestep_off"]["a_passes_exec"] < f["team_headstart_off"]["a_passes_exec"]
    for n in (1, 2):
        assert max(f[f"cg_max_iter{n}"]["cg_iters"] + f[f"cg_max_iter{n}"]["ons_iters"]) == n
    assert f["ranks2_fold_on"]["x1_hist"] == f["ranks2_fold_off"]["x1_hist"]
    assert sum(f["probit_batch_rhs4"]["op_k"]) > 0 and sum(f["probit_batch_rhs1"]["op_k"]) == 0
