"""The schedule and the bits of every branch of the linear VAMP iteration
(vampomi_vamp_step, vamp.cpp), pinned.

tests/golden/vamp_step_schedule.json holds, for each case below, what
tests/golden/pcg_schedule.json holds for its cases (the launches of every
class, the collectives, the host waits, the executed passes, the CG and
Onsager steps, the pre-steps, a SHA-256 of the x1_hat and r1 histories) and
what the iteration's tail forms beside them: the number of iterations run,
a SHA-256 of the float64 bytes of the params and metrics rows (gamw, alpha2
and the error measures: x1 and r1 alone would not see a wrong metric) and the
history of L.  tests/golden/make_vamp_step_schedule.py recorded it with the
commit before vampomi_vamp_step was split into its phases; a change to the
host side of the iteration that queues anything differently, waits once more
or moves one bit of a result fails here.  The fixture is never regenerated to
make this pass.

test_gpu_pcg_schedule.py pins batch_rhs 0-4 at the defaults (one EM round,
no delay, no early stop).  The cases here are the tail's other branches at
the smallest shapes at which each is live: 301 x 517 on the whole-column
operator (no head start) and, for the head start, T = 1 at 1000 x 2000 and
teams of 2 at 3000 x 2000 on two loopback ranks.  max_iter is 6, so the last
iteration (next false: nothing prefetched, nothing queued ahead) is a sixth
of every record."""
import functools
import json
import os

import pytest

import test_gpu_pcg_schedule as P

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vamp_step_schedule.json")
HASHES = ("x1_hist", "r1_hist", "params", "metrics")
# stop_criteria_thr of the early-stop cases, from the recorded commit's NMSE traces with the stop off
# (make_vamp_step_schedule.py --nmse): T1 0.111, 0.119, 0.047 at iterations 7, 8, 9 (stops at 9);
# 301 x 517, batch_rhs 2: 0.389, 0.113, 0.064 at iterations 6, 7, 8 (stops at 8)
STOP_T1, STOP_SMALL = 0.08, 0.09


def _case(N, Mt, its, kind=0, variants=(), extra=None, **opts):
    case = P._vamp_case(N, Mt, its, kind=kind, variants=variants)
    case["opts"].update(opts)  # (stop_criteria_thr is 0.0 unless the case says otherwise)
    return dict(case, tail=True, **(extra or {}))


def _small(its=6, **kw):  # the whole-column operator: no head start, so no start queued ahead
    return _case(301, 517, its, **kw)


def _t1(its=6, **kw):  # the head start and the pre-step live on one rank
    return _case(1000, 2000, its, variants=((3, P.T1), (7, 1)), **kw)


def _ranks2(extra=None, **kw):
    return _case(3000, 2000, 6, kind=1, variants=((3, P.TEAM2),), extra=dict(extra or {}, ranks=2), **kw)


CASES = {
    # several EM rounds: chain on, devem off (EM_max_iter != 1): the host's mixture update (em_finish) sits
    # between the EM sums and the denoising
    "em3_t1_batch_rhs4": _t1(batch_rhs=4, EM_max_iter=3),
    "em3_small_batch_rhs3": _small(batch_rhs=3, EM_max_iter=3),
    # no EM round: r1_in_em false (EM_max_iter < 1), so the host tail on an arec schedule, r1 by lincomb_div
    "em0_t1_batch_rhs4": _t1(batch_rhs=4, EM_max_iter=0),
    # delayed prior learning: em_next (it + 1 > learn_prior_delay) turns true at it = 3, so the tail changes
    # kind inside the run; batch_rhs 1 also skips the first iteration's update_prior (it > learn_prior_delay)
    "delay3_t1_batch_rhs4": _t1(batch_rhs=4, learn_prior_delay=3),
    "delay3_small_batch_rhs1": _small(batch_rhs=1, learn_prior_delay=3),
    # the start queued ahead (tail_plan: devem && R.pre_ahead_on, then ahead), off and on: the same bits, and
    # the same counters (the launch is the solve's own first launch, queued one iteration early)
    "ahead_off_t1_batch_rhs4": _t1(batch_rhs=4, extra=dict(env={"VAMPOMI_PRE_AHEAD": "0"})),
    "ahead_on_t1_batch_rhs4": _t1(batch_rhs=4, extra=dict(env={"VAMPOMI_PRE_AHEAD": None})),
    # early stop (thresholds from the recorded commit's own NMSE trace, between two iterations' values): the
    # prefetched denoising and the start queued ahead are discarded; then one more step through the step-wise
    # API reports stopped and moves no counter
    "stop_t1_batch_rhs4": _t1(12, batch_rhs=4, stop_criteria_thr=STOP_T1, extra=dict(step_after_stop=True)),
    "stop_small_batch_rhs2": _small(12, batch_rhs=2, stop_criteria_thr=STOP_SMALL, extra=dict(step_after_stop=True)),
    # two loopback ranks: the several-rank tail (mr: chain && c->use_comm; vk::tail_post after each all-reduce),
    # the same with the host waiting at each level, several EM rounds, and the !arec tail with collectives
    "ranks2_mr_tail_on": _ranks2(batch_rhs=4),
    "ranks2_mr_tail_off": _ranks2(batch_rhs=4, extra=dict(env={"VAMPOMI_MR_TAIL": "0"})),
    "ranks2_em3": _ranks2(batch_rhs=4, EM_max_iter=3),
    "ranks2_batch_rhs1": _ranks2(batch_rhs=1),
    # the unfused form: two separate solves, nothing prefetched (next false throughout), several EM rounds
    "em3_small_batch_rhs0": _small(batch_rhs=0, EM_max_iter=3),
}


@functools.lru_cache(maxsize=None)
def _fixture():
    with open(FIXTURE) as f:
        return json.load(f)


@pytest.mark.parametrize("name", sorted(CASES))
def test_vamp_step_schedule_and_bits(monkeypatch, name):
    want = _fixture()[name]
    got = P.run_case(name, monkeypatch, CASES)
    print(name, json.dumps(got))
    assert sorted(got) == sorted(want)
    for key in sorted(want):
        assert got[key] == want[key], (name, key)


def test_fixture_covers_the_branches():
    """What the records themselves show: every case recorded with every hash,
    the pairs that differ in schedule only equal in their bits, the early
    stops early, no collective launch on one rank, and the several-rank tail
    with fewer host waits than the host tail on the same run."""
    f = _fixture()
    assert sorted(f) == sorted(CASES)
    for name, rec in f.items():
        assert all(k in rec for k in HASHES + ("iterations", "L", "host_syncs", "coll")), name
        # (loopback ranks reduce through shared memory, which the collectives' launch counter does not see)
        assert rec["coll"] == 0 or CASES[name].get("ranks", 1) > 1, name
        stops = CASES[name].get("step_after_stop", False)
        its = CASES[name]["opts"]["max_iter"]
        assert (3 <= rec["iterations"] < its) if stops else rec["iterations"] == its, name
        assert len(rec["L"]) == len(rec["cg_iters"]) == rec["iterations"], name
    for a, b in (("ahead_off_t1_batch_rhs4", "ahead_on_t1_batch_rhs4"), ("ranks2_mr_tail_off", "ranks2_mr_tail_on")):
        for k in HASHES:
            assert f[a][k] == f[b][k], (a, b, k)
    # the host waiting at each level of the tail, against once at its end (the same CG steps in both)
    assert f["ranks2_mr_tail_off"]["cg_iters"] == f["ranks2_mr_tail_on"]["cg_iters"]
    assert f["ranks2_mr_tail_off"]["host_syncs"] > f["ranks2_mr_tail_on"]["host_syncs"]
    # no EM round: the mixture never changes
    assert set(f["em0_t1_batch_rhs4"]["L"]) == {10}
    # the head start and the pre-step live where the start is queued ahead; no operator launch below batch_rhs 4
    assert min(f["ahead_on_t1_batch_rhs4"]["prestep_counts"]) >= 1
    for name in ("em3_small_batch_rhs3", "delay3_small_batch_rhs1", "stop_small_batch_rhs2", "em3_small_batch_rhs0",
                 "ranks2_batch_rhs1"):
        assert sum(f[name]["op_k"]) == 0, name
    # the delay: no EM update before iteration 3, so the mixture keeps its components until then
    assert len(set(f["delay3_t1_batch_rhs4"]["L"][:3])) == 1
