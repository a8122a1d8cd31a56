"""Mode 3 of the pre-step (pcg.cpp): two Onsager steps ahead.

Regular steps 0 and 1 of every solve are 3-system operator launches whose
third slot forms T1 = A^T A b, U1 = A T1 (step 0) and T2 = A^T A T1, U2 = A T2
(step 1) for the NEXT iteration's Onsager right-hand side b.  With J of them
in hand (J = 2 unless the previous solve ran a single regular step) that
iteration composes J steps of its Onsager solve without a pass over X, the
head-start pass carries step J + 1, and 1 + max(k1, k2 - 1 - J) passes are
executed.  Where no 3-system plan exists (T = 1 plans) the mode is mode 1.

The bars are those of tests/test_gpu_prestep.py (its helpers are used as they
are): on against off <= 1e-11 per iteration on x1 / r1, params at rtol 1e-11,
every CG, Onsager and mixture count equal, the oracle's parity at 1e-10; the
executed passes equal the rule simulated on the run's own counts.

Beside the teams of 2 and 4 the mode runs on every other kind of 3-system
plan: teams of 8 and of 16, configuration 4 with four loads per lane, and a
team of 4 beside a main plan that is a team of 2 (tests/test_gpu_sys3.py has
the single launches of the same plans).  observed, on against off, the worst
iteration: 4.9e-15 (team of 8, 30 iterations), 1.8e-15 (team of 16), 8.2e-16
(configuration 4, S = 4), 1.2e-15 (plans of different team size).
"""
import ctypes as C

import pytest

from test_gpu_prestep import (_assert_bitwise, _assert_close, _assert_parity, _oracle, _problem, _simulate)

va = pytest.importorskip("vampomi_amd")

T2, T4 = 1000 + 2 * 100 + 2, 1000 + 4 * 100 + 4  # operator plans forced through variant 3: teams of 2 and of 4
# teams of 8 and 16 (the 3-system plan is the same team under configuration 2, one load per lane), a team of 2
# under configuration 4 at N = 5377 (3-system plan: four loads per lane under configuration 4), and a team of
# 2 under configuration 5 at N = 7169, beside which the 3-system plan is a team of 4: steps 0 and 1 of every
# solve launch one plan and later steps the other, in every iteration
T8, T16, T2C4, T2C5 = 1000 + 8 * 100 + 2, 1000 + 16 * 100 + 2, 1000 + 2 * 100 + 4, 1000 + 2 * 100 + 5


def _has_plan3(N, Mt, opv):
    return va.load().vampomi_dev_op3_plan(N, Mt, 256, -1 if opv is None else opv, None, None, None, None, None, None,
                                          None, 0, None) == 0


def _plan3(N, Mt, opv):
    """(T, S, cfg) of the 3-system plan beside variant opv's."""
    T, S, cfg = (C.c_int() for _ in range(3))
    assert va.load().vampomi_dev_op3_plan(N, Mt, 256, opv, C.byref(T), C.byref(S), None, None, C.byref(cfg), None,
                                          None, 0, None) == 0
    return T.value, S.value, cfg.value


PLAN3 = {T8: (8, 1, 2), T16: (16, 1, 2), T2C4: (2, 4, 4), T2C5: (4, 3, 2)}  # at the shapes these variants run at


def _simulate3(cg, ons, max_iter):
    """Mode 3's executed passes and the pre-steps made / used, from the run's
    own CG (k1) and Onsager (k2) counts, and the largest J of an iteration.

    Iteration 1 has no head start: one A.x pass, then max(k1, k2) steps.  Later
    the head-start pass carries the Onsager solve's step J + 1, J = the
    pre-steps the previous iteration made, and max(k1, k2 - 1 - J) regular
    steps follow.  Regular steps 0 and 1 each make one pre-step (where a next
    iteration exists): an iteration makes min(2, its regular steps)."""
    passes = made = used = jmax = have = 0
    for i, (k1, k2) in enumerate(zip(cg, ons)):
        head = i > 0
        J = have if head else 0
        used += J
        jmax = max(jmax, J)
        regular = max(k1, k2 - (1 + J if head else 0))
        passes += 1 + regular
        have = min(2, regular) if i + 1 < max_iter else 0
        made += have
    return passes, made, used, jmax


# ---- CPU: the simulator against sequences worked by hand ----------------------------------------------------

def test_simulator_steady_state_takes_seven_passes():
    """(k1, k2) = (6, 9) in every iteration: 1 + max(6, 9) = 10 passes first,
    then J = 2: 1 + max(6, 9 - 3) = 7, against 8 with one pre-step
    (1 + max(6, 9 - 2)) and 9 without."""
    p, made, used, jmax = _simulate3([6] * 5, [9] * 5, 5)
    assert (p, made, used, jmax) == (10 + 4 * 7, 8, 8, 2)
    assert _simulate([6] * 5, [9] * 5, 5)[0] == 10 + 4 * 8
    assert _simulate([6] * 5, [9] * 5, 5, prestep=False)[0] == 10 + 4 * 9


def test_simulator_one_regular_step_leaves_one_prestep():
    """Iteration 2 runs one regular step (k1 = 1, the Onsager solve done in its
    composed and head steps): it makes one pre-step, so iteration 3 has J = 1:
    passes 1 + 5, then 1 + max(1, 3 - 3) = 2, then 1 + max(4, 6 - 2) = 5."""
    p, made, used, jmax = _simulate3([5, 1, 4], [4, 3, 6], 3)
    assert (p, made, used, jmax) == (6 + 2 + 5, 2 + 1 + 0, 0 + 2 + 1, 2)


def test_simulator_on_the_pinned_counts_of_the_first_shape():
    """tests/golden/pcg_schedule.json's counts at 3000 x 2000: 76 passes, 78
    under mode 1, 81 off (each + 1 for A^T y in a run's executed passes)."""
    k1, k2 = [7, 12, 7, 7, 7, 6, 5, 5, 5, 5], [7, 11, 7, 7, 8, 8, 7, 7, 7, 7]
    assert _simulate3(k1, k2, 10)[0] == 76
    assert _simulate(k1, k2, 10)[0] == 78
    assert _simulate(k1, k2, 10, prestep=False)[0] == 81


# ---- GPU -----------------------------------------------------------------------------------------------------

def _run(N, Mt, kind, prestep, opv, storage="f64", X=None, **kw):
    Xp, y, beta = _problem(N, Mt, kind)
    with va.Data(N, Mt, storage=storage) as d:
        d.load_meth(Xp if X is None else X)
        stored = d.get_meth_data() if storage != "f64" else None
        d.set_variant(7, prestep)
        if opv is not None:
            d.set_variant(3, opv)
        d.set_phen(y, standardize=False)
        v = va.Vamp(d, va.VampOptions(**kw), true_signal=beta)
        x1 = v.infere(keep_hist=True)
        s = v.summary()
        n = s["iterations"]
        s["x1_hist"] = v.x1_hist[:n, : d.M].copy()
        s["r1_hist"] = v.r1_hist[:n, : d.M].copy()
        s["x1_final"] = x1
        s["made"], s["used"] = d.prestep_counts()
        s["stored"] = stored
    return s


def _assert_schedule3(s, max_iter, plan3=True):
    if plan3:
        passes, made, used, jmax = _simulate3(s["cg_iters"], s["ons_iters"], max_iter)
    else:  # no 3-system plan: mode 1's slot rule
        passes, made, used = _simulate(s["cg_iters"], s["ons_iters"], max_iter)
        jmax = 1
    print("passes", s["a_passes_exec"] - 1, "simulated", passes, "made/used", s["made"], s["used"], "simulated", made,
          used, "k1", s["cg_iters"], "k2", s["ons_iters"])
    assert s["a_passes_exec"] == 1 + passes  # + A^T y
    assert (s["made"], s["used"]) == (made, used)
    return jmax


@pytest.mark.gpu
@pytest.mark.parametrize("N,Mt,its,kind,opv", [(3000, 2000, 10, 1, T2), (3000, 2000, 10, 1, T4),
                                                (4099, 3001, 12, 1, None), (4099, 3001, 12, 1, T2),
                                                (1000, 2000, 30, 0, None), (1000, 2000, 30, 0, T2),
                                                (1000, 2000, 30, 0, T4), (1000, 2000, 30, 0, T8),
                                                (2000, 1500, 12, 1, T16), (5377, 1200, 6, 1, T2C4),
                                                (7169, 1500, 6, 1, T2C5)])
def test_mode3_against_off_and_the_oracle(N, Mt, its, kind, opv):
    kw = dict(max_iter=its, stop_criteria_thr=0.0)
    plan3 = _has_plan3(N, Mt, opv)
    assert plan3 == (opv is not None)  # (the default plans of these shapes are T = 1)
    if opv in PLAN3:
        assert _plan3(N, Mt, opv) == PLAN3[opv]
    a = _run(N, Mt, kind, 3, opv, **kw)
    b = _run(N, Mt, kind, 0, opv, **kw)
    _assert_close(a, b)
    jmax = _assert_schedule3(a, its, plan3)
    assert jmax == (2 if plan3 else 1)  # two pre-steps used in some iteration: the mode is not idle
    assert a["a_passes_exec"] <= b["a_passes_exec"]
    _assert_parity(a, _oracle(N, Mt, kind, **kw))
    if (N, opv) == (3000, T2):  # the pinned fixture's counts: 76 + 1 passes, 79 under mode 1, 82 off
        assert a["cg_iters"] == [7, 12, 7, 7, 7, 6, 5, 5, 5, 5] and a["ons_iters"] == [7, 11, 7, 7, 8, 8, 7, 7, 7, 7]
        assert (a["a_passes_exec"], b["a_passes_exec"]) == (77, 82)
        assert _run(N, Mt, kind, 1, opv, **kw)["a_passes_exec"] == 79


@pytest.mark.gpu
@pytest.mark.parametrize("cgmax", [1, 2, 3, 4])
def test_mode3_cg_limits(cgmax):
    """Composed steps and the head step count towards CG_max_iter as own steps do."""
    N, Mt = 800, 1500
    kw = dict(max_iter=5, stop_criteria_thr=0.0, CG_max_iter=cgmax)
    a = _run(N, Mt, 0, 3, T2, **kw)
    b = _run(N, Mt, 0, 0, T2, **kw)
    assert a["cg_iters"] == b["cg_iters"] and a["ons_iters"] == b["ons_iters"]
    assert max(a["ons_iters"]) <= cgmax and max(a["cg_iters"]) <= cgmax
    _assert_close(a, b)
    _assert_schedule3(a, 5)
    assert a["used"] >= 1
    _assert_parity(a, _oracle(N, Mt, 0, **kw))


@pytest.mark.gpu
def test_mode3_early_stop():
    """The stop criterion fires: the last iteration's pre-steps are dropped."""
    N, Mt = 1500, 3001
    kw = dict(max_iter=40, stop_criteria_thr=1e-2)
    a = _run(N, Mt, "tail", 3, T2, **kw)
    b = _run(N, Mt, "tail", 0, T2, **kw)
    assert a["iterations"] < 40
    _assert_close(a, b)
    assert _assert_schedule3(a, 40) == 2
    assert a["made"] > a["used"]  # the last iteration's were never used
    _assert_parity(a, _oracle(N, Mt, "tail", **kw))


@pytest.mark.gpu
def test_mode3_repeatable(monkeypatch):
    for N, Mt, kind, opv in ((1000, 2000, 0, T2), (2000, 1500, 1, T16)):
        kw = dict(max_iter=12, stop_criteria_thr=0.0)
        monkeypatch.delenv("VAMPOMI_PRE_AHEAD", raising=False)
        a = _run(N, Mt, kind, 3, opv, **kw)
        b = _run(N, Mt, kind, 3, opv, **kw)
        _assert_bitwise(a, b)
        monkeypatch.setenv("VAMPOMI_PRE_AHEAD", "0")
        c = _run(N, Mt, kind, 3, opv, **kw)
        _assert_bitwise(a, c)
        assert a["used"] >= 2


@pytest.mark.gpu
def test_mode3_without_a_sys3_plan_is_mode1_bitwise():
    N, Mt, opv = 1000, 2000, 1000 + 1 * 100 + 0  # T = 1
    kw = dict(max_iter=8, stop_criteria_thr=0.0)
    assert not _has_plan3(N, Mt, opv)
    a = _run(N, Mt, 0, 3, opv, **kw)
    b = _run(N, Mt, 0, 1, opv, **kw)
    _assert_bitwise(a, b)
    assert a["used"] >= 1


@pytest.mark.gpu
@pytest.mark.parametrize("N,Mt,opv,storage", [pytest.param(800, 1500, T2, "f32", id="f32"),
                                              pytest.param(800, 1500, T2, "u16", id="u16"),
                                              pytest.param(2000, 1500, T16, "f32", id="2000-1500-2602-f32"),
                                              pytest.param(2000, 1500, T16, "u16", id="2000-1500-2602-u16")])
def test_mode3_narrow_storage_bitwise_equal_to_fp64_on_the_widened_matrix(N, Mt, opv, storage):
    # (the methylation-like design: values in [0, 1], which the 16-bit storage holds)
    kw = dict(max_iter=6, stop_criteria_thr=0.0)
    a = _run(N, Mt, 1, 3, opv, storage=storage, **kw)
    b = _run(N, Mt, 1, 3, opv, X=a["stored"], **kw)
    _assert_bitwise(a, b)
    assert a["used"] >= 2
