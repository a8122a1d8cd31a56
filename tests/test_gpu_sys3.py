"""Operator launches with a third system (kernels.h kOpSys, atax_team.hip).

One launch carries the two CG systems of a K = 2 launch and, in a third slot,
the alternate system of OpAlt: diag = tau = 1, gam2 = 0, no direction update,

    d_3 = A^T ar3,   A d_3,

with A = (X - mave) * msig / sqrt(N).  It runs on its own team plan (team sizes
2..16: the hand-off wave sums three systems in groups of 16 lanes), chosen
beside the context's plan.  Checked here against numpy on explicit matrices
at the bar of tests/test_gpu_operator.py (norm-relative 1e-12: every sum is
fp64 over at most N = 5001 or M = 700 terms of size one, an error near
sqrt(n) * 2^-53 = 1e-14), on odd N, on a last member's tile of 5 rows (less
than one wave's 128), with one to three loads per lane, for team sizes 2 and
4; the third slot's results must not depend on what the other two slots
carry, and every result is bitwise repeatable and the same under the narrow
storages of X.

Every kind of plan the default rule can select (team sizes 2, 4, 8, 16;
configuration 2 at S <= 3, configuration 4 at S = 4) is launched at the
smallest N that reaches it, at three marker counts (fewer markers than teams,
fewer columns per team than the pipeline's lag, more than one round of the
ring), against the same formulas evaluated in np.longdouble (64-bit mantissa)
and rounded to double at the end.  The bars are the same: relerr < 1e-12 on d
and A d of all three systems, rtol 1e-12 on <d,p>.  The sums are fp64 over at
most N = 43009 or M = 1541 terms: sqrt(n) * 2^-53 = 2e-14.
observed on one MI355X, the worst over the three marker counts and both forms
(norm-relative error of d and A d; relative error of <d,p>):
    N       variant  (T, S, cfg)   d, A d    <d,p>
    901     1802     (8, 1, 2)     1.7e-15   1.2e-15
    1925    2602     (16, 1, 2)    3.0e-15   7.8e-16
    5377    1204     (2, 4, 4)     6.7e-15   1.1e-15
    10753   -1       (4, 4, 4)     1.4e-14   3.1e-15
    14337   -1       (8, 3, 2)     2.0e-14   2.4e-14
    21505   -1       (8, 4, 4)     4.1e-14   1.9e-13
    28801   -1       (16, 3, 2)    6.4e-14   1.7e-14
    43009   -1       (16, 4, 4)    6.7e-14   2.2e-14
    7169    1205     (4, 3, 2)     8.9e-15   1.4e-15
    9217    -1       (4, 3, 2)     1.6e-14   4.3e-15
(1.9e-13 is a fused <d,p> of 7 markers that cancels, -0.33 from terms summing
to 4.2 in magnitude: 13 times the error of its d; numpy's own fp64 evaluation
is 1.8e-14 off there.)

2-system and 3-system launches alternating on one context whose plans differ
in team size (test_alternating_...) meet the same bars and give the bits of
the same call made first on a fresh context.  observed: d, A d 8.6e-15 and
<d,p> 5.8e-16 at N = 7169, 1.2e-14 and 5.4e-16 at N = 9217.

The CPU tests pin the plan's rules and its LDS layout (tm_lds, the one
source) on every selectable team plan, and sweep the rule over every N
against a restatement written from the constants.
"""
import ctypes as C

import numpy as np
import pytest

from conftest import relerr

va = pytest.importorskip("vampomi_amd")
from oracle import pyoracle as O  # noqa: E402  (checker: the generator and marker statistics)

lib = va.load()
LDS_MAX_DOUBLES = 160 * 1024 // 8


def plan3(N, M=62500, cus=256, variant=-1):
    T, S, TR, grid, cfg = (C.c_int() for _ in range(5))
    ns = C.c_int64()
    name = C.create_string_buffer(128)
    lds = (C.c_int64 * 6)()
    if lib.vampomi_dev_op3_plan(N, M, cus, variant, C.byref(T), C.byref(S), C.byref(TR), C.byref(grid), C.byref(cfg),
                                C.byref(ns), name, 128, lds) != 0:
        return None
    return dict(T=T.value, S=S.value, TR=TR.value, grid=grid.value, cfg=cfg.value, nslots=ns.value,
                name=name.value.decode(), lds=dict(zip(("head", "q", "qs", "part", "tot", "words"), list(lds))))


def plan2(N, M=62500, cus=256, variant=-1):
    T, S, TR, grid = (C.c_int() for _ in range(4))
    ns = C.c_int64()
    if lib.vampomi_dev_op_plan(N, M, cus, variant, 2, C.byref(T), C.byref(S), C.byref(TR), C.byref(grid), C.byref(ns),
                               None, 0) != 0:
        return None
    return dict(T=T.value, S=S.value, TR=TR.value, grid=grid.value)


# ---- CPU: the plan and its LDS layout --------------------------------------------------------------------------

# The rule restated from the constants alone (none of it read from the library).  A hand-off wave leaves 7
# streaming waves of 128 rows each: 896 rows per load step; without a hand-off (T = 1) 8 waves: 1024.  Tiles lie
# on 128-row boundaries, every member holds rows, and the loads per lane are bounded per configuration.
STEP, STEP1, TILE = 896, 1024, 128
MAIN_MAXS = {2: 4, 3: 4, 4: 5, 5: 6, 6: 4}  # the team configurations (with a hand-off) and their K = 2 bounds
SYS3_MAXS = ((2, 3), (4, 4))                # the 3-system kernel's, in the order they are tried
VARIANTS = [0] + [T * 10 + c for T in (1, 2, 4, 8, 16, 32) for c in range(7)] + [-1]


def _team(N, T, maxS):
    """(TR, S) of a team of T whose members' rows fit maxS loads per lane, or None."""
    TR = -(-(-(-N // T)) // TILE) * TILE
    S = -(-TR // STEP)
    return (TR, S) if (T - 1) * TR < N and S <= maxS else None


def _main_T(N, v):
    """The main plan's team size where it is a team (T >= 2), else None."""
    if v == -1:
        if N <= 9 * STEP1:  # whole columns in one workgroup, up to nine loads per lane
            return None
        if _team(N, 2, MAIN_MAXS[5]):  # just past it: a team of 2 under configuration 5
            return 2
        for cfg in (2, 4):
            for T in (2, 4, 8, 16, 32):
                if _team(N, T, MAIN_MAXS[cfg]):
                    return T
        return None
    if v <= 0:
        return None
    T, cfg = (divmod(v - 1000, 100) if v >= 1000 else divmod(v, 10))
    if T < 2 or T > 32 or T & (T - 1) or cfg not in MAIN_MAXS or not _team(N, T, MAIN_MAXS[cfg]):
        return None
    return T


def _rule3(N, v):
    """(T, S, cfg) of the 3-system plan beside variant v's plan at N, or None."""
    T = _main_T(N, v)
    while T is not None and T <= 16:
        for cfg, maxS in SYS3_MAXS:
            t = _team(N, T, maxS)
            if t:
                return T, t[1], cfg
        T *= 2
    return None


def _check_plan3(N, v, m, p):
    """The invariants of a 3-system plan p beside the main plan m."""
    T, S, TR = p["T"], p["S"], p["TR"]
    assert m["T"] <= T <= 16 and T & (T - 1) == 0
    assert (T - 1) * TR < N <= T * TR and TR % 128 == 0
    assert p["cfg"] in (2, 4) and 1 <= S <= (3 if p["cfg"] == 2 else 4) and S * 896 >= min(TR, N)
    assert p["grid"] % (8 * T) == 0 and p["grid"] <= 256 and p["nslots"] == p["grid"] // T
    lay = p["lds"]
    assert lay["head"] >= 3 and lay["q"] == lay["head"]
    assert lay["qs"] >= min(TR, N) and lay["qs"] % 2 == 0
    assert lay["part"] == lay["q"] + 3 * lay["qs"]
    assert lay["tot"] == lay["part"] + 2 * 7 * 3
    assert lay["words"] == lay["tot"] + 2 * 3 <= LDS_MAX_DOUBLES, (N, v, lay)


def test_sys3_plan_of_the_flagship_shape():
    """C2 (N = 10,000): the 2-system plan stays the team of 2 with six loads per
    lane; three accumulator sets fit a team of 4 with three."""
    assert plan2(10000, 50000)["T"] == 2 and plan2(10000, 50000)["S"] == 6
    p = plan3(10000, 50000)
    assert (p["T"], p["S"], p["TR"], p["cfg"], p["grid"], p["nslots"]) == (4, 3, 2560, 2, 256, 64)
    assert p["name"] == "atax_team_kernel<3, 3, 4, 5, 2, true, 2>"


def test_sys3_plan_rules_and_lds_layout_every_selectable_plan():
    """Beside every team plan any variant selects: no 3-system plan for whole
    columns and T = 1; else a team of the main plan's size or larger, at most
    16, every member holding rows, S within what the registers hold (3 loads
    per lane for configuration 2, 4 for configuration 4), and the one LDS
    layout with K = 3: head, q's three strides, the [2][7][3] wave partials,
    the [2][3] totals, disjoint, in order, inside 160 KiB.  A plan exists
    exactly where the restated rule (_rule3) has one, and is that one."""
    seen = 0
    for v in VARIANTS:
        for N in (1, 7, 133, 1000, 1541, 4097, 9216, 9217, 10000, 10752, 10753, 20000, 50000, 50001, 57344, 57345,
                  100000, 143360):
            m, p = plan2(N, variant=v), plan3(N, variant=v)
            if m is None or m["T"] < 2:
                assert p is None, (N, v)
                continue
            want = _rule3(N, v)
            if p is None:  # no team of main.T .. 16 holds the rows in <= 4 loads per lane
                assert want is None, (N, v, m, want)
                continue
            assert (p["T"], p["S"], p["cfg"]) == want, (N, v, p, want)
            seen += 1
            _check_plan3(N, v, m, p)
    assert seen > 60


def test_sys3_plan_sweep_of_every_N_against_the_restated_rule():
    """Every N up to 60,000 under the default variant and up to 12,000 under
    every variant of the test above: a 3-system plan exists exactly where the
    restated rule has one, with its (T, S, cfg), and holds the invariants.

    The default's breakpoints are pinned.  Among them the hole at
    28,673 <= N <= 28,800: the main plan is a team of 8 under configuration 4
    with five loads per lane, one more than a third accumulator set leaves
    room for, and a team of 16 would have tiles of 1920 rows, 15 of which
    already hold every row (15 * 1920 = 28,800 >= N): no 3-system plan."""
    T, S, TR, grid, cfg, T2 = (C.c_int() for _ in range(6))
    ns = C.c_int64()
    lds = (C.c_int64 * 6)()
    a3 = tuple(C.byref(x) for x in (T, S, TR, grid, cfg, ns))
    a2 = C.byref(T2)

    def both(N, v):
        m = dict(T=T2.value) if lib.vampomi_dev_op_plan(N, 62500, 256, v, 2, a2, None, None, None, None, None, 0) == 0 \
            else None
        if lib.vampomi_dev_op3_plan(N, 62500, 256, v, *a3, None, 0, lds) != 0:
            return m, None
        return m, dict(T=T.value, S=S.value, TR=TR.value, grid=grid.value, cfg=cfg.value, nslots=ns.value,
                       lds=dict(zip(("head", "q", "qs", "part", "tot", "words"), list(lds))))

    plans, seen = {}, 0
    for v in VARIANTS:
        for N in range(1, (60000 if v == -1 else 12000) + 1):
            m, p = both(N, v)
            want = _rule3(N, v)
            if p is None:
                assert want is None, (N, v, m, want)
                continue
            assert m is not None and (p["T"], p["S"], p["cfg"]) == want, (N, v, m, p, want)
            _check_plan3(N, v, m, p)
            seen += 1
            if v == -1:
                plans[N] = want
    assert seen > 100000
    steps = {N: plans.get(N) for N in range(2, 60001) if plans.get(N) != plans.get(N - 1)}
    assert steps == {9217: (4, 3, 2), 10753: (4, 4, 4), 14337: (8, 3, 2), 21505: (8, 4, 4), 28673: None,
                     28801: (16, 3, 2), 43009: (16, 4, 4), 57345: None}


# ---- GPU: one 3-system launch against numpy --------------------------------------------------------------------

def _centred(X, mave, dt=np.float64):
    return np.asarray(X, dtype=dt) - np.asarray(mave, dtype=dt)[:, None]


def _ref2(X, mave, msig, ar, qo, p, z, beta, diag, tau, gam2, dt=np.float64, Xc=None):
    """(dt = np.longdouble: the same formulas with every operand widened first, rounded to double at the end;
    Xc: _centred(X, mave, dt) where the caller has it already)"""
    msig, ar, qo, p, z, beta = (None if x is None else np.asarray(x, dtype=dt) for x in (msig, ar, qo, p, z, beta))
    N = X.shape[1]
    Xc = _centred(X, mave, dt) if Xc is None else Xc
    q = ar / diag
    pp = p.copy()
    if z is not None:
        q = q + beta[:, None] * qo
        pp = z + beta[:, None] * p
    t = (Xc @ q.T).T * msig[None, :] / np.sqrt(dt(N))
    d = tau * t + gam2 * pp
    ad = (Xc.T @ (msig[None, :] * d).T).T / np.sqrt(dt(N))
    return d.astype(np.float64), ad.astype(np.float64), np.sum(d * pp, axis=1).astype(np.float64)


def _ref3(X, mave, msig, ar3, dt=np.float64, Xc=None):
    msig, ar3 = (np.asarray(x, dtype=dt) for x in (msig, ar3))
    N = X.shape[1]
    Xc = _centred(X, mave, dt) if Xc is None else Xc
    d = (Xc @ ar3) * msig / np.sqrt(dt(N))
    return d.astype(np.float64), (Xc.T @ (msig * d) / np.sqrt(dt(N))).astype(np.float64)


# (N, Mt, main variant 1000 + 100 T + cfg, the 3-system plan's (T, S)):
# 1541 = 3 * 512 + 5: odd, the fourth member's tile is 5 rows; 133 = 128 + 5 the same for a team of 2;
# 5001: odd, three loads per lane for a team of 2, two for a team of 4; Mt is no multiple of the team count
SHAPES = [(1541, 700, 1404, (4, 1)), (1541, 700, 1202, (2, 1)), (133, 300, 1202, (2, 1)), (5001, 600, 1202, (2, 3)),
          (5001, 600, 1402, (4, 2))]


@pytest.fixture(scope="module")
def matrices():
    out = {}
    for N, Mt in sorted({s[:2] for s in SHAPES}):
        X = O.generate_markers(13, 1, N, 0, Mt)
        out[N, Mt] = (X,) + tuple(O.marker_stats(X))
    return out


def _launch_checks(d, X, mave, msig, pl, rng, dt=np.float64):
    """One context's 3-system launches against the reference in dt: unfused
    and fused, each twice (equal bits); the third slot's bits whatever the
    other two slots carry; the two CG systems against the 2-system launch.
    Returns the worst relative errors seen: of d and A d (norm-wise), and of <d,p>."""
    Mt, N = X.shape
    diag, tau, gam2 = 1.7, 0.9, 0.35
    ar, qo = rng.normal(size=(2, N)), rng.normal(size=(2, N))
    p, z = rng.normal(size=(2, Mt)), rng.normal(size=(2, Mt))
    beta = rng.uniform(0.1, 0.9, size=2)
    ar3, p3 = rng.normal(size=N), rng.normal(size=Mt)
    Xc = _centred(X, mave, dt)
    r3d, r3ad = _ref3(X, mave, msig, ar3, dt=dt, Xc=Xc)
    third, worst, worst_dp = [], 0.0, 0.0
    for fused in (False, True):
        zz, qq, bb = (z, qo, beta) if fused else (None, None, None)
        rd, rad, rdp = _ref2(X, mave, msig, ar, qq, p, zz, bb, diag, tau, gam2, dt=dt, Xc=Xc)
        gd, gad, gdp = d.op_apply3(ar, p, diag, tau, gam2, ar3, p3, z=zz, qo=qq, beta=bb)
        what = "%s fused=%d Mt=%d" % (pl["name"], fused, Mt)
        worst = max(worst, relerr(gd[:2], rd), relerr(gad[:2], rad), relerr(gd[2], r3d), relerr(gad[2], r3ad))
        worst_dp = max(worst_dp, float(np.max(np.abs(gdp - rdp) / np.abs(rdp))))
        assert relerr(gd[:2], rd) < 1e-12, (what, relerr(gd[:2], rd))
        assert relerr(gad[:2], rad) < 1e-12, (what, relerr(gad[:2], rad))
        assert np.allclose(gdp, rdp, rtol=1e-12, atol=0), (what, gdp, rdp)
        assert relerr(gd[2], r3d) < 1e-12, (what, relerr(gd[2], r3d))
        assert relerr(gad[2], r3ad) < 1e-12, (what, relerr(gad[2], r3ad))
        again = d.op_apply3(ar, p, diag, tau, gam2, ar3, p3, z=zz, qo=qq, beta=bb)
        for a, b in zip((gd, gad, gdp), again):
            assert np.array_equal(a, b), what  # bitwise repeatable
        third.append((gd[2].copy(), gad[2].copy()))
    # the third slot alone: a launch computes all three slots whatever the CgState says (only cg_update
    # ignores a stopped system's results), so at this level "stopped" is zeros in the other two slots; a
    # launch whose slot 0 system has stopped in the CgState runs in tests/test_gpu_prestep3.py
    # (test_mode3_cg_limits: the Onsager solve stops in its composed steps before step 0's launch)
    zd, zad, _ = d.op_apply3(np.zeros((2, N)), np.zeros((2, Mt)), diag, tau, gam2, ar3, p3)
    assert not zd[:2].any() and not zad[:2].any()
    third.append((zd[2], zad[2]))
    for td, tad in third[1:]:  # ... and its results do not depend on them
        assert np.array_equal(td, third[0][0]) and np.array_equal(tad, third[0][1])
    # the two CG systems against the 2-system launch of the same plan family: values, not bits
    # (the member sums pass through 16 lanes instead of 32: the same additions of the same members)
    k2 = d.op_apply(ar, p, diag, tau, gam2)
    k3 = d.op_apply3(ar, p, diag, tau, gam2, ar3, p3)
    assert relerr(k3[0][:2], k2[0]) < 1e-12 and relerr(k3[1][:2], k2[1]) < 1e-12
    return worst, worst_dp


@pytest.mark.gpu
@pytest.mark.parametrize("N,Mt,variant,ts", SHAPES, ids=lambda s: str(s).replace(" ", ""))
def test_sys3_launch_vs_numpy(matrices, N, Mt, variant, ts):
    X, mave, msig = matrices[N, Mt]
    rng = np.random.default_rng(N + variant)
    with va.Data(N, Mt) as d:
        d.load_meth(X)
        d.set_variant(3, variant)
        pl = plan3(N, Mt, variant=variant)  # (the device has 256 compute units)
        assert (pl["T"], pl["S"], pl["cfg"]) == ts + (2,), pl
        assert d.kernel_name(3, 3) == pl["name"]
        _launch_checks(d, X, mave, msig, pl, rng)


# ---- GPU: every kind of plan the default rule can select, against np.longdouble -----------------------------

# (N, main variant, the 3-system plan's (T, S, cfg), the main plan's (T, S, cfg) where the two differ in T);
# each N is the smallest that reaches its plan:
# 901 = 7 * 128 + 5 and 1925 = 15 * 128 + 5: the last member's tile is 5 rows, for teams of 8 and of 16 (every
# lane of a 16-lane group carries a member); 5377 = 2 * 3 * 896 + 1: odd, the first N with four loads per lane
# for a team of 2 (configuration 4); -1: the default's own breakpoints (the CPU sweep above); 43009: the last
# member's tile is 769 of 2816 rows; 7169 and 9217: the main plan is a team of 2 (configuration 5) and the
# 3-system plan a team of 4
PLANS = [(901, 1802, (8, 1, 2), None), (1925, 2602, (16, 1, 2), None), (5377, 1204, (2, 4, 4), None),
         (10753, -1, (4, 4, 4), None), (14337, -1, (8, 3, 2), None), (21505, -1, (8, 4, 4), None),
         (28801, -1, (16, 3, 2), None), (43009, -1, (16, 4, 4), None), (7169, 1205, (4, 3, 2), (2, 5, 5)),
         (9217, -1, (4, 3, 2), (2, 6, 5))]
# markers per launch by the 3-system plan's team count (teams take interleaved columns): fewer markers than
# teams (empty teams write zero slots), 3 or 4 columns per team (fewer than the lag of 5 or 4 steps), 12 or 13
# (more than one round of the ring of 10 or 7 columns, no multiple of the team count)
COUNTS = {"few": lambda nteams: 7, "lag": lambda nteams: 3 * nteams + 1, "ring": lambda nteams: 12 * nteams + 5}


def _nteams(N, variant):
    return 256 // _rule3(N, variant)[0]


@pytest.fixture(scope="module")
def plan_matrices():
    """N -> (X, mave, msig) with the most markers any test of N loads, generated once; a test loads the leading
    Mt markers (rows [:Mt] of the marker-major array)."""
    out = {}

    def get(N, variant):
        if N not in out:
            X = O.generate_markers(17, 1, N, 0, COUNTS["ring"](_nteams(N, variant)))
            out[N] = (X,) + tuple(O.marker_stats(X))
            for a in out[N]:
                a.setflags(write=False)
        return out[N]

    return get


# (F, L, P) of the team configurations as the kernel names carry them: <K, S, F, L, P, true, 2>
CFG_FLP = {2: (4, 5, 2), 4: (2, 4, 2), 5: (2, 3, 2)}


WORST = {}


@pytest.mark.gpu
@pytest.mark.parametrize("count", list(COUNTS))
@pytest.mark.parametrize("N,variant,ts,main", PLANS, ids=lambda s: str(s).replace(" ", ""))
def test_sys3_launch_every_default_plan_vs_longdouble(plan_matrices, N, variant, ts, main, count):
    Xall, mave, msig = plan_matrices(N, variant)
    Mt = COUNTS[count](256 // ts[0])
    X, mave, msig = Xall[:Mt], mave[:Mt], msig[:Mt]
    rng = np.random.default_rng(N + Mt)
    with va.Data(N, Mt) as d:
        d.load_meth(X)
        d.set_variant(3, variant)
        pl = plan3(N, Mt, variant=variant)
        assert (pl["T"], pl["S"], pl["cfg"]) == ts, pl
        assert pl["grid"] == 256 and pl["nslots"] == 256 // ts[0]
        assert d.kernel_name(3, 3) == pl["name"]
        if main:
            m = plan2(N, Mt, variant=variant)
            assert (m["T"], m["S"]) == main[:2], m
            assert d.kernel_name(3, 2) == "atax_team_kernel<2, %d, %d, %d, %d, true, 2>" % ((main[1],) + CFG_FLP[main[2]])
        worst = _launch_checks(d, X, mave, msig, pl, rng, dt=np.longdouble)
    key = "N=%d variant %d T=%d %s" % (N, variant, pl["T"], pl["name"])
    WORST[key] = tuple(max(a, b) for a, b in zip(WORST.get(key, (0.0, 0.0)), worst))
    print("\n%s Mt=%d: worst relerr d, A d %.2e <d,p> %.2e (over the counts so far %.2e %.2e)"
          % ((key, Mt) + worst + WORST[key]))


# (N, Mt, main variant): the first is the shape this test has always run; a team of 16 at one load per lane,
# configuration 4 at four loads per lane, and the default's team of 8 with fewer columns per team than the lag
NARROW = [(5001, 600, 1202), (1925, COUNTS["ring"](16), 2602), (5377, COUNTS["lag"](128), 1204),
          (14337, COUNTS["lag"](32), -1)]


@pytest.mark.gpu
@pytest.mark.parametrize("N,Mt,variant,storage",
                         [pytest.param(*s, st, id=st if s == NARROW[0] else "%d-%d-%d-%s" % (s + (st,)))
                          for s in NARROW for st in ("f32", "u16")])
def test_sys3_launch_narrow_storage_bitwise_equal_to_fp64_on_the_widened_matrix(matrices, plan_matrices, N, Mt,
                                                                                variant, storage):
    X = matrices[N, Mt][0] if (N, Mt) in matrices else plan_matrices(N, variant)[0][:Mt]
    rng = np.random.default_rng(7)
    ar, p = rng.normal(size=(2, N)), rng.normal(size=(2, Mt))
    ar3, p3 = rng.normal(size=N), rng.normal(size=Mt)
    with va.Data(N, Mt, storage=storage) as a, va.Data(N, Mt) as b:
        a.load_meth(X)
        b.load_meth(a.get_meth_data())
        for d in (a, b):
            d.set_variant(3, variant)
        assert a.kernel_name(3, 3) == b.kernel_name(3, 3).replace("atax_team_kernel<", "atax_team_kernel_%s<" % storage)
        assert b.kernel_name(3, 3) == plan3(N, Mt, variant=variant)["name"]
        ga = a.op_apply3(ar, p, 1.3, 0.8, 0.4, ar3, p3)
        gb = b.op_apply3(ar, p, 1.3, 0.8, 0.4, ar3, p3)
    for x, y in zip(ga, gb):
        assert np.array_equal(x, y)


# ---- GPU: 2-system and 3-system launches alternating on one context ------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("N,variant,ts,main", [s for s in PLANS if s[3]], ids=lambda s: str(s).replace(" ", ""))
def test_alternating_2_and_3_system_launches_on_plans_of_different_team_size(plan_matrices, N, variant, ts, main):
    """The main plan is a team of 2 (two words per member and column in the
    granule block) and the 3-system plan a team of 4 (K * T = 12 words per
    column in the same block): a granule one layout left behind, under an
    older tag, must never satisfy a poll of the other.  Each launch of the
    sequence meets the bars against np.longdouble and gives the bits of the
    same call made first on a fresh context."""
    Mt = COUNTS["ring"](256 // ts[0])
    Xall, mave, msig = plan_matrices(N, variant)
    X, mave, msig = Xall[:Mt], mave[:Mt], msig[:Mt]
    assert plan2(N, Mt, variant=variant)["T"] == main[0] != ts[0] == plan3(N, Mt, variant=variant)["T"]
    rng = np.random.default_rng(N)
    diag, tau, gam2 = 1.7, 0.9, 0.35

    def call(d, K, fused, ar, qo, p, z, beta, ar3, p3):
        kw = dict(z=z, qo=qo, beta=beta) if fused else {}
        return d.op_apply(ar, p, diag, tau, gam2, **kw) if K == 2 else d.op_apply3(ar, p, diag, tau, gam2, ar3, p3, **kw)

    calls = []
    for i, K in enumerate((2, 3, 2, 3, 3, 2)):  # (every other call in the fused form)
        calls.append((K, i % 2 == 1, rng.normal(size=(2, N)), rng.normal(size=(2, N)), rng.normal(size=(2, Mt)),
                      rng.normal(size=(2, Mt)), rng.uniform(0.1, 0.9, size=2), rng.normal(size=N), rng.normal(size=Mt)))
    worst, worst_dp, Xc = 0.0, 0.0, _centred(X, mave, np.longdouble)
    with va.Data(N, Mt) as d:
        d.load_meth(X)
        d.set_variant(3, variant)
        got = [call(d, *c) for c in calls]
    for i, (c, g) in enumerate(zip(calls, got)):
        K, fused, ar, qo, p, z, beta, ar3, p3 = c
        rd, rad, rdp = _ref2(X, mave, msig, ar, qo if fused else None, p, z if fused else None,
                             beta if fused else None, diag, tau, gam2, dt=np.longdouble, Xc=Xc)
        what = "call %d K=%d fused=%d" % (i, K, fused)
        errs = [relerr(g[0][:2], rd), relerr(g[1][:2], rad), float(np.max(np.abs(g[2] - rdp) / np.abs(rdp)))]
        assert np.allclose(g[2], rdp, rtol=1e-12, atol=0), (what, g[2], rdp)
        if K == 3:
            r3d, r3ad = _ref3(X, mave, msig, ar3, dt=np.longdouble, Xc=Xc)
            errs += [relerr(g[0][2], r3d), relerr(g[1][2], r3ad)]
        worst, worst_dp = max(worst, *(errs[:2] + errs[3:])), max(worst_dp, errs[2])
        assert max(errs[:2] + errs[3:]) < 1e-12, (what, errs)
        with va.Data(N, Mt) as f:  # the same call, first on its context
            f.load_meth(X)
            f.set_variant(3, variant)
            first = call(f, *c)
        for a, b in zip(g, first):
            assert np.array_equal(a, b), what
    print("\nalternating N=%d variant %d: worst relerr d, A d %.2e <d,p> %.2e" % (N, variant, worst, worst_dp))


@pytest.mark.gpu
def test_no_sys3_plan_is_an_error_not_a_fallback():
    """A T = 1 plan has no 3-system plan beside it: the launch is refused."""
    N, Mt = 1000, 200
    X = O.generate_markers(3, 0, N, 0, Mt)
    with va.Data(N, Mt) as d:
        d.load_meth(X)
        assert plan3(N, Mt) is None
        with pytest.raises(va.VampomiError):
            d.op_apply3(np.zeros((2, N)), np.zeros((2, Mt)), 1.0, 1.0, 0.0, np.ones(N), np.ones(Mt))
