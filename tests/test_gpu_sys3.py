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

The CPU tests pin the plan's rules and its LDS layout (tm_lds, the one
source) on every selectable team plan.
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
    the [2][3] totals, disjoint, in order, inside 160 KiB."""
    seen = 0
    for v in [0] + [T * 10 + c for T in (1, 2, 4, 8, 16, 32) for c in range(7)] + [-1]:
        for N in (1, 7, 133, 1000, 1541, 4097, 9216, 9217, 10000, 10752, 10753, 20000, 50000, 50001, 57344, 57345,
                  100000, 143360):
            m, p = plan2(N, variant=v), plan3(N, variant=v)
            if m is None or m["T"] < 2:
                assert p is None, (N, v)
                continue
            if p is None:  # no team of main.T .. 16 holds the rows in <= 4 loads per lane
                assert m["T"] > 16 or N > 16 * 4 * 896 - 15 * 127, (N, v, m)
                continue
            seen += 1
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
    assert seen > 60


# ---- GPU: one 3-system launch against numpy --------------------------------------------------------------------

def _ref2(X, mave, msig, ar, qo, p, z, beta, diag, tau, gam2):
    N = X.shape[1]
    Xc = X - mave[:, None]
    q = ar / diag
    pp = p.copy()
    if z is not None:
        q = q + beta[:, None] * qo
        pp = z + beta[:, None] * p
    t = (Xc @ q.T).T * msig[None, :] / np.sqrt(N)
    d = tau * t + gam2 * pp
    ad = (Xc.T @ (msig[None, :] * d).T).T / np.sqrt(N)
    return d, ad, np.sum(d * pp, axis=1)


def _ref3(X, mave, msig, ar3):
    N = X.shape[1]
    Xc = X - mave[:, None]
    d = (Xc @ ar3) * msig / np.sqrt(N)
    return d, Xc.T @ (msig * d) / np.sqrt(N)


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


@pytest.mark.gpu
@pytest.mark.parametrize("N,Mt,variant,ts", SHAPES, ids=lambda s: str(s).replace(" ", ""))
def test_sys3_launch_vs_numpy(matrices, N, Mt, variant, ts):
    X, mave, msig = matrices[N, Mt]
    rng = np.random.default_rng(N + variant)
    diag, tau, gam2 = 1.7, 0.9, 0.35
    ar, qo = rng.normal(size=(2, N)), rng.normal(size=(2, N))
    p, z = rng.normal(size=(2, Mt)), rng.normal(size=(2, Mt))
    beta = rng.uniform(0.1, 0.9, size=2)
    ar3, p3 = rng.normal(size=N), rng.normal(size=Mt)
    r3d, r3ad = _ref3(X, mave, msig, ar3)
    with va.Data(N, Mt) as d:
        d.load_meth(X)
        d.set_variant(3, variant)
        pl = plan3(N, Mt, variant=variant)  # (the device has 256 compute units)
        assert (pl["T"], pl["S"]) == ts, pl
        assert d.kernel_name(3, 3) == pl["name"]
        third = []
        for fused in (False, True):
            zz, qq, bb = (z, qo, beta) if fused else (None, None, None)
            rd, rad, rdp = _ref2(X, mave, msig, ar, qq, p, zz, bb, diag, tau, gam2)
            gd, gad, gdp = d.op_apply3(ar, p, diag, tau, gam2, ar3, p3, z=zz, qo=qq, beta=bb)
            what = "%s fused=%d" % (pl["name"], fused)
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


@pytest.mark.gpu
@pytest.mark.parametrize("storage", ["f32", "u16"])
def test_sys3_launch_narrow_storage_bitwise_equal_to_fp64_on_the_widened_matrix(matrices, storage):
    N, Mt, variant = 5001, 600, 1202
    X = matrices[N, Mt][0]
    rng = np.random.default_rng(7)
    ar, p = rng.normal(size=(2, N)), rng.normal(size=(2, Mt))
    ar3, p3 = rng.normal(size=N), rng.normal(size=Mt)
    with va.Data(N, Mt, storage=storage) as a, va.Data(N, Mt) as b:
        a.load_meth(X)
        b.load_meth(a.get_meth_data())
        for d in (a, b):
            d.set_variant(3, variant)
        assert a.kernel_name(3, 3) == b.kernel_name(3, 3).replace("atax_team_kernel<", "atax_team_kernel_%s<" % storage)
        ga = a.op_apply3(ar, p, 1.3, 0.8, 0.4, ar3, p3)
        gb = b.op_apply3(ar, p, 1.3, 0.8, 0.4, ar3, p3)
    for x, y in zip(ga, gb):
        assert np.array_equal(x, y)


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
