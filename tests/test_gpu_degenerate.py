"""Degenerate markers on the GPU: constant, all but constant, duplicate and
collinear columns (tests/_degenerate.py), at the smallest shapes that reach
each code path, every N odd:

  301 x 517, 4099 x 333   the whole-column kernels
  12001 x 300             the team operator
  20001 x 160             ax_team_kernel

The tolerances are those of the existing tests of the same operation (1e-13
A.x and A^T.u, 1e-12 the operator, 1e-11 PCG with equal counts, 1e-10 with exact
integers for runs, tests/test_gpu_assoc.py's for LOO).  On top of them stand
the EXACT properties that do not depend on the order of any sum: at a dyadic
constant column mave == c, msig == 1, (x - mave) == 0, so A^T u is +-0 there, x
at such a marker cannot reach A.x whatever its size, d == gam2 * p, x1_hat == 0;
equal columns give equal bits; a narrow storage gives the bits of the fp64
context on the widened matrix; a row subset those of the plain context.

A kernel that scales before it centres passes every other GPU test and fails
here, at the non-dyadic constants, whose msig is ~1e14
(tests/test_degenerate_refs.py: the reference itself is not defined there, so
the device is held to numpy with the device's OWN statistics, not to the
oracle).  Checked on the device with two changed builds of the tile A.x kernel:
  acc += x * w - mave * w      fails test_nondyadic_constants (A.x off by ~1e-3
                               norm-relative) wherever the device's e is not 0;
                               the 1e30 test cannot see it: at a dyadic constant
                               x == mave bit for bit, so the two products cancel
  acc += x * w; acc -= mave * w  (the arithmetic of the GEMV shortcut) fails that
                               and the 1e30 test of every shape, and test mode
"""
import math
from types import SimpleNamespace

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

va = pytest.importorskip("vampomi_amd")
from conftest import relerr  # noqa: E402
import _degenerate as D  # noqa: E402
from _data import oracle_with_spread, sharded_oracle  # noqa: E402
from oracle import pyoracle as O  # noqa: E402  (checker)
from test_gpu_assoc import _check_loo, _estimate, _order_spread  # noqa: E402
from test_gpu_corners import pcg_numpy  # noqa: E402
from test_gpu_operator import _plans, _ref  # noqa: E402
from test_gpu_parity import _assert_parity  # noqa: E402
from test_gpu_probit import _assert_probit_parity  # noqa: E402
from test_gpu_sharded import _cat, _vamp, run_ranks  # noqa: E402

SMALL, COL, TEAM_OP, TEAM_AX = (301, 517), (4099, 333), (12001, 300), (20001, 160)
AX_VARIANTS = [-1] + list(range(8))  # the tuning table's 0-6, 7 = the team plan
ATX_VARIANTS = [-1] + list(range(8))
LOO_VARIANTS = list(range(20))
DEFAULTS = ((0, -1), (1, -1), (2, 16), (3, -1))


def _ids(s):
    return "N%d_M%d" % tuple(s[:2])


@pytest.fixture(scope="module")
def world():
    """(N, Mt, storage, nondyadic, alpha, widened) -> the planted problem in a
    context, made once and shared.  `widened`: an f64 context loaded with what
    the context of that narrow storage holds.  w.H is what the context holds,
    w.const / w.cval its constant columns (more than were planted where the
    storage rounds: u16 holds the 2^-30 entry as 0), w.mave / w.msig the
    oracle's statistics of w.H."""
    made = {}

    def get(N, Mt, storage="f64", nondyadic=False, alpha=1.0, widened=None):
        key = (N, Mt, storage, nondyadic, alpha, widened)
        if key not in made:
            X, idx = D.planted(N, Mt, nondyadic=nondyadic)
            if widened is not None:
                X = get(N, Mt, widened, nondyadic, alpha).H
            d = va.Data(N, Mt, alpha_scale=alpha, storage=storage)
            made[key] = w = SimpleNamespace(N=N, Mt=Mt, d=d, idx=idx, Xin=X, alpha=alpha)
            d.load_meth(X)
            w.H = d.get_meth_data()
            flat = np.nonzero(w.H.min(axis=1) == w.H.max(axis=1))[0]
            w.const = np.setdiff1d(flat, idx["nondyadic"])
            w.cval = w.H[w.const, 0]
            w.mask = np.zeros(Mt, dtype=bool)
            w.mask[w.const] = True
            w.mave, w.msig = O.marker_stats(w.H, alpha)
            w.y, w.beta = D.phen(D.planted(N, Mt)[0])  # one phenotype per shape, whatever the storage
            d.set_phen(w.y, standardize=False)
        return made[key]

    get.made = made
    yield get
    for w in made.values():
        w.d.close()


@pytest.fixture(autouse=True)
def _default_variants(world):
    """The shared contexts run their default kernels when a test starts, also after one that failed."""
    yield
    for w in world.made.values():
        for which, v in DEFAULTS:
            w.d.set_variant(which, v)


def _each(d, which, cands):
    """The variants of `cands` that exist for this context, each set in turn;
    the default is back afterwards, also when the body raised."""
    default = dict(DEFAULTS)[which]
    try:
        for v in cands:
            try:
                d.set_variant(which, v)
            except va.VampomiError:
                continue
            yield v
    finally:
        d.set_variant(which, default)


def _vectors(w, seed=1):
    """x (Mt) and u (N), x equal at the duplicates."""
    rng = np.random.default_rng(seed + w.N)
    x, u = rng.normal(size=w.Mt), rng.normal(size=w.N)
    x[w.idx["dup"]] = x[w.idx["dup"][0]]
    return x, u


def _np_ax(H, mave, msig, x):
    return ((H - mave[:, None]) * (msig * x)[:, None]).sum(axis=0) / math.sqrt(H.shape[1])


def _np_atx(H, mave, msig, u):
    return ((H - mave[:, None]) @ u) * msig / math.sqrt(H.shape[1])


def _same3(a):
    return np.array_equal(a[0], a[1]) and np.array_equal(a[0], a[2])


# ---- a. statistics ------------------------------------------------------------------
@pytest.mark.parametrize("alpha", [1.0, 0.7])
@pytest.mark.parametrize("storage", ["f64", "f32", "u16"])
@pytest.mark.parametrize("shape", [SMALL, COL], ids=_ids)
def test_statistics(world, shape, storage, alpha):
    w = world(*shape, storage, alpha=alpha)
    idx, N = w.idx, w.N
    mave, msig = w.d.get_mave(), w.d.get_msig()
    assert set(idx["const"].tolist()) <= set(w.const.tolist())
    assert np.array_equal(mave[w.const], w.cval), "mave == c, bit for bit"
    assert np.all(msig[w.const] == 1.0), "msig == 1, bit for bit"
    ones = idx["const"][idx["const_val"] == 1.0]
    if storage == "u16":
        assert np.all(w.H[ones] == 65535 / 65536)  # 1.0 is stored as 65535/65536
        assert np.array_equal(w.const, np.sort(np.append(idx["const"], idx["single"][4])))  # 2^-30 is held as 0
        own = np.count_nonzero(np.rint(np.delete(w.Xin, ones, axis=0) * 65536) > 65535)  # the generator's own 1.0s
        assert w.d.quant_stats()["clamped"] - own == N * len(ones) and len(ones) >= 5
    else:
        assert np.array_equal(w.const, idx["const"]) and np.array_equal(w.cval, idx["const_val"])
        assert w.d.quant_stats()["clamped"] == 0
    dup = idx["dup"]
    assert _same3(mave[dup]) and _same3(msig[dup])
    pl = np.concatenate([idx["plain"], dup])
    assert relerr(mave[pl], w.mave[pl]) < 1e-13 and relerr(msig[pl], w.msig[pl]) < 1e-13
    for m in np.setdiff1d(idx["single"], w.const):  # each on its own: one msig is ~1e9 sqrt(N)
        assert relerr(mave[[m]], w.mave[[m]]) < 1e-13 and relerr(msig[[m]], w.msig[[m]]) < 1e-13, m
    assert np.all(msig[~w.mask] != 1.0)


# ---- b. A.x and A^T.u ------------------------------------------------------------------
def _check_ax_atx(w, mave, msig):
    """Every variant of both tables against numpy on the explicit matrix with
    the statistics given, and the order-independent properties."""
    d, N = w.d, w.N
    x, u = _vectors(w)
    ax_ref, atx_ref = _np_ax(w.H, mave, msig, x), _np_atx(w.H, mave, msig, u)
    xb = x.copy()
    xb[w.const] *= 1e30
    names = {}
    for v in _each(d, 0, AX_VARIANTS):
        names[v] = d.kernel_name(0, 1)
        a = d.Ax(x)
        assert relerr(a, ax_ref) < 1e-13, ("ax", v, names[v], relerr(a, ax_ref))
        assert np.array_equal(d.Ax(xb), a), ("x at a constant marker reached A.x", v, names[v])
    assert set(range(7)) <= set(names)
    if N >= 20000:
        assert names[-1].startswith("ax_team_kernel<") and names[7].startswith("ax_team_kernel<"), names
    ran = []
    for v in _each(d, 1, ATX_VARIANTS):
        t = d.ATx(u)
        ran.append(v)
        assert relerr(t, atx_ref) < 1e-13, ("atx", v, relerr(t, atx_ref))
        assert _same3(t[w.idx["dup"]]), ("atx duplicates", v)
        assert np.all(t[w.const] == 0.0), ("atx at a constant", v, t[w.const])
    assert set(range(8)) <= set(ran)


@pytest.mark.parametrize("shape", [SMALL, COL, TEAM_AX], ids=_ids)
def test_ax_atx_every_variant(world, shape):
    """numpy is evaluated with the DEVICE's mave and msig: the operator is what
    is under test here, and the statistics meet the oracle's in
    test_statistics and below.  With the oracle's statistics numpy itself is
    1.7e-13 from the extended-precision A.x at 20001 x 160 (the oracle's
    sequential sums; the device, with its own, is 2.7e-15 from it), which
    leaves no room under the 1e-13 of this operation."""
    w = world(*shape)
    mave, msig = w.d.get_mave(), w.d.get_msig()
    pl = w.idx["plain"]
    assert relerr(mave[pl], w.mave[pl]) < 1e-13 and relerr(msig[pl], w.msig[pl]) < 1e-13
    _check_ax_atx(w, mave, msig)


def _run(d, y, beta, model="linear", its=8, **kw):
    d.set_phen(y, standardize=False)
    v = va.Vamp(d, va.VampOptions(model=model, max_iter=its, stop_criteria_thr=0.0, **kw), true_signal=beta)
    x1 = v.infere(keep_hist=True)
    s = v.summary()
    n = s["iterations"]
    s["x1_hist"], s["r1_hist"], s["x1_final"] = v.x1_hist[:n, :d.M].copy(), v.r1_hist[:n, :d.M].copy(), x1
    return s


def _zeros_stay(s, ref):
    z = ref["x1_hist"] == 0.0
    assert np.all(s["x1_hist"][z] == 0.0), "x1_hat is not +-0 where the oracle's is an exact zero"


@pytest.fixture(scope="module")
def oracle_runs():
    made = {}

    def get(w, model="linear", its=8):
        key = (w.N, w.Mt, model, its)
        if key not in made:
            y = (w.y > 0).astype(np.float64) if model == "bin_class" else w.y
            if model == "linear":
                made[key] = y, O.vamp_infere(w.H, y, w.Mt, true_signal=w.beta, max_iter=its, stop_criteria_thr=0.0), None
            else:
                ref, spread = oracle_with_spread(w.H, y, w.beta, w.Mt, max_iter=its, stop_criteria_thr=0.0,
                                                 model="bin_class")
                made[key] = y, ref, spread
        return made[key]

    return get


@pytest.mark.parametrize("shape", [SMALL, TEAM_AX], ids=_ids)
def test_batched_ax_every_variant(world, oracle_runs, shape):
    """A.x with 2-4 right-hand sides has no entry of its own: a run with
    batch_rhs = 4 launches it (tests/test_gpu_storage_u16.py), here under every
    A.x variant, 3 iterations at 20001 (the team plan's instantiations)."""
    w = world(*shape)
    its = 8 if shape == SMALL else 3
    y, ref, _ = oracle_runs(w, its=its)
    ran = []
    for v in _each(w.d, 0, AX_VARIANTS):
        s = _run(w.d, y, w.beta, its=its, batch_rhs=4)
        _assert_parity(s, ref)
        _zeros_stay(s, ref)
        ran.append(v)
    assert set(range(7)) <= set(ran) and (w.N < 20000 or 7 in ran)


# ---- c. the one-pass operator ------------------------------------------------------------
def _check_operator(w, mave, msig):
    d, N, Mt = w.d, w.N, w.Mt
    plans = _plans(d)
    assert plans, "no operator plan for N=%d" % N
    if N >= D.TEAM_N:
        assert any(v >= 10 for v in plans), plans  # tests/test_gpu_tiny.py relies on a team plan at 12000
    rng = np.random.default_rng(N)
    diag, tau, gam2 = 1.7, 0.9, 0.35
    dup, c = w.idx["dup"], w.const
    for K in (1, 2):
        ar, qo = rng.normal(size=(K, N)), rng.normal(size=(K, N))
        p, z = rng.normal(size=(K, Mt)), rng.normal(size=(K, Mt))
        p[:, dup], z[:, dup] = p[:, dup[:1]], z[:, dup[:1]]
        beta = rng.uniform(0.1, 0.9, size=K)
        pb = p.copy()
        pb[:, c] *= 1e30
        for fused in (False, True):
            zz, qq, bb = (z, qo, beta) if fused else (None, None, None)
            rd, rad, rdp = _ref(w.H, mave, msig, ar, qq, p, zz, bb, diag, tau, gam2)
            for v in _each(d, 3, plans):
                gd, gad, gdp = d.op_apply(ar, p, diag, tau, gam2, z=zz, qo=qq, beta=bb)
                what = "plan %d (%s) K=%d fused=%d" % (v, d.kernel_name(3, K), K, fused)
                assert relerr(gd, rd) < 1e-12, (what, relerr(gd, rd))
                assert relerr(gad, rad) < 1e-12, (what, relerr(gad, rad))
                assert np.allclose(gdp, rdp, rtol=1e-12, atol=0), (what, gdp, rdp)
                assert np.array_equal(gd[:, dup[0]], gd[:, dup[1]]) and np.array_equal(gd[:, dup[0]], gd[:, dup[2]]), what
                pp = z + beta[:, None] * p if fused else p
                assert np.array_equal(gd[:, c], gam2 * pp[:, c]), ("d != gam2 p at a constant", what)
                _, bad, _ = d.op_apply(ar, pb, diag, tau, gam2, z=zz, qo=qq, beta=bb)
                assert np.array_equal(bad, gad), ("p at a constant marker reached A d", what)


@pytest.mark.parametrize("shape", [COL, TEAM_OP], ids=_ids)
def test_operator_every_plan(world, shape):
    w = world(*shape)
    _check_operator(w, w.mave, w.msig)


# ---- d. lmmse_mult and pcg -----------------------------------------------------------------
@pytest.mark.parametrize("warm,onsager", [(False, False), (True, False), (False, True), (True, True)])
def test_lmmse_and_pcg(world, warm, onsager):
    w = world(*SMALL)
    d, Mt, c = w.d, w.Mt, w.const
    rng = np.random.default_rng(4)
    v = rng.normal(size=Mt)
    v[c[::2]] = 0.0
    mu0 = rng.normal(size=Mt) * 0.1 if warm else np.zeros(Mt)
    tau, gam2, tol = 1.7, 0.4, 1e-9

    def lmmse(t):
        return tau * O.atx(w.H, w.mave, w.msig, O.ax(w.H, w.mave, w.msig, t)) + gam2 * t

    g = d.lmmse_mult(v, tau, gam2)
    assert relerr(g, lmmse(v)) < 1e-13
    assert np.array_equal(g[c], gam2 * v[c]), "lmmse_mult at a constant is gam2 * v exactly"
    ref, its = pcg_numpy(w.H, w.mave, w.msig, v, mu0, tau, gam2, onsager, 200, tol)
    mu, it = d.pcg(v, tau, gam2, mu0=mu0 if warm else None, onsager=onsager, tol=tol, max_iter=200)
    assert it == its and 1 < it < 200
    assert relerr(mu, ref) < 1e-11
    # row m of the system at a constant is gam2 * mu_m = v_m: it holds as far as the solver went
    # (the residual the reference solution reached, plus the parity bar)
    reached = np.linalg.norm(v - lmmse(ref))
    assert np.all(np.abs(mu[c] - v[c] / gam2) <= 1.01 * reached / gam2 + 1e-11 * np.linalg.norm(ref))
    if not warm:
        assert np.all(mu[c[::2]] == 0.0), "v_m = 0 at a constant and a cold start: mu_m is exactly 0"


# ---- e. LOO ------------------------------------------------------------------------------
def _loo_problem(H, y, beta, dup=None):
    N = H.shape[1]
    est = _estimate(beta, N)
    if dup is not None:
        est[dup] = est[dup[0]]
    po, sto = O.assoc_loo(H, y, est)
    with np.errstate(invalid="ignore"):
        spread = _order_spread(H, y, est, po)
    return est, po, sto, spread


def _check_loo_nan(p, st, po, sto, spread, N):
    mask = np.isnan(po)
    assert np.array_equal(np.isnan(p), mask), np.nonzero(np.isnan(p) != mask)[0][:8]
    for q in range(5):
        assert relerr(st[:, q], sto[:, q]) < 1e-13, q  # every column
    ok = ~mask
    _check_loo(p[ok], st[ok], po[ok], sto[ok], spread[ok])
    D.nan_aware_pfun(p, st, N)


def test_loo_every_variant(world):
    w = world(*COL)
    d, dup = w.d, w.idx["dup"]
    d.set_phen(w.y, standardize=False)
    est, po, sto, spread = _loo_problem(w.H, w.y, w.beta, dup)
    assert np.array_equal(np.isnan(po), w.mask)
    ran = []
    for v in _each(d, 2, LOO_VARIANTS):
        p, st = d.assoc_loo(est)
        _check_loo_nan(p, st, po, sto, spread, w.N)
        assert _same3(st[dup]) and _same3(p[dup]), ("duplicates", v, d.kernel_name(2, 1, v))
        ran.append(v)
    assert ran == LOO_VARIANTS


def test_loo_all_but_two_columns_planted():
    N, Mt = 5, 7
    X = O.generate_markers(3, 1, N, 0, Mt)
    X[0], X[2], X[5], X[6] = 0.0, 1.0, 0.5, 0.25
    X[3] = 0.0
    X[3, N - 1] = 1.0
    y = O.standardize_phen(np.array([0.3, -1.1, 0.8, 2.0, -0.4]))
    est = np.array([0.1, -0.2, 0.3, 0.05, 0.0, -0.1, 0.2])
    po, sto = O.assoc_loo(X, y, est)
    with np.errstate(invalid="ignore"):
        spread = _order_spread(X, y, est, po)
    assert np.array_equal(np.isnan(po), [True, False, True, False, False, True, True])
    with va.Data(N, Mt) as d:
        d.load_meth(X)
        d.set_phen(y, standardize=False)
        for v in _each(d, 2, LOO_VARIANTS):
            p, st = d.assoc_loo(est)
            _check_loo_nan(p, st, po, sto, spread, N)


# ---- f. whole runs -----------------------------------------------------------------------
@pytest.mark.parametrize("shape", [SMALL, COL], ids=_ids)
def test_linear_run(world, oracle_runs, shape):
    w = world(*shape)
    y, ref, _ = oracle_runs(w)
    assert np.all(ref["x1_hist"][:, w.const] == 0.0)
    s = _run(w.d, y, w.beta)
    _assert_parity(s, ref)
    _zeros_stay(s, ref)


def test_probit_run(world, oracle_runs):
    w = world(*SMALL)
    y, ref, spread = oracle_runs(w, "bin_class", 4)
    assert np.all(ref["x1_hist"][:, w.const] == 0.0)
    s = _run(w.d, y, w.beta, model="bin_class", its=4)
    _assert_probit_parity(s, ref, spread)
    _zeros_stay(s, ref)


def test_two_rank_run_with_the_boundary_inside_constants(monkeypatch):
    """Two loopback ranks; eight more dyadic constants are planted around the
    shard boundary, so that each rank's shard ends or starts inside them."""
    N, Mt, its = SMALL[0], SMALL[1], 8
    X, idx = D.planted(N, Mt)
    S1 = O.divide_work(Mt, 2, 1)[1]
    X[S1 - 4:S1 + 4] = np.array(D.DYADIC + D.DYADIC[:3])[:, None]
    assert not set(range(S1 - 4, S1 + 4)) & set(np.concatenate([idx["single"], idx["dup"]]).tolist())
    y, beta = D.phen(X)
    kw = dict(max_iter=its, stop_criteria_thr=0.0)
    refs = sharded_oracle(X, y, beta, Mt, 2, **kw)
    ref_x1 = np.concatenate([r["x1_hist"] for r in refs], axis=1)
    const = np.concatenate([idx["const"], np.arange(S1 - 4, S1 + 4)])
    assert np.all(ref_x1[:, const] == 0.0)
    parts = run_ranks(monkeypatch, 2, N, Mt, lambda r, d: _vamp(d, X, y, beta, **kw))
    assert [p["S"] for p in parts] == [0, S1]
    for p in parts:
        assert p["cg_iters"] == refs[0]["cg_iters"].tolist() and p["ons_iters"] == refs[0]["ons_iters"].tolist()
        assert p["L"] == refs[0]["L"].tolist()
    x1 = _cat(parts, "x1_hist")
    for k in range(its):
        assert relerr(x1[k], ref_x1[k]) <= 1e-10, k
    assert np.all(x1[ref_x1 == 0.0] == 0.0)


# ---- g. storages ---------------------------------------------------------------------------
def _bundle(w):
    """Everything items a-e compute, under every variant and plan, by name."""
    d, N, Mt = w.d, w.N, w.Mt
    out = {"mave": d.get_mave(), "msig": d.get_msig()}
    x, u = _vectors(w)
    for v in _each(d, 0, AX_VARIANTS):
        out["ax", v] = d.Ax(x)
    for v in _each(d, 1, ATX_VARIANTS):
        out["atx", v] = d.ATx(u)
    rng = np.random.default_rng(N)
    ar, qo = rng.normal(size=(2, N)), rng.normal(size=(2, N))
    p, z = rng.normal(size=(2, Mt)), rng.normal(size=(2, Mt))
    beta = np.array([0.3, 0.6])
    for v in _each(d, 3, _plans(d)):
        for K in (1, 2):
            out["op", v, K, 0] = np.concatenate([a.ravel() for a in d.op_apply(ar[:K], p[:K], 1.7, 0.9, 0.35)])
            out["op", v, K, 1] = np.concatenate([a.ravel() for a in d.op_apply(ar[:K], p[:K], 1.7, 0.9, 0.35, z=z[:K],
                                                                                qo=qo[:K], beta=beta[:K])])
    out["lmmse"] = d.lmmse_mult(x, 1.7, 0.4)
    d.set_phen(w.y, standardize=False)
    for warm in (False, True):
        for ons in (False, True):
            mu, it = d.pcg(x, 1.7, 0.4, mu0=0.1 * p[0] if warm else None, onsager=ons, tol=1e-9, max_iter=200)
            out["pcg", warm, ons] = np.append(mu, it)
    est = _estimate(w.beta, N)
    for v in _each(d, 2, LOO_VARIANTS):
        pv, st = d.assoc_loo(est)
        out["loo", v] = np.concatenate([pv, st.ravel()])
    return out


@pytest.mark.parametrize("storage", ["f32", "u16"])
@pytest.mark.parametrize("shape", [SMALL, COL, TEAM_OP], ids=_ids)
def test_narrow_storage_bitwise_equals_f64_on_the_widened_matrix(world, shape, storage):
    a, b = world(*shape, storage), world(*shape, "f64", widened=storage)
    assert a.d.storage == storage and b.d.storage == "f64" and np.array_equal(a.H, b.H)
    assert not np.array_equal(a.H, a.Xin)  # the storage rounds
    ga, gb = _bundle(a), _bundle(b)
    assert ga.keys() == gb.keys() and len(ga) > 40
    for k in ga:
        assert np.array_equal(ga[k], gb[k], equal_nan=True), k


def test_two_values_on_one_u16_grid_point():
    """A column of two DIFFERENT generator values that share a k: constant to
    the u16 context, not to the f64 context on the original."""
    N, Mt = SMALL
    X, idx = D.planted(N, Mt)
    vals = np.unique(X[idx["plain"]])
    k = np.rint(vals * 65536)
    i = np.nonzero((k[1:] == k[:-1]) & (k[1:] < 65535))[0][0]
    a, b = vals[i], vals[i + 1]
    assert a != b
    col = idx["plain"][3]
    X[col] = np.where(np.arange(N) % 3 == 0, a, b)
    with va.Data(N, Mt, storage="u16") as d16, va.Data(N, Mt) as d64:
        d16.load_meth(X)
        d64.load_meth(X)
        assert d16.get_msig()[col] == 1.0 and d16.get_mave()[col] == k[i] / 65536
        assert d64.get_msig()[col] != 1.0 and d64.get_msig()[col] > 1e4
        u = np.random.default_rng(2).normal(size=N)
        assert d16.ATx(u)[col] == 0.0 and d64.ATx(u)[col] != 0.0


# ---- h. row subset -----------------------------------------------------------------------
@pytest.mark.parametrize("storage", ["f64", "u16"])
def test_row_subset_makes_a_column_constant(storage):
    """0.5 on the kept rows, generated on the dropped ones (kept rows 1, 3, ...,
    N_file = 2 N + 1): bit for bit the plain context on the file without those
    rows (tests/test_gpu_row_subset.py's bar), and constant to it."""
    N, Mt = 301, 77
    rows = np.arange(1, 2 * N + 1, 2, dtype=np.int64)
    F = O.generate_markers(3, 1, 2 * N + 1, 0, Mt)
    cols = np.array([0, 13, 16, 17, 76])
    F[np.ix_(cols, rows)] = 0.5
    assert np.all(np.ptp(F[cols], axis=1) > 0)
    Fk = np.ascontiguousarray(F[:, rows])
    y, beta = D.phen(Fk)
    est = _estimate(beta, N)
    rng = np.random.default_rng(6)
    x, u = rng.normal(size=Mt), rng.normal(size=N)
    got = []
    with va.Data(2 * N + 1, Mt, storage=storage, rows=rows) as d, va.Data(N, Mt, storage=storage) as p:
        d.load_meth(F)
        p.load_meth(Fk)
        for c in (d, p):
            c.set_phen(y, standardize=False)
            pv, st = c.assoc_loo(est)
            got.append({"meth": c.get_meth_data(), "mave": c.get_mave(), "msig": c.get_msig(), "ax": c.Ax(x),
                        "atx": c.ATx(u), "p": pv, "st": st, "r2": np.array(c.test_metrics(est))})
    a, b = got
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), k
    assert np.all(a["msig"][cols] == 1.0) and np.all(a["mave"][cols] == 0.5) and np.all(a["atx"][cols] == 0.0)
    assert np.array_equal(np.isnan(a["p"]), np.isin(np.arange(Mt), cols))


# ---- i. test mode ------------------------------------------------------------------------
def test_test_mode_with_markers_constant_in_the_test_set(world):
    """The test set's statistics are its own: markers that vary in training are
    constant in the planted test set, and their effects cannot reach the
    prediction."""
    w = world(*SMALL)
    w.d.set_phen(w.y, standardize=False)
    train = O.generate_markers(3, 1, w.N, 0, w.Mt)
    assert np.all(np.ptp(train[w.const[1:-1]], axis=1) > 0)
    rng = np.random.default_rng(8)
    est = w.beta * 0.9 / math.sqrt(w.N) + rng.normal(size=w.Mt) * 1e-3
    big = est.copy()
    big[w.const] = 1e3
    for s in (0.5, 1.0, 1.3):
        r2, c2 = w.d.test_metrics(est * s)
        ro, co = O.test_metrics(w.H, w.y, est * s)
        assert abs(r2 - ro) <= 1e-12 * max(1.0, abs(ro)) and abs(c2 - co) <= 1e-12 * abs(co)
        assert w.d.test_metrics(big * s) == (r2, c2)


# ---- j. non-dyadic constants: only what is defined -----------------------------------------
@pytest.mark.parametrize("shape", [SMALL, COL, TEAM_OP, TEAM_AX], ids=_ids)
def test_nondyadic_constants(world, shape):
    """0.3 and 0.7 in f64 storage.  The centring is exact (Sterbenz), so the
    standardised column is e = (c - mave) * msig at every row: 0, or
    +-sqrt((N-1)/N) up to the rounding of a sum of N equal terms.  The operators
    are held to numpy WITH THE DEVICE'S mave AND msig; with msig ~1e14 a kernel
    that scales before it centres is off by msig * 2^-53 * |x| ~ 1e-2 here."""
    w = world(*shape, nondyadic=True)
    d, N = w.d, w.N
    mave, msig = d.get_mave(), d.get_msig()
    for m, c in zip(w.idx["nondyadic"], D.NONDYADIC):
        e = (c - mave[m]) * msig[m]
        eo = (c - w.mave[m]) * w.msig[m]
        print(f"N={N} c={c}: device mave - c {mave[m] - c:+.3e} msig {msig[m]:.6e} e {e:+.9f}; "
              f"oracle mave - c {w.mave[m] - c:+.3e} msig {w.msig[m]:.6e} e {eo:+.9f}")
        r = math.sqrt((N - 1) / N)
        assert e == 0.0 or abs(abs(e) - r) <= N * 2.0 ** -53 * r, (c, e)
        assert (msig[m] == 1.0) == (e == 0.0)
    assert np.array_equal(mave[w.const], w.cval) and np.all(msig[w.const] == 1.0)
    _check_ax_atx(w, mave, msig)
    if shape in (COL, TEAM_OP):
        _check_operator(w, mave, msig)
    if shape == SMALL:
        s = _run(d, w.y, w.beta)
        assert s["iterations"] == 8
        for key in ("x1_hist", "r1_hist", "params"):
            assert np.all(np.isfinite(np.array(s[key]))), key
        assert np.all(s["x1_hist"][:, w.const] == 0.0)


# ---- the p-value at |t| = inf ----------------------------------------------------------------
@pytest.mark.parametrize("N", [64, 301, 4099])
def test_p_is_zero_where_y_is_a_column(N):
    """y_mark = +X[a] or -X[b] (raw values, est = 0): the five sums of that
    marker coincide, rxy = +-1 exactly, t = inf and p = 0 (the reference's
    Boost returns 0 there; before the fix of t_sf this was NaN)."""
    Mt, a, b = 40, 7, 33
    X = O.generate_markers(3, 1, N, 0, Mt)
    est = np.zeros(Mt)
    with va.Data(N, Mt) as d:
        d.load_meth(X)
        for m, sign in ((a, 1.0), (b, -1.0)):
            y = sign * X[m]
            d.set_phen(y, standardize=False)
            po, sto = O.assoc_loo(X, y, est)
            assert po[m] == 0.0
            with np.errstate(invalid="ignore"):
                spread = _order_spread(X, y, est, po)
            rest = np.arange(Mt) != m
            for v in _each(d, 2, (0, 16, 12)):
                name = d.kernel_name(2, 1, v)
                assert name.startswith("loo_wg_kernel") == (v != 0), name
                p, st = d.assoc_loo(est)
                assert p[m] == 0.0, (v, sign, p[m])
                assert np.all(np.isfinite(p)) and np.all(p[rest] > 0)
                _check_loo(p[rest], st[rest], po[rest], sto[rest], spread[rest])
                for q in range(5):
                    assert relerr(st[:, q], sto[:, q]) < 1e-13, q
                D.nan_aware_pfun(p, st, N)
