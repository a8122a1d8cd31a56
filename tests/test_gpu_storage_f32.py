"""fp32 storage of the methylation shard (VAMPOMI_STORE_F32) on the device.

The storage changes one thing, the rounding of X at ingest: an fp32 lane owns
the same rows as the fp64 lane of the same plan and widens what it loads, so
every sum runs in the same order.  Hence the bar of this file: an F32 context
gives, BIT FOR BIT, what an F64 context gives on the widened copy of the same
stored matrix, for the operators under every plan, for whole runs, and for the
association and test modes.  One run is also held to the CPU oracle on the
rounded matrix (the project's 1e-10), which ties the new path to the checker
and not only to the fp64 engine.

Shapes (small; chosen for the code paths, cus = 256 plans):
  (1001, 517)   odd N with a pad row, the reference pin's shape, team size 1
  (9217, 300)   just past the 9216 rows of the default one-workgroup plan: the team of 2
  (20001, 131)  teams of 8-32, a short last tile, M no multiple of the team count
  (20001, 7)    fewer markers than teams: empty teams
  (7001, 150)   under plan 22 its head-start launch is configuration 3
"""
import ctypes as C
import os
import subprocess
import threading
import time

import numpy as np
import pytest

from conftest import relerr

pytestmark = pytest.mark.gpu

va = pytest.importorskip("vampomi_amd")
from oracle import pyoracle as O  # noqa: E402  (checker)

SHAPES = [(1001, 517), (9217, 300), (20001, 131), (20001, 7)]
CANDIDATES = [0] + [T * 10 + c for T in (1, 2, 4, 8, 16, 32) for c in range(7)]  # tests/test_gpu_operator.py
CUS = 256


def widened(X):
    return X.astype(np.float32).astype(np.float64)


def matrix(N, Mt, seed=11):
    """Methylation-like values with full fp64 mantissas (most are not floats)."""
    return O.generate_markers(seed, 1, N, 0, Mt)


def _op_plan(N, M, variant):
    T, S = C.c_int(), C.c_int()
    name = C.create_string_buffer(256)
    st = va.load().vampomi_dev_op_plan(N, M, CUS, variant, 1, C.byref(T), C.byref(S), None, None, None, name, 256)
    return None if st else (T.value, S.value, name.value.decode())


def test_production_plans_exist_at_the_test_shapes():
    """The production (team size, configuration) pairs, each under a forced
    variant at one of the shapes below (no device needed)."""
    assert _op_plan(9217, 300, -1)[0] == 2 and _op_plan(9217, 300, 25) == _op_plan(9217, 300, -1)  # (2, 5): C2's
    assert _op_plan(1001, 517, 25)[0] == 2
    assert _op_plan(20001, 131, 162)[0] == 16 and _op_plan(20001, 7, 162)[0] == 16  # (16, 2)
    assert _op_plan(20001, 131, 322)[0] == 32 and _op_plan(20001, 7, 322)[0] == 32  # (32, 2)
    for v in (83, 163, 323):  # configuration 3, the head-start launch's ring
        assert _op_plan(20001, 131, v) is not None, v
    assert _op_plan(7001, 150, 22)[:2] == (2, 4)  # four loads per lane: its head-start plan is configuration 3


@pytest.fixture(scope="module")
def pairs():
    """shape -> (N, Mt, X, stored, F32 context loaded from the fp64 host matrix
    X, F64 context loaded with what the F32 one stores); made once per shape
    and shared by the tests that use it."""
    made = {}

    def get(shape):
        if shape not in made:
            N, Mt = shape
            X = matrix(N, Mt)
            d32 = va.Data(N, Mt, storage="f32")
            d32.load_meth(X)
            stored = d32.get_meth_data()
            d64 = va.Data(N, Mt, storage="f64")
            d64.load_meth(stored)
            made[shape] = (N, Mt, X, stored, d32, d64)
        return made[shape]

    yield get
    for v in made.values():
        v[4].close()
        v[5].close()


def _ids(s):
    return "N%d_M%d" % s


@pytest.fixture(params=SHAPES, ids=_ids)
def pair(request, pairs):
    return pairs(request.param)


@pytest.fixture(params=[(1001, 517), (9217, 300)], ids=_ids)
def run_pair(request, pairs):  # the shapes of the whole runs
    return pairs(request.param)


@pytest.fixture
def pin_pair(pairs):  # the reference pin's shape
    return pairs((1001, 517))


# ---- 1. rounding -------------------------------------------------------------
def test_storage_attribute_and_late_switch(pair):
    N, Mt, X, stored, d32, d64 = pair
    assert d32.storage == "f32" and d64.storage == "f64"
    lib = va.load()
    assert lib.vampomi_set_storage(d32.ctx, va.STORE_F64) == 6  # VAMPOMI_ERR_STATE: the shard is allocated
    assert lib.vampomi_set_storage(d64.ctx, va.STORE_F32) == 6
    assert d32.storage == "f32" and d64.storage == "f64"


def test_host_fp64_is_rounded_to_nearest_even(pair):
    N, Mt, X, stored, d32, d64 = pair
    assert np.array_equal(stored, widened(X))
    assert not np.array_equal(stored, X)  # the rounding is real at this design
    assert np.array_equal(d64.get_meth_data(), stored)
    assert np.array_equal(d32.get_meth_data(Mt - 3, 3), widened(X[Mt - 3:]))


def test_every_ingest_path_gives_the_same_floats(tmp_path):
    N, Mt = 1001, 517
    X = matrix(N, Mt, seed=5)
    W = widened(X)
    p64, p32 = tmp_path / "x64.bin", tmp_path / "x32.bin"
    X.tofile(p64)
    X.astype(np.float32).tofile(p32)
    with va.Data(N, Mt, storage="f32") as d:
        d.read_methylation_data(str(p64))
        assert np.array_equal(d.get_meth_data(), W)
        mave, msig = d.get_mave(), d.get_msig()
    for storage in ("f32", "f64"):
        with va.Data(N, Mt, storage=storage) as d:
            d.read_methylation_data(str(p32), dtype="f32")
            assert np.array_equal(d.get_meth_data(), W), storage
            assert np.array_equal(d.get_mave(), mave) and np.array_equal(d.get_msig(), msig), storage
        with va.Data(N, Mt, storage=storage) as d:
            d.load_meth(X.astype(np.float32))
            assert np.array_equal(d.get_meth_data(), W), storage
            assert np.array_equal(d.get_mave(), mave) and np.array_equal(d.get_msig(), msig), storage
    mo, so = O.marker_stats(W)  # the statistics are those of the stored values
    assert relerr(mave, mo) < 1e-13 and relerr(msig, so) < 1e-13


def test_ragged_multichunk_ingest_of_both_file_types(tmp_path, monkeypatch):
    """More than one 256 MB staging chunk with a ragged last one, through the
    narrowing kernel (fp64 file) and the direct copy (fp32 file)."""
    monkeypatch.setenv("VAMPOMI_IO_THREADS", "3")
    N, Mt = 4099, 8200  # 269 MB as doubles: two chunks of 8186 and 14 columns
    X = O.generate_markers(31, 1, N, 0, Mt)
    p64, p32 = tmp_path / "big64.bin", tmp_path / "big32.bin"
    X.tofile(p64)
    X.astype(np.float32).tofile(p32)
    with va.Data(N, Mt, storage="f32") as a, va.Data(N, Mt, storage="f32") as b:
        a.read_methylation_data(str(p64))
        b.read_methylation_data(str(p32), dtype="f32")
        for i0 in (0, 8184, 8185, 8186, Mt - 3):
            want = widened(X[i0:i0 + 3])
            assert np.array_equal(a.get_meth_data(i0, 3), want), i0
            assert np.array_equal(b.get_meth_data(i0, 3), want), i0
        assert np.array_equal(a.get_mave(), b.get_mave()) and np.array_equal(a.get_msig(), b.get_msig())


@pytest.mark.parametrize("dtype,es", [("f64", 8), ("f32", 4)])
def test_short_file_is_an_io_error(tmp_path, dtype, es):
    N, Mt = 100, 50
    p = tmp_path / "short.bin"
    p.write_bytes(bytes((Mt * N - 1) * es))  # one element short
    with va.Data(N, Mt, storage="f32") as d:
        with pytest.raises(va.VampomiError) as e:
            d.read_methylation_data(str(p), dtype=dtype)
        assert e.value.status == 4


def test_generated_values_are_rounded():
    N, Mt = 1001, 517
    with va.Data(N, Mt, storage="f32") as a, va.Data(N, Mt, storage="f64") as b:
        a.generate(7, va.GEN_GAUSS)
        b.generate(7, va.GEN_GAUSS)
        assert np.array_equal(a.get_meth_data(), b.get_meth_data())  # every value is exactly a float
        assert np.array_equal(a.get_mave(), b.get_mave()) and np.array_equal(a.get_msig(), b.get_msig())
    with va.Data(N, Mt, storage="f32") as a, va.Data(N, Mt, storage="f64") as b:
        a.generate(7, va.GEN_METH)
        b.generate(7, va.GEN_METH)
        assert np.array_equal(a.get_meth_data(), widened(b.get_meth_data()))


# ---- 2. operators, bit for bit ----------------------------------------------------
@pytest.mark.parametrize("alpha", [1.0, 0.7])
def test_marker_stats_bitwise(alpha):
    N, Mt = 1001, 517
    X = matrix(N, Mt)
    with va.Data(N, Mt, alpha_scale=alpha, storage="f32") as a, va.Data(N, Mt, alpha_scale=alpha) as b:
        a.load_meth(X)
        b.load_meth(a.get_meth_data())
        assert np.array_equal(a.get_mave(), b.get_mave()) and np.array_equal(a.get_msig(), b.get_msig())


def _base(name):
    return name.split("<")[0]


def test_ax_every_variant_bitwise(pair):
    N, Mt, X, stored, d32, d64 = pair
    x = np.random.default_rng(N).normal(size=Mt)
    for v in list(range(7)) + [7]:
        try:
            d32.set_variant(0, v)
        except va.VampomiError:
            continue
        d64.set_variant(0, v)
        n32, n64 = d32.kernel_name(0, 1), d64.kernel_name(0, 1)
        assert _base(n32).endswith("_f32") and _base(n32)[:-4] == _base(n64), (n32, n64)
        assert _base(n64) in ("ax_partial_kernel", "ax_team_kernel") and n32.split("<")[1] == n64.split("<")[1]
        assert np.array_equal(d32.Ax(x), d64.Ax(x)), (v, n32)
    d32.set_variant(0, -1)
    d64.set_variant(0, -1)


def test_atx_lmmse_pcg_bitwise(pair):
    N, Mt, X, stored, d32, d64 = pair
    rng = np.random.default_rng(N + 1)
    u, v = rng.normal(size=N), rng.normal(size=Mt)
    for var in range(8):
        d32.set_variant(1, var)
        d64.set_variant(1, var)
        for mode in (0, 1):
            n32, n64 = d32.kernel_name(1, 1, mode), d64.kernel_name(1, 1, mode)
            assert _base(n64) == "atx_kernel" and _base(n32) == "atx_kernel_f32", (n32, n64)
            assert n32.split("<")[1] == n64.split("<")[1]
        assert np.array_equal(d32.ATx(u), d64.ATx(u)), var
        assert np.array_equal(d32.lmmse_mult(v, 0.9, 0.35), d64.lmmse_mult(v, 0.9, 0.35)), var
    d32.set_variant(1, -1)
    d64.set_variant(1, -1)
    for onsager in (False, True):
        a, ia = d32.pcg(v, 0.9, 0.35, onsager=onsager, max_iter=12)
        b, ib = d64.pcg(v, 0.9, 0.35, onsager=onsager, max_iter=12)
        assert ia == ib and np.array_equal(a, b), onsager


def _plans(d):
    ok = []
    for v in CANDIDATES:
        try:
            d.set_variant(3, v)
        except va.VampomiError:
            continue
        ok.append(v)
    d.set_variant(3, -1)
    return ok


def test_operator_every_plan_bitwise(pair):
    N, Mt, X, stored, d32, d64 = pair
    plans = _plans(d32)
    assert plans == _plans(d64) and plans, plans  # plans do not depend on the storage
    if (N, Mt) == (9217, 300):
        assert {0, 10, 25} <= set(plans)  # the whole-column kernel, one workgroup per column at S = 10, C2's team of 2
    if N == 20001:
        assert {162, 322, 83} <= set(plans)
    rng = np.random.default_rng(N + 2)
    diag, tau, gam2 = 1.7, 0.9, 0.35
    for K in (1, 2):
        ar, qo = rng.normal(size=(K, N)), rng.normal(size=(K, N))
        p, z = rng.normal(size=(K, Mt)), rng.normal(size=(K, Mt))
        beta = rng.uniform(0.1, 0.9, size=K)
        for fused in (False, True):
            zz, qq, bb = (z, qo, beta) if fused else (None, None, None)
            for v in plans:
                d32.set_variant(3, v)
                d64.set_variant(3, v)
                n32, n64 = d32.kernel_name(3, K), d64.kernel_name(3, K)
                assert _base(n64) in ("atax_kernel", "atax_team_kernel") and _base(n32) == _base(n64) + "_f32"
                assert n32.split("<")[1] == n64.split("<")[1]
                a = d32.op_apply(ar, p, diag, tau, gam2, z=zz, qo=qq, beta=bb)
                b = d64.op_apply(ar, p, diag, tau, gam2, z=zz, qo=qq, beta=bb)
                for x, y, what in zip(a, b, ("d", "A d", "<d,p>")):
                    assert np.array_equal(x, y), (what, v, n32, K, fused)
    d32.set_variant(3, -1)
    d64.set_variant(3, -1)


def test_operator_against_numpy_on_the_rounded_matrix(pair):
    """(not only against the fp64 engine: the explicit matrix, 1e-12 as tests/test_gpu_operator.py)"""
    N, Mt, X, stored, d32, d64 = pair
    mave, msig = O.marker_stats(stored)
    rng = np.random.default_rng(N + 3)
    ar, p = rng.normal(size=(1, N)), rng.normal(size=(1, Mt))
    Xc = stored - mave[:, None]
    t = (Xc @ (ar / 1.7).T).T * msig[None, :] / np.sqrt(N)
    d = 0.9 * t + 0.35 * p
    ad = (Xc.T @ (msig[None, :] * d).T).T / np.sqrt(N)
    gd, gad, gdp = d32.op_apply(ar, p, 1.7, 0.9, 0.35)
    assert relerr(gd, d) < 1e-12 and relerr(gad, ad) < 1e-12
    assert np.allclose(gdp, np.sum(d * p, axis=1), rtol=1e-12, atol=0)


# ---- 3. whole runs, bit for bit -------------------------------------------------------
def _phen(N, Mt, binary=False, seed=3):
    rng = np.random.default_rng(seed)
    beta = np.zeros(Mt)
    idx = rng.choice(Mt, max(3, Mt // 10), replace=False)
    beta[idx] = rng.normal(0, np.sqrt(0.8 / len(idx)), len(idx))
    y = rng.normal(size=N)
    if binary:
        return (y > 0).astype(np.float64), beta
    return O.standardize_phen(y), beta


def _run(d, y, beta, model="linear", its=6, **kw):
    d.set_phen(y, standardize=False)
    v = va.Vamp(d, va.VampOptions(max_iter=its, stop_criteria_thr=0.0, model=model, **kw),
                true_signal=beta[d.S:d.S + d.M])
    v.infere(keep_hist=True)
    s = v.summary()
    n = s["iterations"]
    out = {"n": n, "x1": v.x1_hist[:n, :d.M].copy(), "r1": v.r1_hist[:n, :d.M].copy(),
           "params": np.array(s["params"]), "metrics": np.array(s["metrics"]), "cg": s["cg_iters"],
           "ons": s["ons_iters"], "L": s["L"]}
    if "prior" in s:
        out["prior"] = np.array(s["prior"])
    return out


def _same(a, b, what):
    assert a["n"] == b["n"] and a["cg"] == b["cg"] and a["ons"] == b["ons"] and a["L"] == b["L"], what
    for k in ("x1", "r1", "params", "metrics", "prior"):
        if k in a:
            assert np.array_equal(a[k], b[k], equal_nan=True), (what, k)


def test_linear_runs_bitwise(run_pair):
    N, Mt, X, stored, d32, d64 = run_pair
    y, beta = _phen(N, Mt)
    for batch_rhs in (0, 3, 4):
        for hs in (1, 0):
            for pre in (0, 1):
                for d in (d32, d64):
                    d.set_variant(5, hs)
                    d.set_variant(7, pre)
                a = _run(d32, y, beta, batch_rhs=batch_rhs)
                b = _run(d64, y, beta, batch_rhs=batch_rhs)
                _same(a, b, (batch_rhs, hs, pre))
                assert d32.prestep_counts() == d64.prestep_counts()
    for d in (d32, d64):
        d.set_variant(5, 1)
        d.set_variant(7, 2)


def test_headstart_configuration_3_run_bitwise():
    """Under plan 22 at N = 7001 the head-start launch is the short-ring
    configuration 3 (atax_team_plain_kernel<4, 3, 5, 2, ...>), C3's."""
    N, Mt = 7001, 150
    X = matrix(N, Mt, seed=9)
    y, beta = _phen(N, Mt)
    with va.Data(N, Mt, storage="f32") as a, va.Data(N, Mt) as b:
        a.load_meth(X)
        b.load_meth(a.get_meth_data())
        for d in (a, b):
            d.set_variant(3, 22)
            d.set_variant(7, 1)
        assert b.kernel_name(3, 4).startswith("atax_team_plain_kernel<4, 3, 5, 2, true"), b.kernel_name(3, 4)
        assert a.kernel_name(3, 4).startswith("atax_team_plain_kernel_f32<4, 3, 5, 2, true"), a.kernel_name(3, 4)
        ra, rb = _run(a, y, beta, its=4), _run(b, y, beta, its=4)
        _same(ra, rb, "plan 22")
        assert a.prestep_counts() == b.prestep_counts()


def test_probit_run_bitwise(pin_pair):
    N, Mt, X, stored, d32, d64 = pin_pair
    y, beta = _phen(N, Mt, binary=True)
    a = _run(d32, y, beta, model="bin_class", its=4)
    b = _run(d64, y, beta, model="bin_class", its=4)
    assert "prior" in a
    _same(a, b, "bin_class")


def _run_ranks(monkeypatch, P, N, Mt, storage, fn, timeout=100):
    monkeypatch.setenv("VAMPOMI_COMM", "loopback")
    cid = os.urandom(va.UNIQUE_ID_BYTES)
    res, errs = [None] * P, []

    def work(r):
        try:
            with va.Data(N, Mt, rank=r, nranks=P, comm_id=cid, device=0, storage=storage) as d:
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


def test_two_loopback_ranks_bitwise(monkeypatch):
    """The host-free multi-rank tail and the folded CG decisions on an F32
    shard; the storage is rank-local, so a mixed job (rank 0 F32, rank 1 F64 on
    the same stored values) gives the same bits too."""
    N, Mt = 1001, 517
    W = widened(matrix(N, Mt))
    y, beta = _phen(N, Mt)

    def fn(r, d):
        d.load_meth(W[d.S:d.S + d.M])
        return _run(d, y, beta)

    r32 = _run_ranks(monkeypatch, 2, N, Mt, "f32", fn)
    r64 = _run_ranks(monkeypatch, 2, N, Mt, "f64", fn)
    for r in range(2):
        _same(r32[r], r64[r], ("rank", r))


# ---- 4. association and test mode, bit for bit ---------------------------------------------
def test_association_and_test_mode_bitwise(pair):
    N, Mt, X, stored, d32, d64 = pair
    y, beta = _phen(N, Mt)
    est = beta / np.sqrt(N)
    for d in (d32, d64):
        d.set_phen(y, standardize=False)
    for variant in (16, 0):  # the default (loo_wg_kernel) and loo_kernel
        for d in (d32, d64):
            d.set_variant(2, variant)
        n32, n64 = d32.kernel_name(2, 1), d64.kernel_name(2, 1)
        assert _base(n64) in ("loo_kernel", "loo_wg_kernel") and _base(n32) == _base(n64) + "_f32"
        pa, sa = d32.assoc_loo(est)
        pb, sb = d64.assoc_loo(est)
        assert np.array_equal(sa, sb) and np.array_equal(pa, pb, equal_nan=True), variant
    for d in (d32, d64):
        d.set_variant(2, 16)
    r1 = np.random.default_rng(5).normal(size=Mt) * 0.05
    assert np.array_equal(d32.assoc_se(r1, 2.5), d64.assoc_se(r1, 2.5))
    assert d32.test_metrics(est) == d64.test_metrics(est)


# ---- 5. against the oracle --------------------------------------------------------------------
def test_f32_linear_run_vs_oracle_on_the_rounded_matrix(pin_pair):
    N, Mt, X, stored, d32, d64 = pin_pair
    y, beta = _phen(N, Mt)
    its = 6
    ref = O.vamp_infere(stored, y, Mt, true_signal=beta, max_iter=its, stop_criteria_thr=0.0)
    g = _run(d32, y, beta, its=its)
    assert g["n"] == ref["iterations"]
    assert g["cg"] == ref["cg_iters"].tolist() and g["ons"] == ref["ons_iters"].tolist()
    assert g["L"] == ref["L"].tolist()
    for k in range(g["n"]):
        e1, e2 = relerr(g["x1"][k], ref["x1_hist"][k]), relerr(g["r1"][k], ref["r1_hist"][k])
        print(f"iteration {k + 1}: x1 {e1:.3e} r1 {e2:.3e}")
        assert e1 <= 1e-10 and e2 <= 1e-10, (k, e1, e2)


# ---- 6. accounting ------------------------------------------------------------------------------
def test_bytes_are_counted_at_the_stored_element_size(pair):
    N, Mt, X, stored, d32, d64 = pair
    rng = np.random.default_rng(1)
    x, ar, p = rng.normal(size=Mt), rng.normal(size=(1, N)), rng.normal(size=(1, Mt))

    def pass_bytes(es, K):  # engine.cpp pass_bytes: X once, K N-vectors, mave/msig and K M-vectors
        return float(es) * N * Mt + 8.0 * K * N + 8.0 * (2.0 + K) * Mt

    got = {}
    for d, es in ((d32, 4), (d64, 8)):
        d.set_timing(False)
        d.reset_stats()
        d.Ax(x)
        d.op_apply(ar, p, 1.7, 0.9, 0.35)
        s = d.stats()
        assert (s.ax.launches, s.op.launches) == (1, 1)
        assert s.ax.bytes_total == pass_bytes(es, 1) and s.op.bytes_total == pass_bytes(es, 1), es
        got[es] = s.ax.bytes_total
    assert got[8] - got[4] == 4.0 * N * Mt


def test_read_ceiling_counts_resident_bytes():
    N, Mt = 4099, 1024  # 16 MiB as floats: both stream shapes have whole units
    with va.Data(N, Mt, storage="f32") as a, va.Data(N, Mt) as b:
        a.generate(3, va.GEN_METH)
        b.generate(3, va.GEN_METH)
        ca, cb = a.read_ceiling(reps=3), b.read_ceiling(reps=3)
    assert 0 < ca["bytes"] <= 4 * Mt * a.ld and 0 < cb["bytes"] <= 8 * Mt * b.ld
    assert ca["bytes"] > 0.9 * 4 * Mt * a.ld and cb["bytes"] > 0.9 * 8 * Mt * b.ld


# ---- 7. the command-line program -------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_cli_storage_f32_equals_f64_on_the_widened_file(tmp_path, dtype):
    N, Mt, its = 400, 900, 5
    X = matrix(N, Mt, seed=13)
    y, beta = _phen(N, Mt)
    yp = tmp_path / "ex.phen"
    with open(yp, "w") as f:
        for i, v in enumerate(y):
            f.write("%d %d %0.10f\n" % (i, i, v))
    tp = tmp_path / "ex_ts.bin"
    beta.astype("<f8").tofile(tp)
    src = tmp_path / f"x_{dtype}.bin"
    (X if dtype == "f64" else X.astype(np.float32)).tofile(src)
    wide = tmp_path / "x_widened.bin"  # an fp64 file that already holds the stored floats
    widened(X).tofile(wide)
    outs = {}
    for tag, meth, flags in (("f32", src, ["--meth-storage", "f32", "--meth-dtype", dtype]),
                             ("f64", wide, ["--meth-storage", "f64"])):
        out = tmp_path / tag
        out.mkdir()
        cmd = [va.CLI_PATH, "--meth-file", str(meth), "--phen-file", str(yp), "--N", str(N), "--Mt", str(Mt),
               "--out-dir", str(out), "--out-name", "ex", "--iterations", str(its), "--stop-criteria-thr", "0",
               "--true-signal-file", str(tp)] + flags
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        assert f"--meth-storage {tag}\n" in r.stdout
        outs[tag] = out
    names = ["ex_params.csv", "ex_metrics.csv"] + [pat % it for it in range(1, its + 1)
                                                   for pat in ("ex_it_%d.bin", "ex_r1_it_%d.bin")]
    for name in names:
        a, b = (outs["f32"] / name).read_bytes(), (outs["f64"] / name).read_bytes()
        assert len(a) > 0 and a == b, name
