"""16-bit fixed-point storage of the methylation shard (VAMPOMI_STORE_U16) on
the device: the stored element is a uint16 k meaning k * 2^-16.

The storage changes one thing, the quantisation of X at ingest: a u16 lane owns
the same rows as the fp64 lane of the same plan and widens what it loads
((double)k * 2^-16, exact), so every sum runs in the same order.  Hence the bar
of this file, the fp32 storage's: a U16 context gives, BIT FOR BIT, what an F64
context gives on the dequantised matrix (the U16 context's get_meth_data()), for
the operators under every plan, for whole runs, and for the association and
test modes.  One run is also held to the CPU oracle on the dequantised matrix
(the project's 1e-10), which ties the new path to the checker and not only to
the fp64 engine.  The quantisation itself is held to numpy's rint.

Shapes (tests/test_gpu_storage_f32.py's: the smallest that reach each path):
  (1001, 517)   odd N with a pad row, the reference pin's shape, team size 1
  (9217, 300)   just past the 9216 rows of the default one-workgroup plan: the team of 2
  (20001, 131)  teams of 8-32, a short last tile, M no multiple of the team count
  (20001, 7)    fewer markers than teams: empty teams
  (7001, 150)   under plan 22 its head-start launch is configuration 3
"""
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
ERR_RANGE = 9


def quant(X):
    """The format's rule, in numpy: rint rounds ties to even; X * 65536 is exact."""
    return np.minimum(65535, np.rint(np.asarray(X, dtype=np.float64) * 65536)).astype(np.uint16)


def deq(k):
    return k.astype(np.float64) / 65536  # exact


def stored_k(d, i0=0, count=None):
    v = d.get_meth_data(i0, count) * 65536
    assert np.array_equal(v, np.rint(v)) and v.min() >= 0 and v.max() <= 65535  # every stored value is on the grid
    return v.astype(np.uint16)


def matrix(N, Mt, seed=11):
    """Methylation-like values in [0, 1] with full fp64 mantissas."""
    return O.generate_markers(seed, 1, N, 0, Mt)


@pytest.fixture(scope="module")
def pairs():
    """shape -> (N, Mt, X, stored, U16 context loaded from the fp64 host matrix
    X, F64 context loaded with what the U16 one stores, dequantised); made once
    per shape and shared by the tests that use it."""
    made = {}

    def get(shape):
        if shape not in made:
            N, Mt = shape
            X = matrix(N, Mt)
            d16 = va.Data(N, Mt, storage="u16")
            d16.load_meth(X)
            stored = d16.get_meth_data()
            d64 = va.Data(N, Mt, storage="f64")
            d64.load_meth(stored)
            made[shape] = (N, Mt, X, stored, d16, d64)
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


# ---- 1. quantisation against numpy ------------------------------------------------
def test_storage_attribute_and_late_switch(pair):
    N, Mt, X, stored, d16, d64 = pair
    assert d16.storage == "u16" and d64.storage == "f64"
    lib = va.load()
    assert lib.vampomi_set_storage(d16.ctx, va.STORE_F64) == 6  # VAMPOMI_ERR_STATE: the shard is allocated
    assert lib.vampomi_set_storage(d64.ctx, va.STORE_U16) == 6
    assert d16.storage == "u16" and d64.storage == "f64"


def test_generator_matrix_is_quantised_as_numpy_does(pair):
    N, Mt, X, stored, d16, d64 = pair
    k = quant(X)
    assert X.min() >= 0 and X.max() <= 1
    assert np.array_equal(stored_k(d16), k)
    assert np.array_equal(stored, deq(k)) and not np.array_equal(stored, X)  # the quantisation is real
    assert np.array_equal(d64.get_meth_data(), stored)
    assert np.array_equal(d16.get_meth_data(Mt - 3, 3), deq(k[Mt - 3:]))
    qs = d16.quant_stats()
    assert qs["clamped"] == int(np.count_nonzero(np.rint(X * 65536) > 65535))
    assert qs["max_abs_err"] == np.abs(deq(k) - X).max()
    # the grid's bound: half a step, or a whole one where an entry was clamped (1.0 is stored as 1 - 2^-16)
    assert 0 < qs["max_abs_err"] <= (2.0 ** -16 if qs["clamped"] else 2.0 ** -17)
    assert d64.quant_stats() == {"clamped": 0, "max_abs_err": 0.0}


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_edge_values_ties_and_clamps(dtype):
    col = np.array([0.0, -0.0, 2.0 ** -17, 3 * 2.0 ** -17, 1 - 2.0 ** -17, 1.0, 65535 / 65536, 0.5,
                    5 * 2.0 ** -17, 2.0 ** -16, 1 - 2.0 ** -16 - 2.0 ** -18, 0.25 + 2.0 ** -18])
    want = np.array([0, 0, 0, 2, 65535, 65535, 65535, 32768, 2, 1, 65535, 16384], dtype=np.uint16)
    assert np.array_equal(col.astype(np.float32).astype(np.float64), col)  # every value is a float too
    N, Mt = len(col), 2
    X = np.stack([col, col[::-1]]).astype(dtype)
    assert np.array_equal(quant(X[0]), want)  # numpy agrees with the values worked out by hand
    with va.Data(N, Mt, storage="u16") as d:
        d.load_meth(X)
        assert np.array_equal(stored_k(d), np.stack([want, want[::-1]]))
        qs = d.quant_stats()
        assert qs["clamped"] == 4  # 1 - 2^-17 and 1.0, in both columns
        assert qs["max_abs_err"] == np.abs(deq(quant(X)) - X.astype(np.float64)).max() == 2.0 ** -16  # 1.0 -> 65535/65536


# ---- 2. rejection --------------------------------------------------------------------
@pytest.mark.parametrize("bad", [np.nan, np.inf, -1e-300, 1 + 2.0 ** -52], ids=["nan", "inf", "neg", "above1"])
def test_out_of_range_input_is_rejected(bad):
    N, Mt = 1001, 40
    X = matrix(N, Mt, seed=2)
    Xb = X.copy()
    Xb[23, 700] = bad
    with va.Data(N, Mt, storage="u16") as d:
        with pytest.raises(va.VampomiError) as e:
            d.load_meth(Xb)
        assert e.value.status == ERR_RANGE
        assert "marker 23, row 700" in str(e.value) and str(e.value).split(": ", 1)[1].startswith("1 "), str(e.value)
        with pytest.raises(va.VampomiError) as e2:
            d.get_meth_data()
        assert e2.value.status == 6  # no shard, as after an I/O error
        # two more, an earlier and a later one: the count, and the smallest (marker, row)
        Xb[23, 650] = -0.5
        Xb[30, 2] = np.nan
        with pytest.raises(va.VampomiError) as e:
            d.load_meth(Xb)
        assert e.value.status == ERR_RANGE and "marker 23, row 650" in str(e.value)
        assert str(e.value).split(": ", 1)[1].startswith("3 "), str(e.value)
        d.load_meth(X)  # the context is reusable
        assert np.array_equal(stored_k(d), quant(X))
        assert d.quant_stats()["max_abs_err"] == np.abs(deq(quant(X)) - X).max()
    with va.Data(N, Mt, storage="f64") as d:  # the other storages take the same matrix as before
        d.load_meth(Xb)
        assert np.array_equal(d.get_meth_data(), Xb, equal_nan=True)


def test_gaussian_generator_is_refused_on_u16():
    with va.Data(1001, 40, storage="u16") as d:
        with pytest.raises(va.VampomiError) as e:
            d.generate(7, va.GEN_GAUSS)
        assert e.value.status == ERR_RANGE
        d.generate(7, va.GEN_METH)  # still usable
        assert d.get_meth_data().shape == (40, 1001)


# ---- 3. every ingest path --------------------------------------------------------------
def test_every_ingest_path_gives_the_same_k(tmp_path, monkeypatch):
    """Host fp64 / fp32 / uint16 and fp64 / fp32 / uint16 files, the files in
    ragged chunks: 100 000-byte staging chunks are 12 fp64, 24 fp32 and 49 uint16
    columns of N = 1001, none a divisor of Mt = 517, and more chunks than the
    three staging buffers."""
    N, Mt = 1001, 517
    X = matrix(N, Mt, seed=5).astype(np.float32).astype(np.float64)  # exactly floats: one k for both input types
    k = quant(X)
    p64, p32, p16 = tmp_path / "x64.bin", tmp_path / "x32.bin", tmp_path / "x16.bin"
    X.tofile(p64)
    X.astype(np.float32).tofile(p32)
    k.astype("<u2").tofile(p16)
    monkeypatch.setenv("VAMPOMI_IO_THREADS", "3")
    got = {}
    for chunk in (None, "100000"):
        if chunk:
            monkeypatch.setenv("VAMPOMI_IO_CHUNK_BYTES", chunk)
        for name, load in (("host f64", lambda d: d.load_meth(X)),
                           ("host f32", lambda d: d.load_meth(X.astype(np.float32))),
                           ("host u16", lambda d: d.load_meth(k)),
                           ("file f64", lambda d: d.read_methylation_data(str(p64))),
                           ("file f32", lambda d: d.read_methylation_data(str(p32), dtype="f32")),
                           ("file u16", lambda d: d.read_methylation_data(str(p16), dtype="u16"))):
            with va.Data(N, Mt, storage="u16") as d:
                load(d)
                assert np.array_equal(stored_k(d), k), (name, chunk)
                got[name, chunk] = (d.get_mave(), d.get_msig(), d.quant_stats())
    ref = got["host f64", None]
    for key, v in got.items():
        assert np.array_equal(v[0], ref[0]) and np.array_equal(v[1], ref[1]), key
        if "u16" in key[0]:
            assert v[2] == {"clamped": 0, "max_abs_err": 0.0}, key  # nothing was quantised
        else:
            assert v[2] == ref[2], key
    mo, so = O.marker_stats(deq(k))  # the statistics are those of the stored values
    assert relerr(ref[0], mo) < 1e-13 and relerr(ref[1], so) < 1e-13


def test_generator_path_gives_numpys_k(monkeypatch):
    N, Mt = 1001, 517
    k = quant(O.generate_markers(7, 1, N, 0, Mt))
    with va.Data(N, Mt, storage="u16") as a:
        a.generate(7, va.GEN_METH)
        assert np.array_equal(stored_k(a), k)
        whole = a.quant_stats()
    monkeypatch.setenv("VAMPOMI_IO_CHUNK_BYTES", "100000")  # 12 columns per generated chunk
    with va.Data(N, Mt, storage="u16") as a:
        a.generate(7, va.GEN_METH)
        assert np.array_equal(stored_k(a), k)
        assert a.quant_stats() == whole


@pytest.mark.parametrize("storage", ["f32", "f64"])
def test_u16_input_widens_exactly_on_the_other_storages(tmp_path, storage):
    N, Mt = 1001, 517
    k = quant(matrix(N, Mt, seed=5))
    p16 = tmp_path / "x16.bin"
    k.astype("<u2").tofile(p16)
    with va.Data(N, Mt, storage=storage) as d:
        d.read_methylation_data(str(p16), dtype="u16")
        assert np.array_equal(d.get_meth_data(), deq(k))
        mave, msig = d.get_mave(), d.get_msig()
        d.load_meth(k)
        assert np.array_equal(d.get_meth_data(), deq(k))
        assert np.array_equal(d.get_mave(), mave) and np.array_equal(d.get_msig(), msig)
        assert d.quant_stats() == {"clamped": 0, "max_abs_err": 0.0}


@pytest.mark.parametrize("storage", ["u16", "f64"])
def test_short_u16_file_is_an_io_error(tmp_path, storage):
    N, Mt = 100, 50
    p = tmp_path / "short.bin"
    p.write_bytes(bytes((Mt * N - 1) * 2))  # one element short
    with va.Data(N, Mt, storage=storage) as d:
        with pytest.raises(va.VampomiError) as e:
            d.read_methylation_data(str(p), dtype="u16")
        assert e.value.status == 4


# ---- 4. operators, bit for bit ----------------------------------------------------------
@pytest.mark.parametrize("alpha", [1.0, 0.7])
def test_marker_stats_bitwise(alpha):
    N, Mt = 1001, 517
    X = matrix(N, Mt)
    with va.Data(N, Mt, alpha_scale=alpha, storage="u16") as a, va.Data(N, Mt, alpha_scale=alpha) as b:
        a.load_meth(X)
        b.load_meth(a.get_meth_data())
        assert np.array_equal(a.get_mave(), b.get_mave()) and np.array_equal(a.get_msig(), b.get_msig())


def _base(name):
    return name.split("<")[0]


def test_ax_every_variant_bitwise(pair):
    N, Mt, X, stored, d16, d64 = pair
    x = np.random.default_rng(N).normal(size=(4, Mt))
    for v in list(range(7)) + [7]:
        try:
            d16.set_variant(0, v)
        except va.VampomiError:
            continue
        d64.set_variant(0, v)
        for K in (1, 2, 3, 4):
            n16, n64 = d16.kernel_name(0, K), d64.kernel_name(0, K)
            assert _base(n16).endswith("_u16") and _base(n16)[:-4] == _base(n64), (n16, n64)
            assert _base(n64) in ("ax_partial_kernel", "ax_team_kernel") and n16.split("<")[1] == n64.split("<")[1]
        for k in range(4):
            assert np.array_equal(d16.Ax(x[k]), d64.Ax(x[k])), (v, n16)
    d16.set_variant(0, -1)
    d64.set_variant(0, -1)


def test_atx_lmmse_pcg_bitwise(pair):
    N, Mt, X, stored, d16, d64 = pair
    rng = np.random.default_rng(N + 1)
    u, v = rng.normal(size=N), rng.normal(size=Mt)
    for var in range(8):
        d16.set_variant(1, var)
        d64.set_variant(1, var)
        for mode in (0, 1):
            n16, n64 = d16.kernel_name(1, 1, mode), d64.kernel_name(1, 1, mode)
            assert _base(n64) == "atx_kernel" and _base(n16) == "atx_kernel_u16", (n16, n64)
            assert n16.split("<")[1] == n64.split("<")[1]
        assert np.array_equal(d16.ATx(u), d64.ATx(u)), var
        assert np.array_equal(d16.lmmse_mult(v, 0.9, 0.35), d64.lmmse_mult(v, 0.9, 0.35)), var
    d16.set_variant(1, -1)
    d64.set_variant(1, -1)
    for onsager in (False, True):
        a, ia = d16.pcg(v, 0.9, 0.35, onsager=onsager, max_iter=12)
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
    N, Mt, X, stored, d16, d64 = pair
    plans = _plans(d16)
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
                d16.set_variant(3, v)
                d64.set_variant(3, v)
                n16, n64 = d16.kernel_name(3, K), d64.kernel_name(3, K)
                assert _base(n64) in ("atax_kernel", "atax_team_kernel") and _base(n16) == _base(n64) + "_u16"
                assert n16.split("<")[1] == n64.split("<")[1]
                a = d16.op_apply(ar, p, diag, tau, gam2, z=zz, qo=qq, beta=bb)
                b = d64.op_apply(ar, p, diag, tau, gam2, z=zz, qo=qq, beta=bb)
                for x, y, what in zip(a, b, ("d", "A d", "<d,p>")):
                    assert np.array_equal(x, y), (what, v, n16, K, fused)
    d16.set_variant(3, -1)
    d64.set_variant(3, -1)


def test_operator_against_numpy_on_the_dequantised_matrix(pair):
    """(not only against the fp64 engine: the explicit matrix, 1e-12 as tests/test_gpu_operator.py)"""
    N, Mt, X, stored, d16, d64 = pair
    mave, msig = O.marker_stats(stored)
    rng = np.random.default_rng(N + 3)
    ar, p = rng.normal(size=(1, N)), rng.normal(size=(1, Mt))
    Xc = stored - mave[:, None]
    t = (Xc @ (ar / 1.7).T).T * msig[None, :] / np.sqrt(N)
    d = 0.9 * t + 0.35 * p
    ad = (Xc.T @ (msig[None, :] * d).T).T / np.sqrt(N)
    gd, gad, gdp = d16.op_apply(ar, p, 1.7, 0.9, 0.35)
    assert relerr(gd, d) < 1e-12 and relerr(gad, ad) < 1e-12
    assert np.allclose(gdp, np.sum(d * p, axis=1), rtol=1e-12, atol=0)


# ---- 5. whole runs, bit for bit -------------------------------------------------------
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
    N, Mt, X, stored, d16, d64 = run_pair
    y, beta = _phen(N, Mt)
    for batch_rhs in (0, 3, 4):
        for hs in (1, 0):
            for pre in (0, 1):
                for d in (d16, d64):
                    d.set_variant(5, hs)
                    d.set_variant(7, pre)
                a = _run(d16, y, beta, batch_rhs=batch_rhs)
                b = _run(d64, y, beta, batch_rhs=batch_rhs)
                _same(a, b, (batch_rhs, hs, pre))
                assert d16.prestep_counts() == d64.prestep_counts()
    for d in (d16, d64):
        d.set_variant(5, 1)
        d.set_variant(7, 2)


def test_batched_ax_under_every_variant_bitwise(run_pair):
    """A.x with 2-4 right-hand sides has no entry point of its own: a run with
    batch_rhs = 4 launches it (the instantiations named in
    test_ax_every_variant_bitwise), here under every A.x variant and the team
    plan."""
    N, Mt, X, stored, d16, d64 = run_pair
    y, beta = _phen(N, Mt)
    ran = []
    for v in list(range(7)) + [7]:
        try:
            d16.set_variant(0, v)
        except va.VampomiError:
            continue
        d64.set_variant(0, v)
        _same(_run(d16, y, beta, its=2, batch_rhs=4), _run(d64, y, beta, its=2, batch_rhs=4), ("ax variant", v))
        ran.append(v)
    d16.set_variant(0, -1)
    d64.set_variant(0, -1)
    assert set(range(7)) <= set(ran) and (N < 9217 or 7 in ran), ran


def test_headstart_configuration_3_run_bitwise():
    """Under plan 22 at N = 7001 the head-start launch is the short-ring
    configuration 3 (atax_team_plain_kernel<4, 3, 5, 2, ...>), C3's."""
    N, Mt = 7001, 150
    X = matrix(N, Mt, seed=9)
    y, beta = _phen(N, Mt)
    with va.Data(N, Mt, storage="u16") as a, va.Data(N, Mt) as b:
        a.load_meth(X)
        b.load_meth(a.get_meth_data())
        for d in (a, b):
            d.set_variant(3, 22)
            d.set_variant(7, 1)
        assert b.kernel_name(3, 4).startswith("atax_team_plain_kernel<4, 3, 5, 2, true"), b.kernel_name(3, 4)
        assert a.kernel_name(3, 4).startswith("atax_team_plain_kernel_u16<4, 3, 5, 2, true"), a.kernel_name(3, 4)
        ra, rb = _run(a, y, beta, its=4), _run(b, y, beta, its=4)
        _same(ra, rb, "plan 22")
        assert a.prestep_counts() == b.prestep_counts()


def test_probit_run_bitwise(pin_pair):
    N, Mt, X, stored, d16, d64 = pin_pair
    y, beta = _phen(N, Mt, binary=True)
    a = _run(d16, y, beta, model="bin_class", its=4)
    b = _run(d64, y, beta, model="bin_class", its=4)
    assert "prior" in a
    _same(a, b, "bin_class")


def _run_ranks(monkeypatch, P, N, Mt, storages, fn, timeout=100):
    monkeypatch.setenv("VAMPOMI_COMM", "loopback")
    cid = os.urandom(va.UNIQUE_ID_BYTES)
    res, errs = [None] * P, []

    def work(r):
        try:
            with va.Data(N, Mt, rank=r, nranks=P, comm_id=cid, device=0, storage=storages[r]) as d:
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
    """The host-free multi-rank tail and the folded CG decisions on a U16
    shard; the storage is rank-local: rank 0 U16 and rank 1 F64 on the
    dequantised shard give the bits of two F64 ranks, and so do two U16 ranks."""
    N, Mt = 1001, 517
    W = deq(quant(matrix(N, Mt)))
    y, beta = _phen(N, Mt)

    def fn(r, d):
        d.load_meth(W[d.S:d.S + d.M])
        assert d.storage == ("u16", "f64")[fn.kinds[r]]
        return _run(d, y, beta)

    out = {}
    for name, kinds in (("mixed", (0, 1)), ("f64", (1, 1)), ("u16", (0, 0))):
        fn.kinds = kinds
        out[name] = _run_ranks(monkeypatch, 2, N, Mt, [("u16", "f64")[q] for q in kinds], fn)
    for r in range(2):
        _same(out["mixed"][r], out["f64"][r], ("mixed, rank", r))
        _same(out["u16"][r], out["f64"][r], ("u16, rank", r))


# ---- 6. association and test mode, bit for bit ---------------------------------------------
def test_association_and_test_mode_bitwise(pair):
    N, Mt, X, stored, d16, d64 = pair
    y, beta = _phen(N, Mt)
    est = beta / np.sqrt(N)
    for d in (d16, d64):
        d.set_phen(y, standardize=False)
    for variant in (16, 0):  # the default (loo_wg_kernel) and loo_kernel
        for d in (d16, d64):
            d.set_variant(2, variant)
        n16, n64 = d16.kernel_name(2, 1), d64.kernel_name(2, 1)
        assert _base(n64) in ("loo_kernel", "loo_wg_kernel") and _base(n16) == _base(n64) + "_u16"
        pa, sa = d16.assoc_loo(est)
        pb, sb = d64.assoc_loo(est)
        assert np.array_equal(sa, sb) and np.array_equal(pa, pb, equal_nan=True), variant
    for d in (d16, d64):
        d.set_variant(2, 16)
    r1 = np.random.default_rng(5).normal(size=Mt) * 0.05
    assert np.array_equal(d16.assoc_se(r1, 2.5), d64.assoc_se(r1, 2.5))
    assert d16.test_metrics(est) == d64.test_metrics(est)


# ---- 7. against the oracle --------------------------------------------------------------------
def test_u16_linear_run_vs_oracle_on_the_dequantised_matrix(pin_pair):
    N, Mt, X, stored, d16, d64 = pin_pair
    y, beta = _phen(N, Mt)
    its = 6
    ref = O.vamp_infere(stored, y, Mt, true_signal=beta, max_iter=its, stop_criteria_thr=0.0)
    g = _run(d16, y, beta, its=its)
    assert g["n"] == ref["iterations"]
    assert g["cg"] == ref["cg_iters"].tolist() and g["ons"] == ref["ons_iters"].tolist()
    assert g["L"] == ref["L"].tolist()
    for k in range(g["n"]):
        e1, e2 = relerr(g["x1"][k], ref["x1_hist"][k]), relerr(g["r1"][k], ref["r1_hist"][k])
        print(f"iteration {k + 1}: x1 {e1:.3e} r1 {e2:.3e}")
        assert e1 <= 1e-10 and e2 <= 1e-10, (k, e1, e2)


# ---- 8. accounting ------------------------------------------------------------------------------
def test_bytes_are_counted_at_two_per_element(pair):
    N, Mt, X, stored, d16, d64 = pair
    rng = np.random.default_rng(1)
    x, ar, p = rng.normal(size=Mt), rng.normal(size=(1, N)), rng.normal(size=(1, Mt))

    def pass_bytes(es, K):  # engine.cpp pass_bytes: X once, K N-vectors, mave/msig and K M-vectors
        return float(es) * N * Mt + 8.0 * K * N + 8.0 * (2.0 + K) * Mt

    got = {}
    for d, es in ((d16, 2), (d64, 8)):
        d.set_timing(False)
        d.reset_stats()
        d.Ax(x)
        d.op_apply(ar, p, 1.7, 0.9, 0.35)
        s = d.stats()
        assert (s.ax.launches, s.op.launches) == (1, 1)
        assert s.ax.bytes_total == pass_bytes(es, 1) and s.op.bytes_total == pass_bytes(es, 1), es
        got[es] = s.ax.bytes_total
    assert got[8] - got[2] == 6.0 * N * Mt


def test_read_ceiling_counts_resident_bytes():
    N, Mt = 4099, 2048  # 16 MiB as u16: both stream shapes have whole units
    with va.Data(N, Mt, storage="u16") as a:
        a.generate(3, va.GEN_METH)
        ca = a.read_ceiling(reps=3)
        assert 0.9 * 2 * Mt * a.ld < ca["bytes"] <= 2 * Mt * a.ld
        assert ca["us_med"] > 0


# ---- 9. the command-line program -------------------------------------------------------------------
def test_cli_storage_u16_equals_f64_on_the_dequantised_file(tmp_path):
    N, Mt, its = 400, 900, 5
    X = matrix(N, Mt, seed=13)
    y, beta = _phen(N, Mt)
    yp = tmp_path / "ex.phen"
    with open(yp, "w") as f:
        for i, v in enumerate(y):
            f.write("%d %d %0.10f\n" % (i, i, v))
    tp = tmp_path / "ex_ts.bin"
    beta.astype("<f8").tofile(tp)
    p64, p16, pdq = tmp_path / "x_f64.bin", tmp_path / "x_u16.bin", tmp_path / "x_dequantised.bin"
    X.tofile(p64)
    quant(X).astype("<u2").tofile(p16)
    deq(quant(X)).tofile(pdq)  # an fp64 file that already holds the stored values
    outs = {}
    for tag, storage, meth, flags in (("from_f64", "u16", p64, ["--meth-storage", "u16"]),
                                      ("from_u16", "u16", p16, ["--meth-storage", "u16", "--meth-dtype", "u16"]),
                                      ("f64", "f64", pdq, ["--meth-storage", "f64"])):
        out = tmp_path / tag
        out.mkdir()
        cmd = [va.CLI_PATH, "--meth-file", str(meth), "--phen-file", str(yp), "--N", str(N), "--Mt", str(Mt),
               "--out-dir", str(out), "--out-name", "ex", "--iterations", str(its), "--stop-criteria-thr", "0",
               "--true-signal-file", str(tp)] + flags
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        assert f"--meth-storage {storage}\n" in r.stdout
        outs[tag] = out
    names = ["ex_params.csv", "ex_metrics.csv"] + [pat % it for it in range(1, its + 1)
                                                   for pat in ("ex_it_%d.bin", "ex_r1_it_%d.bin")]
    for name in names:
        ref = (outs["f64"] / name).read_bytes()
        assert len(ref) > 0, name
        for tag in ("from_f64", "from_u16"):
            assert (outs[tag] / name).read_bytes() == ref, (tag, name)


def test_cli_reports_a_value_out_of_range(tmp_path):
    N, Mt = 50, 20
    X = matrix(N, Mt, seed=13)
    X[4, 9] = 1.5
    p64, yp = tmp_path / "x.bin", tmp_path / "ex.phen"
    X.tofile(p64)
    with open(yp, "w") as f:
        for i in range(N):
            f.write("%d %d %0.10f\n" % (i, i, np.sin(i)))
    r = subprocess.run([va.CLI_PATH, "--meth-file", str(p64), "--phen-file", str(yp), "--N", str(N), "--Mt", str(Mt),
                        "--out-dir", str(tmp_path), "--out-name", "ex", "--iterations", "2", "--meth-storage", "u16"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode != 0
    assert "marker 4, row 9" in r.stdout + r.stderr
