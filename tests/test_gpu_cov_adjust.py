"""Covariate adjustment on the device: vampomi_set_adjust / vampomi_read_adjust,
vk::adjust_cols behind every load route, the phenotype's projection, the guards
and --cov-adjust residual.

The bars of this file:
  * read-back: a stored F64 marker against x - Z1 lstsq(Z1, x), Z1 = [1, Z
    without the dropped columns] with cond(Z1) <= 10 (asserted): 1e-12 absolute.
    Two CPU routes (the Gram-Schmidt Q and lstsq) differ by at most 1.2e-14 at
    2049 x 64 with entries <= 1; the bar is about 100 times that, for the
    device's summation order.  |Q^T r| <= 1e-11 on the markers that are left.
  * the absorbed markers are exactly the planted in-span ones and read back as
    exact zeros (mave 0, msig 1).
  * the phenotype: 1e-13 relative against numpy; y = Z1 g exactly leaves less
    than 1e-12 |y|.
Everything else is np.array_equal or integer equality.

Shapes, with VAMPOMI_IO_CHUNK_BYTES=4096: 301 x 37 (N odd, ragged thread rows,
one fp64 column per chunk, M no multiple of the kernel's column block), 4099 x
23 and 70001 x 5, each with C in {0, 5, 64} (R = 1, 3, 61: C = 64 with its four
planted degenerate columns; R = 65 in test_full_rank_R65).  Matrix: the
methylation generator's with planted markers: constant 0.5, all zero, exactly
the first covariate, 0.3 Z_1 + 0.2, a duplicate pair.  (70001 x 5, as in
tests/test_gpu_meth_na.py, takes the five long-column ones: constant, 0.3 Z_1 +
0.2, an ordinary marker and the pair.)  With C = 0 the first covariate is not
adjusted for, so "exactly a covariate" and "0.3 Z_1 + 0.2" are ordinary markers.
"""
import os
import subprocess
import threading

import numpy as np
import pytest

import _cov_adjust as H
from _data import phen_from_markers

pytestmark = pytest.mark.gpu

va = pytest.importorskip("vampomi_amd")
from oracle import pyoracle as O  # noqa: E402  (the index-keyed generator and the phenotype's scaling only)

SHAPES = {(301, 37): ("const", "zero", "cov", "affine", "pair"), (4099, 23): ("const", "zero", "cov", "affine", "pair"),
          (70001, 5): ("const", "affine", "pair")}
CS = (0, 5, 64)
ERR_ARG, ERR_STATE = 1, 6
BAR_READBACK, BAR_ORTH, BAR_PHEN = 1e-12, 1e-11, 1e-13


def _ids(s):
    return "N%d_M%d" % s


@pytest.fixture(autouse=True)
def _small_chunks(monkeypatch):
    monkeypatch.setenv("VAMPOMI_IO_CHUNK_BYTES", "4096")
    monkeypatch.setenv("VAMPOMI_IO_THREADS", "3")


_cases = {}


def case(shape, nc):
    """X (M, N) with its planted markers, Z, the planted flags of Z, the in-span
    markers, Z1 and the numpy reference of the adjusted matrix; made once."""
    if (shape, nc) not in _cases:
        N, M = shape
        Z, zdrop = H.covariates(N, nc)
        z1 = Z[:, 0] if nc else H.covariates(N, 1)[0][:, 0]
        X = O.generate_markers(11, 1, N, 0, M)
        at = H.plant(X, z1, SHAPES[shape])
        inspan = sorted(at[k] for k in (("const", "zero", "cov", "affine") if nc else ("const", "zero")) if k in at)
        Z1 = H.design(Z, zdrop)
        assert np.linalg.cond(Z1) <= 10
        ref = H.residual(Z1, X.T).T
        _cases[(shape, nc)] = dict(X=X, Z=Z, zdrop=zdrop, at=at, inspan=inspan, Z1=Z1, ref=ref)
    return _cases[(shape, nc)]


def state(d):
    return {"meth": d.get_meth_data(), "mave": d.get_mave(), "msig": d.get_msig(), "stats": d.adjust_stats()}


def same_state(a, b):
    for k in ("meth", "mave", "msig"):
        assert a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), k
    assert a["stats"]["absorbed"] == b["stats"]["absorbed"] and np.array_equal(a["stats"]["flags"], b["stats"]["flags"])


# ---- read-back against numpy, and every route to the same bits -------------------------------------
@pytest.mark.parametrize("nc", CS, ids=lambda c: "C%d" % c)
@pytest.mark.parametrize("shape", list(SHAPES), ids=_ids)
def test_read_back_and_determinism(tmp_path, monkeypatch, shape, nc):
    N, M = shape
    cs = case(shape, nc)
    X, Z = cs["X"], cs["Z"]
    p = tmp_path / "x.bin"
    X.tofile(p)
    with va.Data(N, M, adjust=Z) as d:
        info = d.adjust_info()
        assert info["R"] == cs["Z1"].shape[1] == 1 + nc - int(cs["zdrop"].sum())
        assert info["dropped"].tolist() == cs["zdrop"].tolist() and info["Q"].shape == (N, info["R"])
        Qb, db = va.adjust_basis(Z)
        assert np.array_equal(info["Q"], Qb) and np.array_equal(info["dropped"], db)
        d.load_meth(X)
        got = state(d)
        # 1. against numpy
        err = np.abs(got["meth"] - cs["ref"]).max()
        rest = np.setdiff1d(np.arange(M), cs["inspan"])
        orth = np.abs(got["meth"][rest] @ info["Q"]).max()
        print("read-back %s C=%d: max |stored - lstsq residual| = %.3e, max |Q^T r| = %.3e" % (shape, nc, err, orth))
        assert err <= BAR_READBACK
        assert orth <= BAR_ORTH
        # 2. absorbed: exactly the planted in-span markers, stored as exact zeros
        assert np.flatnonzero(got["stats"]["flags"]).tolist() == cs["inspan"]
        assert got["stats"]["absorbed"] == len(cs["inspan"]) and got["stats"]["flags"].dtype == bool
        assert not got["meth"][cs["inspan"]].any()
        assert np.all(got["mave"][cs["inspan"]] == 0) and np.all(got["msig"][cs["inspan"]] == 1)
        assert np.all(np.abs(got["meth"][rest]).max(axis=1) > 1e-3)  # and nobody else
        pa, pb = cs["at"]["pair"], cs["at"]["pair"] + 1
        assert np.array_equal(got["meth"][pa], got["meth"][pb]) and got["meth"][pa].any()
        # 3. the same bits from a second load, the file, and the default chunk size (one chunk)
        d.load_meth(X)
        same_state(state(d), got)
        d.read_methylation_data(str(p))
        same_state(state(d), got)
        monkeypatch.delenv("VAMPOMI_IO_CHUNK_BYTES")
        d.load_meth(X)
        same_state(state(d), got)
        d.read_methylation_data(str(p))
        same_state(state(d), got)
    # 4. F32 holds (float) of what F64 holds
    with va.Data(N, M, adjust=Z, storage="f32") as f:
        f.load_meth(X)
        got32 = state(f)
        assert np.array_equal(got32["meth"], got["meth"].astype(np.float32).astype(np.float64))
        assert np.array_equal(got32["stats"]["flags"], got["stats"]["flags"])
        monkeypatch.setenv("VAMPOMI_IO_CHUNK_BYTES", "4096")
        f.read_methylation_data(str(p))
        same_state(state(f), got32)


@pytest.mark.parametrize("shape", list(SHAPES), ids=_ids)
def test_fp32_and_uint16_input_are_widened_then_adjusted(tmp_path, shape):
    N, M = shape
    cs = case(shape, 5)
    X32 = cs["X"].astype(np.float32)  # float-exact data
    X16 = np.rint(cs["X"] * 65536).clip(0, 65535).astype(np.uint16)
    X32.tofile(tmp_path / "x32.bin")
    for storage in ("f64", "f32"):
        with va.Data(N, M, adjust=cs["Z"], storage=storage) as d:
            d.load_meth(X32.astype(np.float64))
            want = state(d)
            d.load_meth(X32)
            same_state(state(d), want)
            d.read_methylation_data(str(tmp_path / "x32.bin"), dtype="f32")
            same_state(state(d), want)
            d.load_meth(X16.astype(np.float64) / 65536.0)
            want16 = state(d)
            d.load_meth(X16)
            same_state(state(d), want16)


def test_full_rank_R65():
    """64 independent covariates: R = 65, the widest basis."""
    N, M = 301, 9
    Z = np.random.default_rng(8).uniform(-1, 1, (N, 64))
    Z1 = H.design(Z)
    assert np.linalg.cond(Z1) <= 10
    X = O.generate_markers(12, 1, N, 0, M)
    X[4] = Z[:, 63] * 0.25 + 0.5
    with va.Data(N, M, adjust=Z) as d:
        info = d.adjust_info()
        assert info["R"] == 65 and not info["dropped"].any()
        d.load_meth(X)
        R = d.get_meth_data()
        err = np.abs(R - H.residual(Z1, X.T).T).max()
        print("R = 65: max |stored - lstsq residual| = %.3e" % err)
        assert err <= BAR_READBACK
        assert np.flatnonzero(d.adjust_stats()["flags"]).tolist() == [4] and not R[4].any()
        assert np.abs(np.delete(R, 4, axis=0) @ info["Q"]).max() <= BAR_ORTH


@pytest.mark.parametrize("storage", ["f64", "f32"])
def test_three_loopback_ranks_hold_the_bits_of_one(tmp_path, monkeypatch, storage):
    monkeypatch.setenv("VAMPOMI_COMM", "loopback")
    shape = (301, 37)
    N, M = shape
    cs = case(shape, 5)
    p = tmp_path / "x.bin"
    cs["X"].tofile(p)
    with va.Data(N, M, adjust=cs["Z"], storage=storage) as d:
        d.read_methylation_data(str(p))
        want = state(d)
    cid = os.urandom(va.UNIQUE_ID_BYTES)
    got, errs = {}, {}

    def work(r):
        try:
            with va.Data(N, M, rank=r, nranks=3, comm_id=cid, device=0, adjust=cs["Z"], storage=storage) as d:
                d.read_methylation_data(str(p))
                got[r] = (d.S, d.M, state(d))
        except BaseException as e:  # noqa: BLE001
            errs[r] = repr(e)

    th = [threading.Thread(target=work, args=(r,), daemon=True) for r in range(3)]
    [t.start() for t in th]
    [t.join(120) for t in th]
    assert not any(t.is_alive() for t in th) and not errs, errs
    parts = [got[r] for r in range(3)]
    assert [s for s, _, _ in parts] == [0, parts[0][1], parts[0][1] + parts[1][1]]
    assert np.array_equal(np.vstack([s["meth"] for _, _, s in parts]), want["meth"])
    assert np.array_equal(np.concatenate([s["stats"]["flags"] for _, _, s in parts]), want["stats"]["flags"])
    assert sum(s["stats"]["absorbed"] for _, _, s in parts) == want["stats"]["absorbed"] == 4


# ---- the contract ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def problem():
    N, Mt = 301, 517
    X = O.generate_markers(5, 1, N, 0, Mt)
    Z, _ = H.covariates(N, 5)
    H.plant(X, Z[:, 0], ("const", "zero", "cov", "affine", "pair"))
    y, beta = phen_from_markers(X, seed=5)
    y = y + Z[:, 0] * 0.7 - 0.4 * Z[:, 2] + 3.0  # the covariates act on the phenotype
    return X, y, beta, Z


@pytest.mark.parametrize("storage", ["f64", "f32"])
def test_contract_an_adjusted_context_computes_what_a_plain_one_does_on_its_read_back(problem, storage):
    X, y, beta, Z = problem
    Mt, N = X.shape
    its = 4
    with va.Data(N, Mt, adjust=Z, storage=storage) as a, va.Data(N, Mt, storage=storage) as b:
        a.load_meth(X)
        a.set_phen(y)
        stored, ya = a.get_meth_data(), a.get_phen()
        b.load_meth(stored)
        b.set_phen(ya, standardize=False)
        assert np.array_equal(b.get_meth_data(), stored) and np.array_equal(b.get_phen(), ya)
        assert b.adjust_info()["R"] == 0 and b.adjust_stats()["absorbed"] == 0 and not b.adjust_stats()["flags"].any()
        gone = np.flatnonzero(a.adjust_stats()["flags"])
        assert gone.tolist() == [0, 1, 2, 3]
        for f in ("get_mave", "get_msig"):
            assert np.array_equal(getattr(a, f)(), getattr(b, f)()), f
        runs = []
        for d in (a, b):
            v = va.Vamp(d, va.VampOptions(max_iter=its, stop_criteria_thr=0.0), true_signal=beta)
            v.infere(keep_hist=True)
            s = v.summary()
            assert s["iterations"] == its
            runs.append((v.x1_hist[:its, :Mt].copy(), v.r1_hist[:its, :Mt].copy(), s["cg_iters"], s["ons_iters"]))
        assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])
        assert runs[0][2:] == runs[1][2:] and np.any(runs[0][0] != 0)
        assert not runs[0][0][:, gone].any()  # x1_hat is exactly 0 at an absorbed marker
        est = runs[0][0][-1] / np.sqrt(N)
        (pa, sa), (pb, sb) = a.assoc_loo(est), b.assoc_loo(est)
        assert np.array_equal(pa, pb, equal_nan=True) and np.array_equal(sa, sb)


# ---- composition -------------------------------------------------------------------------------------
N_FILE, N_KEEP, M_SUB = 700, 301, 37
_rng = np.random.default_rng(20)
_must = np.array([0, 123, 699])
ROWS = np.sort(np.concatenate([_must, _rng.choice(np.setdiff1d(np.arange(N_FILE), _must), N_KEEP - 3,
                                                  replace=False)])).astype(np.int64)


@pytest.mark.parametrize("storage", ["f64", "f32"])
def test_row_subset_equals_an_adjusted_load_of_the_cut_files(tmp_path, storage):
    X = O.generate_markers(13, 1, N_FILE, 0, M_SUB)
    Z, zdrop = H.covariates(N_FILE, 5)
    H.plant(X, Z[:, 0], ("const", "zero", "cov", "affine", "pair"))
    y = np.random.default_rng(1).standard_normal(N_FILE) + Z[:, 2]
    X.tofile(tmp_path / "full.bin")
    H.write_cov(tmp_path / "full.cov", Z)
    H.write_phen(tmp_path / "full.phen", y)
    with va.Data(N_KEEP, M_SUB, adjust=np.ascontiguousarray(Z[ROWS]), storage=storage) as q:
        q.load_meth(np.ascontiguousarray(X[:, ROWS]))
        q.set_phen(y[ROWS])
        want, ywant, qinfo = state(q), q.get_phen(), q.adjust_info()
    assert want["stats"]["absorbed"] == 4
    for how in ("array", "file"):
        kw = dict(adjust=np.ascontiguousarray(Z[ROWS])) if how == "array" else dict(adjust=str(tmp_path / "full.cov"),
                                                                                     adjust_C=5)
        with va.Data(N_FILE, M_SUB, rows=ROWS, storage=storage, **kw) as d:
            assert np.array_equal(d.adjust_info()["Q"], qinfo["Q"]) and d.adjust_info()["dropped"].tolist() == zdrop.tolist()
            if how == "array":
                d.load_meth(X)
                d.set_phen(y[ROWS])
            else:
                d.read_methylation_data(str(tmp_path / "full.bin"))
                d.read_phen(str(tmp_path / "full.phen"))
            same_state(state(d), want)
            assert np.array_equal(d.get_phen(), ywant)


@pytest.mark.parametrize("storage", ["f64", "f32"])
def test_meth_na_mean_equals_adjusting_the_filled_matrix(storage):
    shape = (301, 37)
    N, M = shape
    cs = case(shape, 5)
    Xin = cs["X"].copy()
    Xin[10, ::7] = np.nan
    Xin[11, 5] = np.nan
    Xin[12, :] = np.nan  # no observed entry: masked, stored as zeros before the adjustment, absorbed by it
    Xin[cs["at"]["cov"], 3] = np.nan  # its fill takes this marker out of the covariates' span
    with va.Data(N, M, meth_na="mean") as m:  # (F64: the fill is formed and adjusted in fp64 whatever the storage)
        m.load_meth(Xin)
        filled = m.get_meth_data()
    assert not np.isnan(filled).any() and not filled[12].any()
    with va.Data(N, M, adjust=cs["Z"], storage=storage) as q:
        q.load_meth(filled)
        want = state(q)
    with va.Data(N, M, adjust=cs["Z"], storage=storage, meth_na="mean") as d:
        d.load_meth(Xin)
        got = state(d)
        assert d.missing_stats() == {"missing": 43 + 1 + 301 + 1, "markers_with_missing": 4, "markers_masked": 1}
    same_state(got, want)
    gone = np.flatnonzero(got["stats"]["flags"]).tolist()
    assert 12 in gone and cs["at"]["cov"] not in gone and gone == sorted(set(cs["inspan"]) - {cs["at"]["cov"]} | {12})


# ---- the phenotype -----------------------------------------------------------------------------------
@pytest.mark.parametrize("nc", CS, ids=lambda c: "C%d" % c)
def test_phenotype_is_projected_then_scaled(tmp_path, nc):
    N, M = 301, 4
    Z, zdrop = H.covariates(N, nc)
    Z1 = H.design(Z, zdrop)
    rng = np.random.default_rng(4)
    y = rng.standard_normal(N) + 2.0 + (Z[:, 0] * 1.5 if nc else 0.0)
    want = H.residual(Z1, y)
    H.write_phen(tmp_path / "y.phen", y)
    with va.Data(N, M, adjust=Z) as d:
        d.set_phen(y, standardize=False)
        got = d.get_phen()
        rel = np.linalg.norm(got - want) / np.linalg.norm(want)
        print("phenotype C=%d: relative error %.3e" % (nc, rel))
        assert rel <= BAR_PHEN
        d.set_phen(y, standardize=True)
        scaled = d.get_phen()
        assert np.allclose(scaled, O.standardize_phen(got.copy()), rtol=BAR_PHEN, atol=0)
        with va.Data(N, M) as q:  # the scaling is the plain context's own, applied to the projected vector
            q.set_phen(got, standardize=True)
            assert np.array_equal(q.get_phen(), scaled)
        d.read_phen(str(tmp_path / "y.phen"), standardize=True)
        assert np.array_equal(d.get_phen(), scaled)
        # inside the span: nothing is left
        g = rng.standard_normal(Z1.shape[1])
        yin = Z1 @ g
        d.set_phen(yin, standardize=False)
        left = np.linalg.norm(d.get_phen()) / np.linalg.norm(yin)
        print("phenotype C=%d: |P y| / |y| = %.3e for y in the span" % (nc, left))
        assert left < 1e-12


# ---- guards ------------------------------------------------------------------------------------------
def _status(fn, *a, **k):
    with pytest.raises(va.VampomiError) as e:
        fn(*a, **k)
    return e.value.status


def test_guards():
    import ctypes as C

    lib = va.load()
    N, M = 301, 6
    Z, _ = H.covariates(N, 5)
    Zc = np.ascontiguousarray(Z.T)
    zp = Zc.ctypes.data_as(C.c_void_p)
    X = O.generate_markers(3, 1, N, 0, M)
    y = np.random.default_rng(2).integers(0, 2, N).astype(np.float64)
    with va.Data(N, M) as d:
        assert _status(d.adjust_stats) == ERR_STATE  # before a load
        assert d.adjust_info()["R"] == 0
        assert lib.vampomi_set_adjust(d.ctx, zp, 65, N) == ERR_ARG and lib.vampomi_set_adjust(d.ctx, zp, -1, N) == ERR_ARG
        assert lib.vampomi_set_adjust(d.ctx, zp, 5, N - 1) == ERR_ARG and lib.vampomi_set_adjust(d.ctx, None, 5, N) == ERR_ARG
        assert d.adjust_info()["R"] == 0  # a refusal changes nothing
        d.set_phen(y)
        assert lib.vampomi_set_adjust(d.ctx, zp, 5, N) == ERR_STATE  # after the phenotype
        assert b"before the phenotype" in lib.vampomi_last_error()
    with va.Data(N, M) as d:
        d.load_meth(X)
        assert lib.vampomi_set_adjust(d.ctx, zp, 5, N) == ERR_STATE  # after the shard is allocated
        assert d.adjust_info()["R"] == 0 and d.adjust_stats()["absorbed"] == 0
    with va.Data(N, M, storage="u16") as d:
        assert lib.vampomi_set_adjust(d.ctx, zp, 5, N) == ERR_ARG  # residuals leave [0, 1]
    with pytest.raises(va.VampomiError) as e:
        va.Data(N, M, storage="u16", adjust=Z)
    assert e.value.status == ERR_ARG
    with va.Data(N, M, adjust=Z) as d:
        assert lib.vampomi_set_storage(d.ctx, va.STORE_U16) == ERR_ARG
        assert lib.vampomi_set_storage(d.ctx, va.STORE_F32) == 0 and d.storage == "f32"
        rows = np.arange(N, dtype=np.int64)
        assert lib.vampomi_set_row_subset(d.ctx, N + 5, rows.ctypes.data_as(C.c_void_p), N) == ERR_STATE  # subset first
        assert _status(d.generate, 7, va.GEN_METH) == ERR_STATE
        assert _status(d.get_meth_data) == ERR_STATE  # (nothing was generated)
        d.load_meth(X)
        d.set_phen(y, standardize=False)
        v = va.Vamp(d, va.VampOptions(max_iter=2, model="bin_class"))
        assert _status(v.infere) == ERR_STATE  # the probit model has its own covariates
        assert _status(v.begin) == ERR_STATE
        va.Vamp(d, va.VampOptions(max_iter=2, stop_criteria_thr=0.0)).infere()  # the linear model runs
    with va.Data(N, M, adjust=np.empty((N, 0))) as d:  # C == 0: the intercept only
        assert d.adjust_info()["R"] == 1 and d.adjust_info()["dropped"].shape == (0,)
        k = np.rint(X * 65536).clip(0, 65535).astype(np.uint16)
        d.load_meth(k)  # uint16 input into F64 storage: widened, then adjusted
        assert np.abs(d.get_meth_data().sum(axis=1)).max() < 1e-10
    with pytest.raises(ValueError):
        va.Data(N, M, adjust=np.ones((N + 1, 2)))


# ---- no adjustment: nothing changes ------------------------------------------------------------------
def test_without_an_adjustment_a_load_and_a_run_are_what_they_are(problem):
    X, y, beta, _ = problem
    Mt, N = X.shape
    runs = []
    for kw in ({}, dict(adjust=None)):
        with va.Data(N, Mt, **kw) as d:
            d.load_meth(X)
            d.set_phen(y)
            assert np.array_equal(d.get_meth_data(), X)  # a plain F64 load is a copy
            assert d.adjust_info()["R"] == 0 and d.adjust_stats()["absorbed"] == 0
            assert not d.adjust_stats()["flags"].any()
            v = va.Vamp(d, va.VampOptions(max_iter=2, stop_criteria_thr=0.0), true_signal=beta)
            v.infere(keep_hist=True)
            runs.append((v.x1_hist[:2, :Mt].copy(), v.r1_hist[:2, :Mt].copy(), v.summary()["cg_iters"]))
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1]) and runs[0][2] == runs[1][2]
    assert np.any(runs[0][0] != 0)


# ---- the CLI: infere, association_test, test ---------------------------------------------------------
def _run(cmd):
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    return r.stdout


def _same_files(a, b):
    names = sorted(f for f in os.listdir(a) if not f.startswith("."))
    assert names and names == sorted(f for f in os.listdir(b) if not f.startswith("."))
    for f in names:
        assert (a / f).read_bytes() == (b / f).read_bytes(), f
    return names


def test_cli_residual_writes_what_a_plain_run_on_the_adjusted_files_writes(tmp_path):
    shape = (301, 37)
    N, M = shape
    cs = case(shape, 5)
    X, Z = cs["X"], cs["Z"]
    y, beta = phen_from_markers(X, seed=5)
    y = y + 0.7 * Z[:, 0] + 1.0
    t = tmp_path
    X.astype("<f8").tofile(t / "raw.bin")
    H.write_cov(t / "z.cov", Z)
    H.write_phen(t / "raw.phen", y)
    beta.astype("<f8").tofile(t / "ts.bin")
    with va.Data(N, M, adjust=str(t / "z.cov"), adjust_C=5) as d:
        d.read_methylation_data(str(t / "raw.bin"))
        d.read_phen(str(t / "raw.phen"), standardize=False)
        d.get_meth_data().astype("<f8").tofile(t / "adj.bin")
        H.write_phen(t / "adj.phen", d.get_phen())
    base = ["--N", str(N), "--Mt", str(M), "--out-name", "ex"]
    adj = ["--cov-adjust", "residual", "--C", "5"]
    a, b = t / "a", t / "b"
    a.mkdir(), b.mkdir()
    run = ["--iterations", "3", "--stop-criteria-thr", "0", "--true-signal-file", str(t / "ts.bin")]
    out = _run([va.CLI_PATH, *base, "--meth-file", str(t / "raw.bin"), "--phen-file", str(t / "raw.phen"), "--out-dir",
                str(a), *run, *adj, "--cov-file", str(t / "z.cov")])
    assert "INFO   : adjusting for 2 of 5 covariates + intercept (dropped: 1, 3, 4)" in out.splitlines(), out[-3000:]
    assert "INFO   : markers [0, 37): 4 absorbed by the covariates" in out.splitlines(), out[-3000:]
    assert "are ignored" not in out
    out = _run([va.CLI_PATH, *base, "--meth-file", str(t / "adj.bin"), "--phen-file", str(t / "adj.phen"), "--out-dir",
                str(b), *run])
    assert "adjusting for" not in out and "absorbed" not in out
    names = _same_files(a, b)
    assert sum(f.endswith(".bin") and "_it_" in f for f in names) == 2 * 3, names
    x1 = np.fromfile(a / "ex_it_3.bin", dtype="<f8")
    assert x1.shape == (M,) and np.any(x1 != 0) and not x1[cs["inspan"]].any()
    # association_test on the estimate just written
    a2, b2 = t / "a2", t / "b2"
    a2.mkdir(), b2.mkdir()
    loo = ["--run-mode", "association_test", "--pval-method", "loo", "--estimate-file", str(a / "ex_it_3.bin")]
    _run([va.CLI_PATH, *base, "--meth-file", str(t / "raw.bin"), "--phen-file", str(t / "raw.phen"), "--out-dir",
          str(a2), *loo, *adj, "--cov-file", str(t / "z.cov")])
    _run([va.CLI_PATH, *base, "--meth-file", str(t / "adj.bin"), "--phen-file", str(t / "adj.phen"), "--out-dir",
          str(b2), *loo])
    assert _same_files(a2, b2) == ["ex_it_3_pval_loo.bin"]
    # test mode: the test set's own table
    a3, b3 = t / "a3", t / "b3"
    a3.mkdir(), b3.mkdir()
    tm = ["--run-mode", "test", "--N-test", str(N), "--estimate-file", str(a / "ex_it_1.bin"), "--test-iter-range", "1,3"]
    out = _run([va.CLI_PATH, *base, "--meth-file-test", str(t / "raw.bin"), "--phen-file-test", str(t / "raw.phen"),
                "--out-dir", str(a3), *tm, *adj, "--cov-file-test", str(t / "z.cov")])
    assert "INFO   : adjusting for 2 of 5 covariates + intercept (dropped: 1, 3, 4)" in out.splitlines()
    _run([va.CLI_PATH, *base, "--meth-file-test", str(t / "adj.bin"), "--phen-file-test", str(t / "adj.phen"),
          "--out-dir", str(b3), *tm])
    assert _same_files(a3, b3) == ["ex_test.csv"]
    assert len((a3 / "ex_test.csv").read_bytes().splitlines()) == 4
