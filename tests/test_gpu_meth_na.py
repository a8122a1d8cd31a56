"""Missing methylation values (NaN) on the device: vampomi_set_meth_na, the
policies pass / fatal / mean, --meth-na and --meth-na-max-frac.

The bars of this file:
  * read-back: under "mean" an observed entry is stored as a plain context of
    the same storage stores it (bit-equal), a missing one as the marker's mean:
    with m the exact mean (math.fsum) and gamma = (n_obs + 1) 2^-53 mean|x_obs|,
    the first-order bound of any-order fp64 summation plus one division, the
    stored fill lies in [conv(m - gamma), conv(m + gamma)] (tests/_meth_na.py);
  * determinism: the stored bits do not depend on the chunk size, on file or
    host, or on the load;
  * contract: a "mean" context computes, bit for bit, what a plain context of
    the same storage computes after loading its get_meth_data().
Everything else is np.array_equal or integer equality.

Shapes (N odd, the smallest that reach each part of the 256-thread column
kernel): 301 x 37 with VAMPOMI_IO_CHUNK_BYTES=4096 (one fp64 or three fp32
columns per chunk: the chunk boundaries fall between markers, and the last
thread rows are ragged), 4099 x 23 (several rows per lane, 17 sweeps) and
70001 x 5 (274 sweeps).  Planted patterns, one per marker (tests/_meth_na.py):
none, row 0, row N-1, runs of 64 and 65 rows, every second row, all but one
row, all rows, negative / payload / signalling NaNs, the rest 0.5 % at random.
"""
import os
import subprocess
import threading

import numpy as np
import pytest

import _meth_na as H
from _data import phen_from_markers

pytestmark = pytest.mark.gpu

va = pytest.importorskip("vampomi_amd")
from oracle import pyoracle as O  # noqa: E402  (the index-keyed generator only)

SHAPES = {(301, 37): None, (4099, 23): None,
          (70001, 5): ("ends", "alternate", "all_but_one", "payload", "random")}  # five markers: the long-column ones
DT = {"f64": np.float64, "f32": np.float32}
STORAGES = ("f64", "f32", "u16")
ERR_STATE, ERR_RANGE, ERR_NAN_METH = 6, 9, 10
FILLER = 0.5  # in range, on the 2^-16 grid and a float: stored exactly, never clamped


def _ids(s):
    return "N%d_M%d" % s


@pytest.fixture(autouse=True)
def _small_chunks(monkeypatch):
    monkeypatch.setenv("VAMPOMI_IO_CHUNK_BYTES", "4096")
    monkeypatch.setenv("VAMPOMI_IO_THREADS", "3")


@pytest.fixture(scope="module")
def planted():
    """(shape, intype) -> (Xin with NaNs, mask); the generator's methylation-like
    values, made once per shape."""
    base, made = {}, {}

    def get(shape, intype):
        if shape not in base:
            N, M = shape
            base[shape] = (O.generate_markers(11, 1, N, 0, M), H.plant_mask(N, M, SHAPES.get(shape)))
        if (shape, intype) not in made:
            X, mask = base[shape]
            made[(shape, intype)] = (H.with_nans(X, mask, DT[intype]), mask)
        return made[(shape, intype)]

    return get


def state(d):
    return {"meth": d.get_meth_data(), "mave": d.get_mave(), "msig": d.get_msig(), "quant": d.quant_stats(),
            "stats": d.missing_stats(), "counts": d.missing_counts()}


def same_state(a, b, keys=("meth", "mave", "msig", "counts")):
    for k in keys:
        assert a[k].shape == b[k].shape and np.array_equal(a[k], b[k], equal_nan=True), k
    assert a["quant"] == b["quant"] and a["stats"] == b["stats"], (a["quant"], b["quant"], a["stats"], b["stats"])


@pytest.fixture(scope="module")
def plain_state():
    """(shape, intype, storage) -> the state of a plain context loaded from the
    host with the NaNs replaced by FILLER; made once and shared."""
    made = {}

    def get(key, Xin):
        if key not in made:
            N, M = key[0]
            with va.Data(N, M, storage=key[2]) as d:
                d.load_meth(np.where(np.isnan(Xin), DT[key[1]](FILLER), Xin))
                made[key] = state(d)
        return made[key]

    return get


def load(d, Xin, source, tmp_path, intype):
    if source == "host":
        d.load_meth(Xin)
    else:
        p = tmp_path / f"x_{intype}.bin"
        if not p.exists():
            Xin.tofile(p)
        d.read_methylation_data(str(p), dtype=intype)


# ---- 1. read-back, 2. determinism, 4. counts ---------------------------------------------------
_first_bits = {}  # (shape, intype, storage) -> the first read-back: every later load must give these bits


@pytest.mark.parametrize("source", ["host", "file"])
@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("intype", ["f64", "f32"])
@pytest.mark.parametrize("shape", list(SHAPES), ids=_ids)
def test_mean_fills_counts_and_is_deterministic(tmp_path, monkeypatch, planted, plain_state, shape, intype, storage,
                                                source):
    N, M = shape
    Xin, mask = planted(shape, intype)
    plain = plain_state((shape, intype, storage), Xin)
    with va.Data(N, M, storage=storage, meth_na="mean") as d:
        assert d.meth_na == "mean" and d.max_missing_frac == 1.0
        load(d, Xin, source, tmp_path, intype)
        got = state(d)
        ref = H.check_filled(got["meth"], plain["meth"], Xin, storage)
        # exact integers
        assert got["stats"] == ref["stats"] and got["counts"].dtype == np.int64
        assert np.array_equal(got["counts"], ref["counts"]) and np.array_equal(ref["counts"], mask.sum(axis=1))
        assert ref["stats"]["markers_masked"] == (0 if shape == (70001, 5) else 1)  # the all-missing marker alone
        # the quantisation record is that of the observed entries alone
        assert got["quant"] == plain["quant"]
        if storage == "u16":
            assert got["quant"]["max_abs_err"] > 0
        # the statistics are those of the filled column
        assert not np.isnan(got["mave"]).any() and not np.isnan(got["msig"]).any()
        # determinism: the same bits from file and host (whichever came first), after a second load, and with
        # the default chunk size (one chunk)
        first = _first_bits.setdefault((shape, intype, storage), got["meth"])
        assert np.array_equal(got["meth"], first)
        load(d, Xin, source, tmp_path, intype)
        same_state(state(d), got)
        monkeypatch.delenv("VAMPOMI_IO_CHUNK_BYTES")
        load(d, Xin, source, tmp_path, intype)
        same_state(state(d), got)


def test_fill_is_exact_where_the_mean_is():
    """Dyadic values whose every partial sum is exact: any order gives the mean
    itself, so the fill is pinned to the bit on every storage."""
    N, M = 301, 3
    X = ((np.arange(N * M).reshape(M, N) * 37) % 256) / 256.0
    mask = H.plant_mask(N, M, ("alternate", "runs", "payload"))
    Xin = H.with_nans(X, mask, np.float64)
    for storage in STORAGES:
        with va.Data(N, M, storage=storage, meth_na="mean") as d:
            d.load_meth(Xin)
            R = d.get_meth_data()
        for i in range(M):
            want = H.conv(np.float64(sum(int(v * 256) for v in X[i][~mask[i]])) / 256 / int((~mask[i]).sum()), storage)
            assert np.all(R[i][mask[i]] == want), (storage, i)


@pytest.mark.parametrize("frac,masked", [(0.0, [1, 2, 3, 4, 5, 6, 7] + list(range(8, 37))),
                                          (0.45, [4, 5, 6]), (129 / 301, [4, 5, 6]), (0.4, [3, 4, 5, 6]),
                                          (1.0, [6])], ids=["0", "0.45", "at_the_count", "0.4", "1"])
def test_max_missing_frac(planted, plain_state, frac, masked):
    """0.0, 1.0 and values that split the planted markers: the runs marker has
    129 of 301 missing, which is more than 0.4 of them and not more than
    129/301 or 0.45 of them."""
    shape = (301, 37)
    Xin, mask = planted(shape, "f64")
    plain = plain_state((shape, "f64", "u16"), Xin)
    with va.Data(*shape, storage="u16", meth_na="mean", max_missing_frac=frac) as d:
        assert d.max_missing_frac == frac
        d.load_meth(Xin)
        got = state(d)
    ref = H.check_filled(got["meth"], plain["meth"], Xin, "u16", frac)
    assert np.flatnonzero(ref["masked"]).tolist() == masked
    assert got["stats"] == ref["stats"] and got["stats"]["markers_masked"] == len(masked)
    assert np.array_equal(got["counts"], mask.sum(axis=1))  # a masked marker's true count
    assert np.all(got["mave"][masked] == 0) and np.all(got["msig"][masked] == 1)
    assert not got["meth"][masked].any()
    assert got["quant"] == plain["quant"]  # the observed entries of a masked marker are still checked and counted


# ---- 3. the contract -----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def problem():
    N, Mt = 301, 517
    X = O.generate_markers(5, 1, N, 0, Mt)
    y, beta = phen_from_markers(X, seed=5)
    return X, y, beta, H.plant_mask(N, Mt)


@pytest.mark.parametrize("storage", STORAGES)
def test_contract_a_mean_context_computes_what_a_plain_one_does_on_its_read_back(problem, storage):
    X, y, beta, mask = problem
    Mt, N = X.shape
    its = 3
    Xin = H.with_nans(X, mask, np.float64)
    with va.Data(N, Mt, storage=storage, meth_na="mean", max_missing_frac=0.4) as a, \
            va.Data(N, Mt, storage=storage) as b:
        a.load_meth(Xin)
        filled = a.get_meth_data()
        assert not np.isnan(filled).any()
        b.load_meth(filled)
        assert np.array_equal(b.get_meth_data(), filled)
        masked = np.flatnonzero(H.fill_reference(Xin, 0.4)["masked"])
        assert masked.tolist() == [3, 4, 5, 6] and a.missing_stats()["markers_masked"] == 4
        assert b.missing_stats() == {"missing": 0, "markers_with_missing": 0, "markers_masked": 0}
        for f in ("get_mave", "get_msig"):
            assert np.array_equal(getattr(a, f)(), getattr(b, f)()), f
        assert np.all(a.get_mave()[masked] == 0) and np.all(a.get_msig()[masked] == 1)
        rng = np.random.default_rng(3)
        x, u = rng.standard_normal(Mt), rng.standard_normal(N)
        assert np.array_equal(a.Ax(x), b.Ax(x)) and np.any(a.Ax(x) != 0)
        assert np.array_equal(a.ATx(u), b.ATx(u)) and np.all(a.ATx(u)[masked] == 0)
        runs = []
        for d in (a, b):
            d.set_phen(y)
            v = va.Vamp(d, va.VampOptions(max_iter=its, stop_criteria_thr=0.0), true_signal=beta)
            v.infere(keep_hist=True)
            s = v.summary()
            assert s["iterations"] == its
            runs.append((v.x1_hist[:its, :Mt].copy(), v.r1_hist[:its, :Mt].copy(), s["cg_iters"], s["ons_iters"]))
        assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])
        assert runs[0][2:] == runs[1][2:] and np.any(runs[0][0] != 0)
        assert not runs[0][0][:, masked].any()  # x1_hat is exactly 0 at a masked marker
        est = runs[0][0][-1] / np.sqrt(N)
        (pa, sa), (pb, sb) = a.assoc_loo(est), b.assoc_loo(est)
        assert np.array_equal(pa, pb, equal_nan=True) and np.array_equal(sa, sb)


# ---- 5. fatal ---------------------------------------------------------------------------------------
def _raises(d, X, status):
    with pytest.raises(va.VampomiError) as e:
        d.load_meth(X)
    assert e.value.status == status, str(e.value)
    with pytest.raises(va.VampomiError) as e2:
        d.get_meth_data()
    assert e2.value.status == ERR_STATE  # the context is left without a shard
    return str(e.value)


@pytest.mark.parametrize("intype", ["f64", "f32"])
@pytest.mark.parametrize("storage", STORAGES)
def test_fatal_names_the_count_and_the_first_global_marker(tmp_path, monkeypatch, planted, storage, intype):
    """Two loopback ranks read their shards of one file: rank 0 (markers [0, 19))
    is clean and loads, rank 1 (markers [19, 37)) fails and names GLOBAL markers."""
    monkeypatch.setenv("VAMPOMI_COMM", "loopback")
    N, M = 301, 37
    X = planted((N, M), intype)[0]
    X = np.where(np.isnan(X), DT[intype](FILLER), X)
    mask = np.zeros((M, N), dtype=bool)
    mask[25, [7, 100]] = True  # the smallest index is (25, 7), not the first found in memory order of a later chunk
    mask[30, 2] = True
    Xb = H.with_nans(X, mask, DT[intype])
    p = tmp_path / "x.bin"
    Xb.tofile(p)
    cid = os.urandom(va.UNIQUE_ID_BYTES)
    got, errs = {}, {}

    def work(r):
        try:
            with va.Data(N, M, rank=r, nranks=2, comm_id=cid, device=0, storage=storage, meth_na="fatal") as d:
                try:
                    d.read_methylation_data(str(p), dtype=intype)
                    got[r] = (d.S, d.get_meth_data(), d.missing_stats(), d.missing_counts())
                except va.VampomiError as e:
                    errs[r] = (e.status, str(e))
                    try:
                        d.get_meth_data()
                    except va.VampomiError as e2:
                        errs[r] += (e2.status,)
        except BaseException as e:  # noqa: BLE001
            errs[r] = ("crash", repr(e))

    th = [threading.Thread(target=work, args=(r,), daemon=True) for r in range(2)]
    [t.start() for t in th]
    [t.join(120) for t in th]
    assert not any(t.is_alive() for t in th)
    assert list(errs) == [1] and list(got) == [0], (errs, list(got))
    status, msg, after = errs[1]
    assert status == ERR_NAN_METH and after == ERR_STATE, errs
    assert msg == "ERR_NAN_METH: 3 missing methylation value(s) (NaN); the first is marker 25, row 7", msg
    S, meth, stats, counts = got[0]
    assert S == 0 and stats == {"missing": 0, "markers_with_missing": 0, "markers_masked": 0} and not counts.any()
    with va.Data(N, 19, storage=storage) as q:  # a clean shard under fatal is stored as a plain context stores it
        q.load_meth(np.ascontiguousarray(X[:19]))
        assert np.array_equal(meth, q.get_meth_data())


@pytest.mark.parametrize("intype", ["f64", "f32"])
def test_fatal_on_u16_nan_is_10_and_out_of_range_is_9(planted, intype):
    N, M = 301, 37
    X = planted((N, M), intype)[0]
    X = np.where(np.isnan(X), DT[intype](FILLER), X)
    nan_only, range_only, both = X.copy(), X.copy(), X.copy()
    nan_only[20, 300] = np.nan
    range_only[3, 5] = 1.5
    range_only[36, 0] = np.inf  # an infinity is a value: out of range, not missing
    both[3, 5] = 1.5
    both[20, 300] = np.nan
    with va.Data(N, M, storage="u16", meth_na="fatal") as d:
        assert d.meth_na == "fatal"
        assert "1 missing methylation value(s) (NaN); the first is marker 20, row 300" in _raises(d, nan_only,
                                                                                               ERR_NAN_METH)
        msg = _raises(d, range_only, ERR_RANGE)
        assert "marker 3, row 5" in msg and msg.split(": ", 1)[1].startswith("2 "), msg
        assert "marker 20, row 300" in _raises(d, both, ERR_NAN_METH)  # of the two, the NaN is reported
        d.load_meth(X)  # the context is reusable
        with va.Data(N, M, storage="u16") as q:
            q.load_meth(X)
            same_state(state(d), state(q))


# ---- 6. row subset -----------------------------------------------------------------------------------
N_FILE, N_KEEP, M_SUB = 700, 301, 37
_rng = np.random.default_rng(20)
_must = np.array([0, 123, 699])
ROWS = np.sort(np.concatenate([_must, _rng.choice(np.setdiff1d(np.arange(N_FILE), _must), N_KEEP - 3,
                                                  replace=False)])).astype(np.int64)
DROPPED = np.setdiff1d(np.arange(N_FILE), ROWS)


@pytest.fixture(scope="module")
def X700():
    return O.generate_markers(13, 1, N_FILE, 0, M_SUB)


@pytest.mark.parametrize("source", ["host", "file"])
@pytest.mark.parametrize("intype,storage", [("f64", "f64"), ("f64", "u16"), ("f32", "f32"), ("f32", "u16")])
def test_row_subset_nans_in_dropped_rows_are_not_seen(tmp_path, X700, intype, storage, source):
    mask = np.zeros((M_SUB, N_FILE), dtype=bool)
    mask[:, DROPPED[::3]] = True  # every marker, dropped rows only
    mask[4, DROPPED] = True
    Xin = H.with_nans(X700, mask, DT[intype])
    with va.Data(N_KEEP, M_SUB, storage=storage) as q:
        q.load_meth(np.ascontiguousarray(Xin[:, ROWS]))
        want = state(q)
    for policy in ("fatal", "mean"):
        with va.Data(N_FILE, M_SUB, storage=storage, rows=ROWS, meth_na=policy) as d:
            load(d, Xin, source, tmp_path, intype)
            got = state(d)
        same_state(got, want)
        assert got["stats"] == {"missing": 0, "markers_with_missing": 0, "markers_masked": 0}


@pytest.mark.parametrize("source", ["host", "file"])
@pytest.mark.parametrize("intype,storage", [("f64", "f64"), ("f64", "u16"), ("f32", "f32"), ("f32", "f64")])
def test_row_subset_mean_equals_mean_of_the_taken_rows(tmp_path, X700, intype, storage, source):
    mask = np.zeros((M_SUB, N_FILE), dtype=bool)
    mask[:, ROWS] = H.plant_mask(N_KEEP, M_SUB)  # the planted patterns over the kept rows ...
    mask[:, DROPPED[1::2]] = True  # ... and NaNs in dropped rows of every marker
    Xin = H.with_nans(X700, mask, DT[intype])
    with va.Data(N_KEEP, M_SUB, storage=storage, meth_na="mean", max_missing_frac=0.45) as q:
        q.load_meth(np.ascontiguousarray(Xin[:, ROWS]))
        want = state(q)
    with va.Data(N_FILE, M_SUB, storage=storage, rows=ROWS, meth_na="mean", max_missing_frac=0.45) as d:
        load(d, Xin, source, tmp_path, intype)
        got = state(d)
    same_state(got, want)
    assert np.array_equal(got["counts"], mask[:, ROWS].sum(axis=1))  # the kept rows' alone
    assert got["stats"]["markers_masked"] == 3 and got["stats"]["missing"] == int(mask[:, ROWS].sum())


def test_row_subset_fatal_names_the_file_row(X700):
    Xb = X700.copy()
    Xb[5, 123] = np.nan  # a kept row
    Xb[5, DROPPED[0]] = np.nan  # an earlier dropped row: neither named nor counted
    Xb[9, 699] = np.nan
    assert DROPPED[0] < 123 and 123 in ROWS
    with va.Data(N_FILE, M_SUB, rows=ROWS, meth_na="fatal") as d:
        msg = _raises(d, Xb, ERR_NAN_METH)
    assert msg == "ERR_NAN_METH: 2 missing methylation value(s) (NaN); the first is marker 5, row 123", msg


# ---- 7. pass, and the setter's arguments ---------------------------------------------------------------
@pytest.mark.parametrize("storage", ["f64", "f32"])
def test_pass_set_explicitly_is_the_default(planted, storage):
    N, M = 301, 37
    Xin = planted((N, M), "f64")[0]
    with va.Data(N, M, storage=storage, meth_na="pass") as d, va.Data(N, M, storage=storage) as q:
        assert d.meth_na == q.meth_na == "pass"
        d.load_meth(Xin)
        q.load_meth(Xin)
        a, b = state(d), state(q)
        same_state(a, b)  # (NaNs included, wherever they are)
        assert a["stats"] == {"missing": 0, "markers_with_missing": 0, "markers_masked": 0} and not a["counts"].any()


def test_generated_and_uint16_shards_have_zero_counts(planted):
    N, M = 301, 37
    for policy in ("fatal", "mean"):
        with va.Data(N, M, storage="u16", meth_na=policy) as d:
            d.generate(7, va.GEN_METH)
            assert d.missing_stats()["missing"] == 0 and not d.missing_counts().any()
            k = (d.get_meth_data() * 65536).astype(np.uint16)
            if policy == "mean":
                d.load_meth(H.with_nans(k / 65536.0, H.plant_mask(N, M), np.float64))
                assert d.missing_stats()["missing"] > 0
            d.load_meth(k)  # uint16 input has no missing code: nobody looks, and the last load's counts are gone
            assert d.missing_stats() == {"missing": 0, "markers_with_missing": 0, "markers_masked": 0}
            assert not d.missing_counts().any() and np.array_equal((d.get_meth_data() * 65536).astype(np.uint16), k)


def test_setter_argument_and_state_errors(planted):
    import ctypes as C

    lib = va.load()
    N, M = 301, 37
    with va.Data(N, M) as d:
        for policy, frac in ((3, 1.0), (-1, 1.0), (2, -0.01), (2, 1.01), (2, float("nan")), (1, 2.0)):
            assert lib.vampomi_set_meth_na(d.ctx, policy, frac) == 1, (policy, frac)
        assert d.meth_na == "pass" and d.max_missing_frac == 1.0  # a refusal changes nothing
        with pytest.raises(va.VampomiError) as e:
            d.missing_stats()
        assert e.value.status == ERR_STATE  # before a load
        assert lib.vampomi_set_meth_na(d.ctx, 2, 0.25) == 0 and lib.vampomi_set_meth_na(d.ctx, 2, 0.0) == 0
        assert (d.meth_na, d.max_missing_frac) == ("mean", 0.0)
        p, f = C.c_int(-1), C.c_double(-1)
        assert lib.vampomi_get_meth_na(d.ctx, C.byref(p), None) == 0 and p.value == 2
        assert lib.vampomi_get_meth_na(d.ctx, None, C.byref(f)) == 0 and f.value == 0.0
        d.load_meth(planted((N, M), "f64")[0])
        assert lib.vampomi_set_meth_na(d.ctx, 0, 1.0) == ERR_STATE  # the shard is allocated
        assert b"NaN policy" in lib.vampomi_last_error() and d.meth_na == "mean"
        a, b, c = C.c_int64(-1), C.c_int64(-1), C.c_int64(-1)
        assert lib.vampomi_get_missing_stats(d.ctx, C.byref(a), C.byref(b), C.byref(c), None) == 0
        assert (a.value, b.value, c.value) == (int(planted((N, M), "f64")[1].sum()), 36, 36)  # 0.0 masks them all
    with pytest.raises(ValueError):
        va.Data(N, M, meth_na="median")


# ---- 8. the CLI, one process --------------------------------------------------------------------------
def _phen_text(y):
    return "".join("f%d i%d %0.10f\n" % (i, i, v) for i, v in enumerate(y))


@pytest.fixture(scope="module")
def cli_files(tmp_path_factory, problem):
    X, y, beta, mask = problem
    t = tmp_path_factory.mktemp("na_cli")
    Xin = H.with_nans(X, mask, np.float64)
    Xin.astype("<f8").tofile(t / "nan.bin")
    with va.Data(*X.shape[::-1], meth_na="mean", max_missing_frac=0.4) as d:
        d.read_methylation_data(str(t / "nan.bin"))
        d.get_meth_data().astype("<f8").tofile(t / "filled.bin")
        stats = d.missing_stats()
    (t / "y.phen").write_text(_phen_text(y))
    beta.astype("<f8").tofile(t / "ts.bin")
    return t, stats


def _cli(t, out, meth, *extra):
    out.mkdir()
    cmd = [va.CLI_PATH, "--meth-file", str(t / meth), "--phen-file", str(t / "y.phen"), "--N", "301", "--Mt", "517",
           "--out-dir", str(out), "--out-name", "ex", "--iterations", "3", "--stop-criteria-thr", "0",
           "--true-signal-file", str(t / "ts.bin"), *extra]
    return subprocess.run(cmd, capture_output=True, text=True, timeout=300)


def test_cli_mean_writes_what_a_plain_run_on_the_filled_file_writes(cli_files, tmp_path):
    t, stats = cli_files
    a = _cli(t, tmp_path / "mean", "nan.bin", "--meth-na", "mean", "--meth-na-max-frac", "0.4")
    b = _cli(t, tmp_path / "plain", "filled.bin")
    assert a.returncode == 0 and b.returncode == 0, a.stdout[-3000:] + b.stdout[-3000:]
    assert stats["markers_masked"] == 4
    line = "INFO   : markers [0, 517): %d missing values in %d markers, %d masked" % (
        stats["missing"], stats["markers_with_missing"], stats["markers_masked"])
    assert line in a.stdout.splitlines(), a.stdout[-3000:]
    assert "missing values" not in b.stdout
    names = sorted(f for f in os.listdir(tmp_path / "mean") if not f.startswith("."))
    assert names == sorted(f for f in os.listdir(tmp_path / "plain") if not f.startswith("."))
    assert sum(f.endswith(".bin") and "_it_" in f for f in names) == 2 * 3, names
    for f in names:
        assert (tmp_path / "mean" / f).read_bytes() == (tmp_path / "plain" / f).read_bytes(), f
    x1 = np.fromfile(tmp_path / "mean" / "ex_it_3.bin", dtype="<f8")
    assert x1.shape == (517,) and not np.isnan(x1).any() and np.any(x1 != 0) and not x1[[3, 4, 5, 6]].any()


def test_cli_fatal_exits_1_with_the_message(cli_files, tmp_path):
    t, stats = cli_files
    r = _cli(t, tmp_path / "fatal", "nan.bin", "--meth-na", "fatal")
    assert r.returncode == 1, r.stdout[-3000:]
    want = "FATAL  : methylation data: %d missing methylation value(s) (NaN); the first is marker 1, row 0" % stats[
        "missing"]
    assert want in r.stdout.splitlines(), r.stdout[-3000:]
    assert not [f for f in os.listdir(tmp_path / "fatal") if f.endswith(".bin")]


def test_cli_test_mode_applies_the_policy_to_the_test_trio(cli_files, tmp_path):
    t, stats = cli_files
    est = np.fromfile(t / "ts.bin", dtype="<f8") / np.sqrt(301) * 0.9
    for it in (1, 2):
        (est * it).astype("<f8").tofile(tmp_path / f"est_it_{it}.bin")
    outs = []
    for tag, meth, extra in (("mean", "nan.bin", ["--meth-na", "mean", "--meth-na-max-frac", "0.4"]),
                             ("plain", "filled.bin", [])):
        out = tmp_path / tag
        out.mkdir()
        r = subprocess.run([va.CLI_PATH, "--run-mode", "test", "--meth-file-test", str(t / meth), "--phen-file-test",
                            str(t / "y.phen"), "--N-test", "301", "--N", "301", "--Mt", "517", "--out-dir", str(out),
                            "--out-name", "ex", "--estimate-file", str(tmp_path / "est_it_1.bin"),
                            "--test-iter-range", "1,2", *extra], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
        assert ("%d missing values in" % stats["missing"] in r.stdout) == (tag == "mean")
        outs.append((out / "ex_test.csv").read_bytes())
    assert outs[0] == outs[1] and b"nan" not in outs[0].lower() and len(outs[0].splitlines()) == 3
