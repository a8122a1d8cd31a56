"""Row subsets on the device (vampomi_set_row_subset, --keep-file, --phen-na).

The bar of this file: a context that loads the FULL files with a row subset
holds, bit for bit, what a plain context of N = n holds after loading files
from which the other rows were removed beforehand, and therefore computes the
same bits and writes the same bytes in everything that follows.  Every
comparison is np.array_equal on raw doubles (or on file bytes) against such a
plain context; there is no tolerance anywhere.

Shapes: N_file = 301 rows of which 257 seeded ones are kept, rows 0 and 300
among them (ld = 272: pad rows; 301 odd: a float or uint16 column of the file
starts only 4- or 2-byte aligned); M = 37 markers; VAMPOMI_IO_CHUNK_BYTES=4096,
so one fp64 column or six uint16 columns make a staging chunk, the chunk
boundaries fall inside the shard and there are more chunks than the three
pinned buffers.  n = 301 (nothing dropped), n = 16 (no pad rows) and n = 2 are
the edges; whole runs are 301 -> 257 x 517.
"""
import ctypes as C
import os
import subprocess
import threading

import numpy as np
import pytest

from _data import phen_from_markers
from test_covariates import write_table

pytestmark = pytest.mark.gpu

va = pytest.importorskip("vampomi_amd")
from oracle import pyoracle as O  # noqa: E402  (the index-keyed generator only)

N_FILE, N_KEEP, M, MT_RUN = 301, 257, 37, 517
_rng = np.random.default_rng(20)
_must = np.array([0, 123, 300])
ROWS = np.sort(np.concatenate([_must, _rng.choice(np.setdiff1d(np.arange(N_FILE), _must), N_KEEP - 3,
                                                  replace=False)])).astype(np.int64)
DROPPED = np.setdiff1d(np.arange(N_FILE), ROWS)
DTYPES = {"f64": np.float64, "f32": np.float32, "u16": np.uint16}
assert len(ROWS) == N_KEEP and ROWS[0] == 0 and ROWS[-1] == 300 and 123 in ROWS and len(DROPPED) == 44


@pytest.fixture(autouse=True)
def _small_chunks(monkeypatch):
    monkeypatch.setenv("VAMPOMI_IO_CHUNK_BYTES", "4096")
    monkeypatch.setenv("VAMPOMI_IO_THREADS", "3")


def as_input(X, intype):
    """X (fp64, in [0, 1]) as the input type: floats rounded, uint16 quantised."""
    if intype == "u16":
        return np.minimum(65535, np.rint(X * 65536)).astype(np.uint16)
    return X.astype(DTYPES[intype])


@pytest.fixture(scope="module")
def X37():
    return O.generate_markers(11, 1, N_FILE, 0, M)


def state(d):
    return {"meth": d.get_meth_data(), "mave": d.get_mave(), "msig": d.get_msig(), "quant": d.quant_stats()}


def same_state(a, b):
    for k in ("meth", "mave", "msig"):
        assert a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), k
    assert a["quant"] == b["quant"], (a["quant"], b["quant"])


@pytest.fixture(scope="module")
def plain_state(X37):
    """(storage, input type) -> the state of a plain context of N = 257 loaded
    with X[:, ROWS] from the host; made once and shared."""
    made = {}

    def get(storage, intype):
        if (storage, intype) not in made:
            with va.Data(N_KEEP, M, storage=storage) as d:
                d.load_meth(np.ascontiguousarray(as_input(X37, intype)[:, ROWS]))
                made[(storage, intype)] = state(d)
        return made[(storage, intype)]

    return get


def load(d, Xin, source, tmp_path, intype):
    if source == "host":
        d.load_meth(Xin)
    else:
        p = tmp_path / f"x_{intype}.bin"
        Xin.tofile(p)
        d.read_methylation_data(str(p), dtype=intype)


# ---- 1. ingest ------------------------------------------------------------------------
@pytest.mark.parametrize("source", ["file", "host"])
@pytest.mark.parametrize("intype", ["f64", "f32", "u16"])
@pytest.mark.parametrize("storage", ["f64", "f32", "u16"])
def test_ingest_equals_plain_load_of_the_taken_rows(tmp_path, X37, plain_state, storage, intype, source):
    Xin = as_input(X37, intype)
    with va.Data(N_FILE, M, storage=storage, rows=ROWS) as d:
        assert (d.N, d.N_file, d.ld) == (N_KEEP, N_FILE, 272) and np.array_equal(d.rows, ROWS)
        load(d, Xin, source, tmp_path, intype)
        got = state(d)
    same_state(got, plain_state(storage, intype))
    assert got["meth"].shape == (M, N_KEEP)
    if storage == "u16" and intype != "u16":
        assert got["quant"]["max_abs_err"] > 0  # the record is real
    if storage == "f64" and intype == "f64":
        assert np.array_equal(got["meth"], X37[:, ROWS])


@pytest.mark.parametrize("source", ["file", "host"])
def test_all_rows_kept_equals_a_plain_load_of_the_full_file(tmp_path, X37, source):
    with va.Data(N_FILE, M, storage="u16", rows=np.arange(N_FILE)) as d, va.Data(N_FILE, M, storage="u16") as p:
        load(d, X37, source, tmp_path, "f64")
        load(p, X37, source, tmp_path, "f64")
        same_state(state(d), state(p))


@pytest.mark.parametrize("rows", [np.arange(3, 300, 19), np.array([7, 300])], ids=["n16", "n2"])
@pytest.mark.parametrize("storage,intype", [("f64", "f64"), ("f32", "f64"), ("u16", "f32"), ("f64", "u16")])
def test_small_subsets(tmp_path, X37, rows, storage, intype):
    n = len(rows)
    assert n in (16, 2)
    Xin = as_input(X37, intype)
    with va.Data(N_FILE, M, storage=storage, rows=rows) as d, va.Data(n, M, storage=storage) as p:
        assert d.ld == 16
        load(d, Xin, "file", tmp_path, intype)
        p.load_meth(np.ascontiguousarray(Xin[:, rows]))
        same_state(state(d), state(p))


def test_get_row_subset(X37):
    lib = va.load()
    nf = C.c_int64(-1)
    out = np.zeros(N_KEEP, dtype=np.int64)
    with va.Data(N_FILE, M, rows=ROWS) as d, va.Data(N_KEEP, M) as p:
        assert lib.vampomi_get_row_subset(d.ctx, C.byref(nf), out.ctypes.data_as(C.c_void_p)) == 0
        assert nf.value == N_FILE and np.array_equal(out, ROWS)
        assert lib.vampomi_get_row_subset(d.ctx, C.byref(nf), None) == 0 and nf.value == N_FILE
        assert lib.vampomi_get_row_subset(p.ctx, C.byref(nf), None) == 0 and nf.value == 0
        assert p.N_file == N_KEEP and p.rows is None


# ---- 2. u16 storage: only the kept entries are range-checked -----------------------------
@pytest.mark.parametrize("intype", ["f64", "f32"])
def test_u16_ignores_what_dropped_rows_hold(tmp_path, X37, plain_state, intype):
    Xb = X37.copy()
    Xb[5, DROPPED[0]] = np.nan
    Xb[20, DROPPED[-1]] = 1.5
    Xb[36, DROPPED[7]] = -np.inf
    for source in ("file", "host"):
        with va.Data(N_FILE, M, storage="u16", rows=ROWS) as d:
            load(d, as_input(Xb, intype), source, tmp_path, intype)
            same_state(state(d), plain_state("u16", intype))


@pytest.mark.parametrize("source", ["file", "host"])
def test_u16_rejection_names_the_file_row(tmp_path, X37, source):
    Xb = X37.copy()
    Xb[5, 123] = np.nan  # a kept row
    Xb[5, DROPPED[0]] = np.nan  # an earlier dropped row: not the one named, not counted
    assert DROPPED[0] < 123
    with va.Data(N_FILE, M, storage="u16", rows=ROWS) as d:
        with pytest.raises(va.VampomiError) as e:
            load(d, Xb, source, tmp_path, "f64")
        assert e.value.status == 9, str(e.value)
        assert "marker 5, row 123" in str(e.value) and str(e.value).split(": ", 1)[1].startswith("1 "), str(e.value)


def test_u16_rejection_in_the_last_chunk_and_the_last_file_row(X37):
    Xb = X37.copy()
    Xb[36, 300] = 2.0
    with va.Data(N_FILE, M, storage="u16", rows=ROWS) as d:
        with pytest.raises(va.VampomiError) as e:
            d.load_meth(Xb)
        assert e.value.status == 9 and "marker 36, row 300" in str(e.value), str(e.value)


# ---- 3. arguments ---------------------------------------------------------------------
def _set(d, N_file, rows):
    rows = np.ascontiguousarray(rows, dtype=np.int64)
    return va.load().vampomi_set_row_subset(d.ctx, N_file, rows.ctypes.data_as(C.c_void_p), len(rows))


def test_argument_checks(tmp_path, X37):
    lib = va.load()
    with va.Data(N_KEEP, M) as d:
        assert _set(d, N_FILE, ROWS[:-1]) == 1  # n != N
        assert _set(d, N_FILE, ROWS[::-1]) == 1  # descending
        dup = ROWS.copy()
        dup[10] = dup[9]
        assert _set(d, N_FILE, dup) == 1
        hi = ROWS.copy()
        hi[-1] = N_FILE
        assert _set(d, N_FILE, hi) == 1
        lo = ROWS.copy()
        lo[0] = -1
        assert _set(d, N_FILE, lo) == 1
        assert _set(d, N_KEEP - 1, np.arange(N_KEEP)) == 1  # n > N_file
        assert _set(d, 2 ** 31, ROWS) == 1
        assert lib.vampomi_set_row_subset(d.ctx, N_FILE, None, N_KEEP) == 1
        assert _set(d, N_FILE, ROWS) == 0  # still settable after the refusals, and twice
        assert _set(d, N_FILE, ROWS) == 0
    with va.Data(N_KEEP, M) as d:
        d.set_phen(np.arange(N_KEEP, dtype=np.float64))
        assert _set(d, N_FILE, ROWS) == 6  # after the phenotype
    with va.Data(N_KEEP, M) as d:
        d.set_covariates(np.arange(2.0 * N_KEEP).reshape(N_KEEP, 2) % 7)
        assert _set(d, N_FILE, ROWS) == 6  # after the covariates
    with va.Data(N_KEEP, M) as d:
        d.load_meth(np.ascontiguousarray(X37[:, ROWS]))
        assert _set(d, N_FILE, ROWS) == 6  # after a load
        assert b"row subset" in lib.vampomi_last_error()
    with va.Data(N_FILE, M, rows=ROWS) as d:
        with pytest.raises(va.VampomiError) as e:
            d.generate(3, va.GEN_METH)
        assert e.value.status == 6
        small = np.ascontiguousarray(X37[:, ROWS])
        with pytest.raises(ValueError):
            d.load_meth(small)  # (M, n): the subset context takes the files' rows
        assert lib.vampomi_load_meth_host(d.ctx, small.ctypes.data_as(C.c_void_p), N_KEEP) == 1  # ld_in < N_file
        p = tmp_path / "short.bin"
        small.tofile(p)  # a file sized for n rows
        with pytest.raises(va.VampomiError) as e:
            d.read_methylation_data(str(p))
        assert e.value.status == 4
        d.load_meth(X37)  # the context is still usable
        assert np.array_equal(d.get_meth_data(), small)
    with pytest.raises(va.VampomiError) as e:
        va.Data(N_FILE, M, rows=ROWS[::-1])
    assert e.value.status == 1


# ---- 4. phenotype and covariates ---------------------------------------------------------
def _phen_text(y, na=()):
    return "".join("f%d i%d %s\n" % (i, i, "NA" if i in na else "%0.10f" % v) for i, v in enumerate(y))


@pytest.mark.parametrize("standardize", [True, False])
def test_read_phen_keeps_the_rows_then_standardises(tmp_path, standardize):
    y = np.array([float("%0.10f" % v) for v in np.random.default_rng(4).standard_normal(N_FILE) * 3 + 1])
    p = tmp_path / "y.phen"
    p.write_text(_phen_text(y, na=(int(DROPPED[3]), int(DROPPED[-1]))))  # NA in dropped rows only
    with va.Data(N_FILE, M, rows=ROWS) as d, va.Data(N_KEEP, M) as q:
        d.read_phen(str(p), standardize=standardize)
        q.set_phen(y[ROWS], standardize=standardize)
        assert np.array_equal(d.get_phen(), q.get_phen()) and d.get_phen().shape == (N_KEEP,)
        if not standardize:
            assert np.array_equal(d.get_phen(), y[ROWS])
        d.set_phen(y[ROWS], standardize=standardize)  # set_phen keeps taking n values
        assert np.array_equal(d.get_phen(), q.get_phen())
        with pytest.raises(ValueError):
            d.set_phen(y)
        p.write_text(_phen_text(y, na=(123,)))  # NA in a kept row
        with pytest.raises(va.VampomiError) as e:
            d.read_phen(str(p))
        assert e.value.status == 5 and "NAN in data!" in str(e.value)
        p.write_text(_phen_text(y[ROWS]))  # a file of n rows is not the subset's file
        with pytest.raises(va.VampomiError) as e:
            d.read_phen(str(p))
        assert e.value.status == 1


def test_read_covariates_keeps_the_rows_then_standardises(tmp_path):
    rng = np.random.default_rng(9)
    Z = rng.standard_normal((N_FILE, 3)) * np.array([0.3, 12.0, 1.0]) + np.array([40.0, -2.0, 0.0])
    p = tmp_path / "z.cov"
    write_table(p, Z)
    with va.Data(N_FILE, M, rows=ROWS) as d, va.Data(N_KEEP, M) as q:
        d.read_covariates(str(p), 3)
        q.set_covariates(Z[ROWS], standardize=True)
        assert np.array_equal(d.get_covariates(), q.get_covariates()) and d.get_covariates().shape == (N_KEEP, 3)
        d.set_covariates(Z[ROWS], standardize=True)  # set_covariates keeps taking n rows
        assert np.array_equal(d.get_covariates(), q.get_covariates())
        write_table(p, Z[ROWS])
        with pytest.raises(va.VampomiError) as e:
            d.read_covariates(str(p), 3)
        assert e.value.status == 4  # vampomi_parse_covariates: not N_file rows


# ---- 5. whole runs -------------------------------------------------------------------------
@pytest.fixture(scope="module")
def problem():
    X = O.generate_markers(5, 1, N_FILE, 0, MT_RUN)
    y, beta = phen_from_markers(X, seed=5)
    Z = np.random.default_rng(6).standard_normal((N_FILE, 3)) * np.array([1.0, 5.0, 0.2]) + np.array([0.0, 3.0, -1.0])
    return X, y, beta, Z


def _pair(X, storage="f64"):
    d = va.Data(N_FILE, MT_RUN, storage=storage, rows=ROWS)
    d.load_meth(X)
    p = va.Data(N_KEEP, MT_RUN, storage=storage)
    p.load_meth(np.ascontiguousarray(X[:, ROWS]))
    return d, p


def _run(d, beta, its, model):
    v = va.Vamp(d, va.VampOptions(model=model, max_iter=its, stop_criteria_thr=0.0), true_signal=beta)
    v.infere(keep_hist=True)
    s = v.summary()
    assert s["iterations"] == its
    return v, s


def _same_run(a, b, its):
    (va_, sa), (vb, sb) = a, b
    assert sa["cg_iters"] == sb["cg_iters"] and sa["ons_iters"] == sb["ons_iters"] and sa["L"] == sb["L"]
    assert np.array_equal(va_.x1_hist[:its], vb.x1_hist[:its]) and np.array_equal(va_.r1_hist[:its], vb.r1_hist[:its])
    assert np.array_equal(va_.params[:its], vb.params[:its], equal_nan=True)
    assert np.array_equal(va_.metrics[:its], vb.metrics[:its], equal_nan=True)
    assert np.array_equal(va_.x1_final, vb.x1_final) and np.any(va_.x1_final != 0)


@pytest.mark.parametrize("storage", ["f64", "u16"])
def test_linear_run_assoc_and_test_metrics_are_bitwise_the_plain_ones(problem, storage):
    X, y, beta, _ = problem
    d, p = _pair(X, storage)
    with d, p:
        d.set_phen(y[ROWS])
        p.set_phen(y[ROWS])
        a, b = _run(d, beta, 6, "linear"), _run(p, beta, 6, "linear")
        _same_run(a, b, 6)
        est = a[0].x1_final.copy()
        (pa, sa), (pb, sb) = d.assoc_loo(est), p.assoc_loo(est)
        assert np.array_equal(pa, pb) and np.array_equal(sa, sb) and sa.shape == (MT_RUN, 5)
        assert d.test_metrics(est) == p.test_metrics(est)


def test_probit_run_with_covariates_is_bitwise_the_plain_one(problem):
    X, y, beta, Z = problem
    yb = (y > 0).astype(np.float64)
    d, p = _pair(X)
    with d, p:
        for c in (d, p):
            c.set_phen(yb[ROWS], standardize=False)
            c.set_covariates(Z[ROWS], standardize=True)
        a, b = _run(d, beta, 5, "bin_class"), _run(p, beta, 5, "bin_class")
        _same_run(a, b, 5)
        assert np.array_equal(a[0].cov_eff, b[0].cov_eff) and np.any(a[0].cov_eff != 0)
        assert np.array_equal(a[0].prior[:5], b[0].prior[:5], equal_nan=True)


# ---- 6. two loopback ranks: the S * N_file file offset -----------------------------------------
@pytest.mark.parametrize("intype,storage", [("f64", "f64"), ("u16", "f32"), ("f32", "u16")])
def test_two_ranks_read_their_shard_of_the_full_file(tmp_path, monkeypatch, X37, plain_state, intype, storage):
    monkeypatch.setenv("VAMPOMI_COMM", "loopback")
    p = tmp_path / "x.bin"
    as_input(X37, intype).tofile(p)
    cid = os.urandom(va.UNIQUE_ID_BYTES)
    got, errs = {}, []

    def work(r):
        try:
            with va.Data(N_FILE, M, rank=r, nranks=2, comm_id=cid, device=0, storage=storage, rows=ROWS) as d:
                d.read_methylation_data(str(p), dtype=intype)
                got[r] = (d.S, d.M, d.get_meth_data(), d.get_mave(), d.get_msig())
        except BaseException as e:  # noqa: BLE001
            errs.append((r, e))

    th = [threading.Thread(target=work, args=(r,), daemon=True) for r in range(2)]
    [t.start() for t in th]
    [t.join(120) for t in th]
    assert not any(t.is_alive() for t in th) and not errs, errs
    assert [(got[r][0], got[r][1]) for r in range(2)] == [(0, 19), (19, 18)]
    ref = plain_state(storage, intype)
    for k, name in ((2, "meth"), (3, "mave"), (4, "msig")):
        assert np.array_equal(np.concatenate([got[0][k], got[1][k]]), ref[name]), name


# ---- 7. the CLI: full files + flags against reduced files, byte for byte -----------------------
NA_CLI = (17, 250)
KEEP_OUT = (0, 3, 123, 299, 300)  # five more, dropped by the keep file
KEPT_CLI = np.array([i for i in range(N_FILE) if i not in NA_CLI + KEEP_OUT])


@pytest.fixture(scope="module")
def cli_files(tmp_path_factory, problem):
    X, y, beta, Z = problem
    t = tmp_path_factory.mktemp("cli")
    yb = (y > 0).astype(np.float64)
    X.astype("<f8").tofile(t / "full.bin")
    np.ascontiguousarray(X[:, KEPT_CLI]).astype("<f8").tofile(t / "less.bin")
    for name, v in (("lin", y), ("bin", yb)):
        (t / f"full_{name}.phen").write_text(_phen_text(v, na=NA_CLI))
        (t / f"less_{name}.phen").write_text("".join("f%d i%d %0.10f\n" % (i, i, v[i]) for i in KEPT_CLI))
    ids = [i for i in range(N_FILE) if i not in KEEP_OUT]  # names the NA rows too: --phen-na drop takes them out
    np.random.default_rng(1).shuffle(ids)
    (t / "keep.txt").write_text("".join("f%d i%d\n" % (i, i) for i in ids + ids[:3]))
    write_table(t / "full.cov", Z)
    with open(t / "less.cov", "w") as f:  # write_table's rows, the kept ones with their own IDs
        lines = open(t / "full.cov").read().splitlines(keepends=True)
        f.write(lines[0] + "".join(lines[1 + i] for i in KEPT_CLI))
    beta.astype("<f8").tofile(t / "ts.bin")
    est = beta / np.sqrt(N_FILE) * 0.9
    for it in (1, 2):
        (est * it).astype("<f8").tofile(t / f"est_it_{it}.bin")
    return t


def _cli_pair(t, tmp_path, phen, common, full_extra=(), less_extra=(), test_mode=False):
    outs = []
    nflag, mflag, pflag, kflag = (("--N-test", "--meth-file-test", "--phen-file-test", "--keep-file-test") if test_mode
                                  else ("--N", "--meth-file", "--phen-file", "--keep-file"))
    for tag in ("full", "less"):
        out = tmp_path / tag
        out.mkdir()
        cmd = [va.CLI_PATH, mflag, str(t / f"{tag}.bin"), pflag, str(t / f"{tag}_{phen}.phen"), "--Mt", str(MT_RUN),
               "--out-dir", str(out), "--out-name", "ex", *common]
        if tag == "full":
            cmd += [nflag, str(N_FILE), kflag, str(t / "keep.txt"), "--phen-na", "drop", *full_extra]
        else:
            cmd += [nflag, str(len(KEPT_CLI)), *less_extra]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
        if tag == "full":
            assert "INFO   : kept 294 of 301 samples (5 not in the keep file, 2 with an NA phenotype)" in r.stdout
        else:
            assert "INFO   : kept" not in r.stdout
        outs.append(out)
    names = sorted(f for f in os.listdir(outs[0]) if not f.startswith("."))
    assert names and names == sorted(f for f in os.listdir(outs[1]) if not f.startswith("."))
    for f in names:
        assert (outs[0] / f).read_bytes() == (outs[1] / f).read_bytes(), f
    return names


def test_cli_infere_linear(cli_files, tmp_path):
    t = cli_files
    names = _cli_pair(t, tmp_path, "lin", ["--iterations", "4", "--stop-criteria-thr", "0", "--true-signal-file",
                                           str(t / "ts.bin")])
    assert len(names) == 2 * 4 + 3, names


def test_cli_infere_bin_class_with_covariates(cli_files, tmp_path):
    t = cli_files
    common = ["--iterations", "3", "--stop-criteria-thr", "0", "--true-signal-file", str(t / "ts.bin"), "--model",
              "bin_class", "--C", "3"]
    names = _cli_pair(t, tmp_path, "bin", common, ["--cov-file", str(t / "full.cov")],
                      ["--cov-file", str(t / "less.cov")])
    assert "ex_cov_eff.bin" in names
    assert np.any(np.fromfile(tmp_path / "full" / "ex_cov_eff.bin", dtype="<f8") != 0)


def test_cli_association_test_loo(cli_files, tmp_path):
    t = cli_files
    names = _cli_pair(t, tmp_path, "lin", ["--run-mode", "association_test", "--pval-method", "loo",
                                           "--estimate-file", str(t / "est_it_2.bin")])
    assert names == ["ex_it_2_pval_loo.bin"]
    pv = np.fromfile(tmp_path / "full" / names[0], dtype="<f8")
    assert pv.shape == (MT_RUN,) and np.all((pv >= 0) & (pv <= 1)) and len(np.unique(pv)) > MT_RUN // 2


def test_cli_test_mode(cli_files, tmp_path):
    t = cli_files
    names = _cli_pair(t, tmp_path, "lin", ["--run-mode", "test", "--N", str(N_FILE), "--estimate-file",
                                           str(t / "est_it_1.bin"), "--test-iter-range", "1,2"], test_mode=True)
    assert names == ["ex_test.csv"]
