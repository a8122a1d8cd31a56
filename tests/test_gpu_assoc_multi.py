"""Association tests for several phenotypes in one pass over the matrix
(vampomi_assoc_loo_multi) on the GPU.

The contract: block t of the statistics and p-values is, bit for bit, what
set_phen(Y_t) followed by assoc_loo(est_t) returns on the same context, for
every chunk width (T = 1 ... 9: the single kernel, KT = 2, 3, 4, two chunks and
a remainder), every storage, any number of ranks, adjusted and mean-filled
contexts, and through the command line (--trait-file).  The capability: T = 9
phenotypes read the matrix 6 times where the loop reads it 18 times.  One
comparison against the oracle, with the bars of tests/test_gpu_assoc.py, is
independent of the engine's own single path."""
import os
import threading
import time

import numpy as np
import pytest

import _assoc_multi as H

pytestmark = pytest.mark.gpu

va = pytest.importorskip("vampomi_amd")
from oracle import pyoracle as O  # noqa: E402  (checker)

TS = (1, 2, 3, 4, 5, 9)
ESIZE = {"f64": 8, "f32": 4, "u16": 2}
# odd N with the zero pad row and several load rounds; many unrolled rounds and
# fewer markers than CUs; fewer markers than a workgroup's G; N below one load round
SHAPES = [(4099, 301, 1), (20000, 64, 0), (257, 5, 1), (5, 7, 0)]
CASES = [(s, st) for st in ("f64", "f32", "u16") for s in SHAPES if st != "u16" or s[2] == 1]


@pytest.mark.parametrize("shape,storage", CASES)
def test_blocks_equal_the_single_calls_bitwise(shape, storage):
    N, Mt, kind = shape
    standardize = SHAPES.index(shape) % 2 == 0  # both ways, at fixed shapes
    X, Y, est = H.problem(N, Mt, kind)
    Yin = Y * 2.5 if standardize else Y  # something for the scaling to undo
    with va.Data(N, Mt, storage=storage) as d:
        d.load_meth(X)
        p1, s1 = H.single_loop(d, Yin, est, standardize)
        for T in TS:
            d.reset_stats()
            p, s = d.assoc_loo_multi(Yin[:T], est[:T], standardize=standardize)
            assert p.shape == (T, Mt) and s.shape == (T, Mt, 5)
            for t in range(T):
                assert np.array_equal(s[t], s1[t]), (T, t)
                assert np.array_equal(p[t], p1[t]), (T, t)
            st = d.stats()
            widths = [4] * (T // 4) + ([T % 4] if T % 4 else [])
            assert st.a_passes_exec == 2 * len(widths) and st.loo.launches == len(widths)
            assert st.loo.bytes_total == sum(H.loo_bytes(d, ESIZE[storage], k) for k in widths)
            assert [st.ax_k[k - 1].launches for k in (1, 2, 3, 4)] == [widths.count(k) for k in (1, 2, 3, 4)]


def test_nine_phenotypes_read_the_matrix_six_times():
    """The capability itself: 3 A.x + 3 association passes against the loop's 18."""
    N, Mt, kind = SHAPES[0]
    X, Y, est = H.problem(N, Mt, kind)
    with va.Data(N, Mt) as d:
        d.load_meth(X)
        d.reset_stats()
        H.single_loop(d, Y, est, False)
        assert d.stats().a_passes_exec == 18 and d.stats().loo.launches == 9
        d.reset_stats()
        d.assoc_loo_multi(Y, est, standardize=False)
        st = d.stats()
        assert st.a_passes_exec == 6 and st.loo.launches == 3 and st.ax.launches == 3
        assert st.loo.bytes_total == 2 * H.loo_bytes(d, 8, 4) + H.loo_bytes(d, 8, 1)


def test_no_estimate_is_the_zero_estimate_without_the_ax_pass():
    N, Mt, kind = SHAPES[0]
    X, Y, _ = H.problem(N, Mt, kind)
    with va.Data(N, Mt) as d:
        d.load_meth(X)
        p0, s0 = d.assoc_loo_multi(Y[:3], np.zeros((3, Mt)), standardize=False)
        d.reset_stats()
        p, s = d.assoc_loo_multi(Y[:3], None, standardize=False)
        st = d.stats()
        assert st.a_passes_exec == 1 and st.ax.launches == 0 and st.loo.launches == 1
        assert np.array_equal(s, s0) and np.array_equal(p, p0)
        p1, s1 = H.single_loop(d, Y[:3], np.zeros((3, Mt)), False)
        assert np.array_equal(s, s1) and np.array_equal(p, p1)


def test_blocks_against_the_oracle():
    """Independent of the engine's single path: each block against the oracle's
    assoc_loo, with the bars of tests/test_gpu_assoc.py (sums 1e-13, p-value
    function 1e-12, p-values 1e-10 or 10x the measured order spread)."""
    N, Mt, T = 1000, 2000, 3
    X, Y, est = H.problem(N, Mt, 1, T=3)
    with va.Data(N, Mt) as d:
        d.load_meth(X)
        p, s = d.assoc_loo_multi(Y, est, standardize=False)
    for t in range(T):
        po, sto = O.assoc_loo(X, Y[t], est[t])
        H.check_pfun(p[t], s[t], N)
        H.check_loo(p[t], s[t], po, sto, H.order_spread(X, Y[t], est[t], po))


def test_the_context_keeps_its_phenotype():
    N, Mt, kind = SHAPES[2]
    X, Y, est = H.problem(N, Mt, kind)
    with va.Data(N, Mt) as d:
        d.load_meth(X)
        pm, sm = d.assoc_loo_multi(Y[:3], est[:3], standardize=False)  # no phenotype set: works
        with pytest.raises(va.VampomiError) as e:
            d.get_phen()
        assert e.value.status == 6  # still none
        d.set_phen(Y[8] * 3.0, standardize=True)
        y0 = d.get_phen()
        p0, s0 = d.assoc_loo(est[8])
        p, s = d.assoc_loo_multi(Y[:3], est[:3], standardize=False)
        assert np.array_equal(p, pm) and np.array_equal(s, sm)
        assert np.array_equal(d.get_phen(), y0)
        p1, s1 = d.assoc_loo(est[8])
        assert np.array_equal(p1, p0) and np.array_equal(s1, s0)


def test_argument_and_state_errors():
    import ctypes as C

    N, Mt, kind = SHAPES[2]
    X, Y, est = H.problem(N, Mt, kind)
    lib = va.load()
    Yc = np.ascontiguousarray(Y[:2])
    dp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    with va.Data(N, Mt) as d:
        with pytest.raises(va.VampomiError) as e:
            d.assoc_loo_multi(Y[:2], est[:2])
        assert e.value.status == 6  # ERR_STATE: nothing loaded
        d.load_meth(X)
        assert lib.vampomi_assoc_loo_multi(d.ctx, 0, dp(Yc), N, 0, None, None, None, 0) == 1
        assert lib.vampomi_assoc_loo_multi(d.ctx, 2, None, N, 0, None, None, None, 0) == 1
        assert lib.vampomi_assoc_loo_multi(d.ctx, 2, dp(Yc), N - 1, 0, None, None, None, 0) == 1
        assert lib.vampomi_assoc_loo_multi(d.ctx, 2, dp(Yc), N, 0, None, None, None, 0) == 0
        # a stride above N: the columns are taken where they are
        wide = np.zeros((2, N + 3))
        wide[:, :N] = Yc
        pv = np.zeros((2, Mt))
        assert lib.vampomi_assoc_loo_multi(d.ctx, 2, dp(wide), N + 3, 0, None, dp(pv), None, 0) == 0
        assert np.array_equal(pv, d.assoc_loo_multi(Yc, None, standardize=False)[0])


@pytest.mark.parametrize("what", ["adjust", "meth_na"])
def test_adjusted_and_mean_filled_contexts_meet_the_contract(what):
    N, Mt, T = 301, 257, 3
    X, Y, est = H.problem(N, Mt, 1, T=3)
    rng = np.random.default_rng(4)
    kw = {}
    if what == "adjust":
        kw["adjust"] = rng.normal(size=(N, 3))
    else:
        X = X.copy()
        X[rng.integers(0, Mt, 400), rng.integers(0, N, 400)] = np.nan
        kw["meth_na"] = "mean"
    with va.Data(N, Mt, **kw) as d:
        d.load_meth(X)
        p1, s1 = H.single_loop(d, Y * 1.5 + 0.25, est, True)
        p, s = d.assoc_loo_multi(Y * 1.5 + 0.25, est, standardize=True)
    assert np.array_equal(s, s1) and np.array_equal(p, p1)
    assert np.all(np.isfinite(s)) and np.all(np.isfinite(p))


def _run_ranks(monkeypatch, P, N, Mt, fn, timeout=100):
    """fn(rank, data) on P loopback rank threads (tests/test_gpu_sharded.py's run_ranks)."""
    monkeypatch.setenv("VAMPOMI_COMM", "loopback")
    cid = os.urandom(va.UNIQUE_ID_BYTES)
    res, errs = [None] * P, []

    def work(r):
        try:
            with va.Data(N, Mt, rank=r, nranks=P, comm_id=cid, device=0) as d:
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


_one_rank = {}


@pytest.mark.parametrize("P", [2, 3])
def test_ranks_meet_the_contract(monkeypatch, P):
    N, Mt, T = 1000, 333, 5
    X, Y, est = H.problem(N, Mt, 1, T=5)
    if not _one_rank:
        with va.Data(N, Mt) as d:
            d.load_meth(X)
            _one_rank["single"] = H.single_loop(d, Y, est, False)[0]
            _one_rank["multi"] = d.assoc_loo_multi(Y, est, standardize=False)[0]

    def fn(r, d):
        d.load_meth(X[d.S:d.S + d.M])
        e = est[:, d.S:d.S + d.M]
        return H.single_loop(d, Y, e, False), d.assoc_loo_multi(Y, e, standardize=False)

    res = _run_ranks(monkeypatch, P, N, Mt, fn)
    for (p1, s1), (p, s) in res:
        assert np.array_equal(s, s1) and np.array_equal(p, p1)
    cat1 = np.concatenate([r[0][0] for r in res], axis=1)
    cat = np.concatenate([r[1][0] for r in res], axis=1)
    assert cat.shape == (T, Mt)
    same = cat1 == _one_rank["single"]  # where the rank-ordered A.x sum changed nothing
    assert np.array_equal(cat[same], _one_rank["multi"][same])


@pytest.mark.parametrize("mode", ["plain", "na_drop", "two_processes", "bin_class"])
def test_cli_trait_file_writes_the_single_runs_files(tmp_path, mode):
    """--trait-file: each phenotype's file is byte for byte that of a single
    run with its --phen-file, --estimate-file and --out-name; with NA rows
    under --phen-na drop against single runs that keep the common rows; as two
    processes against single runs of two processes; with --model bin_class,
    where the single run leaves its 0/1 phenotype raw (not standardised)."""
    N, Mt, T = 301, 500, 3
    X, Y, est = H.problem(N, Mt, 1, T=3)
    if mode == "bin_class":  # cases and controls: above the phenotype's median or not
        Y = (Y > np.median(Y, axis=1, keepdims=True)).astype(np.float64)
    tmp = str(tmp_path)
    na = {1: (17, 200)} if mode == "na_drop" else None
    Xp, phen, ests, tf = H.write_inputs(tmp, X, Y, est, na)
    P = 2 if mode == "two_processes" else 1
    outs = [tmp_path / ("out%d" % k) for k in range(T + 1)]
    for o in outs:
        o.mkdir()
    base = [va.CLI_PATH, "--meth-file", Xp, "--N", str(N), "--Mt", str(Mt), "--run-mode", "association_test",
            "--pval-method", "loo"] + (["--model", "bin_class"] if mode == "bin_class" else [])
    cmds = [base + ["--out-dir", str(outs[T]), "--trait-file", tf] + (["--phen-na", "drop"] if na else [])]
    keep = []
    if na:
        rows, _, counts = va.phen_rows_common(phen, drop_na=True)
        assert len(rows) == N - 2 and counts.tolist() == [0, 2, 0]
        kf = tmp_path / "common.keep"
        kf.write_text("".join("%d %d\n" % (i, i) for i in rows))
        keep = ["--keep-file", str(kf)]
    for t in range(T):
        cmds.append(base + ["--out-dir", str(outs[t]), "--out-name", "trait%d" % t, "--phen-file", phen[t],
                            "--estimate-file", ests[t]] + keep)
    jobs = [H.launch(c, P, tmp, "job%d" % k) for k, c in enumerate(cmds)]  # four jobs side by side
    for procs, logs in jobs:
        assert H.wait(procs, 120) == [0] * P, [open(lg).read()[-2000:] for lg in logs]
    if na:
        txt = open(jobs[0][1][0]).read()
        assert "INFO   : kept 299 of 301 samples (0 not in the keep file, 2 with an NA phenotype)" in txt
        assert "INFO   : NA phenotypes: trait0 0 trait1 2 trait2 0" in txt
    for t in range(T):
        name = "trait%d_it_7_pval_loo.bin" % t
        got, ref = (outs[T] / name).read_bytes(), (outs[t] / name).read_bytes()
        assert len(got) == 8 * Mt and got == ref, name
    assert sorted(f for f in os.listdir(outs[T]) if not f.startswith(".")) == \
        ["trait%d_it_7_pval_loo.bin" % t for t in range(T)]
    p = np.fromfile(outs[T] / "trait0_it_7_pval_loo.bin", dtype="<f8")
    assert np.all((p >= 0) & (p <= 1))
