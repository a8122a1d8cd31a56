"""Covariates of the probit model on the device (src/vamp_probit.cpp:62-95,
213-233, 469-617) against the numpy restatement tests/_cov_ref.py: the Newton
sums, the offset z-denoiser, the whole fit, and each iteration's z-side stage
of a whole run, on one rank, on two loopback ranks and through the CLI.

Every figure is printed before it is asserted."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import relerr
from _data import make_problem
import _cov_ref as R
from test_covariates import SAFE_FITS, write_table

pytestmark = pytest.mark.gpu

va = pytest.importorskip("vampomi_amd")
from vampomi_amd import _lib  # noqa: E402

T = 64  # vk::kCovTile: samples per workgroup of the Newton sums


def _ctx(N, y, Z=None, Mt=4, standardize=False):
    d = va.Data(N, Mt)
    d.set_phen(y, standardize=False)
    if Z is not None:
        d.set_covariates(Z, standardize=standardize)
    return d


# N = 1 of the issue's list cannot be opened (vampomi_open: N >= 2, tests/test_abi.py); 2 stands for it.
# T - 1, T, T + 1 are 63, 64, 65.
@pytest.mark.parametrize("N", [2, T - 1, T, T + 1, 301, 4099])
def test_cov_eval_matches_restatement(N):
    rng = np.random.default_rng(100 + N)
    y = (rng.random(N) < 0.45).astype(np.float64)
    gg = 0.3 * rng.standard_normal(N)
    for Cn in (1, 2, 5, 64):
        Z = rng.standard_normal((N, Cn))
        eta = 0.4 * rng.standard_normal(Cn) / np.sqrt(Cn)
        with _ctx(N, y, Z) as d:
            assert np.array_equal(d.get_covariates(), Z)
            H, rhs, ml = d.cov_eval(eta, gg)
            H2, rhs2, ml2 = d.cov_eval(eta, gg)
        Hr, rr, mr = R.cov_eval(Z, y, gg, eta)
        eh, er, em = relerr(H, Hr), relerr(rhs, rr), abs(ml - mr) / abs(mr)
        print(f"cov_eval N={N} C={Cn}: H {eh:.2e} rhs {er:.2e} mlogL {em:.2e}")
        assert eh <= 1e-12 and er <= 1e-12 and em <= 1e-12, (N, Cn)
        assert np.array_equal(H, H.T)
        assert np.array_equal(H, H2) and np.array_equal(rhs, rhs2) and ml == ml2, "not repeatable"


def test_cov_eval_without_gg_is_gg_zero():
    Z, y, _ = R.probit_problem(301, 3, 11)
    eta = np.array([0.3, -0.2, 0.1])
    with _ctx(301, y, Z) as d:
        a, b = d.cov_eval(eta), d.cov_eval(eta, np.zeros(301))
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]


def test_denoise_bin_cov_matches_restatement():
    N = 5000
    rng = np.random.default_rng(11)
    y = (rng.random(N) < 0.5).astype(np.float64)
    lib = va.load()
    with _ctx(N, y) as d:
        for tau1 in (1e-6, 0.3, 2.0, 500.0):
            sq = np.sqrt(1 + 1 / tau1)
            # arguments of erfcx spread over [-16, 16]: both clamps and both branches
            p = rng.uniform(-12, 12, N) * np.sqrt(2) * sq
            m = rng.uniform(-4, 4, N) * np.sqrt(2) * sq
            z, sd = d.denoise_bin(p, tau1, m_cov=m)
            zo, gd = R.g1_bin_cov(p, tau1, y, m), R.g1d_bin_cov(p, tau1, y, m)
            e_el = float(np.max(np.abs(z - zo) / np.abs(zo)))
            e_sd = abs(sd - gd.sum()) / max(1.0, abs(gd).sum())
            print(f"denoise_bin_cov tau1={tau1}: per element {e_el:.2e} sum_d {e_sd:.2e}")
            assert e_el <= 1e-13, tau1
            assert e_sd <= 1e-12, tau1
            # m_cov = NULL is vampomi_denoise_bin, bit for bit
            z0, sd0 = d.denoise_bin(p, tau1)
            zn, sdn = np.zeros(N), C.c_double()
            _lib.check(lib.vampomi_denoise_bin_cov(d.ctx, p.ctypes.data_as(C.c_void_p), tau1, None,
                                                   zn.ctypes.data_as(C.c_void_p), C.byref(sdn), 0))
            assert np.array_equal(z0, zn) and sd0 == sdn.value
            # g1(p, m) = g1(p + m, 0) - m; g1d(p, m) = g1d(p + m, 0): the same c
            zs, sds = d.denoise_bin(p + m, tau1, m_cov=np.zeros(N))
            e_id = relerr(zs - m, z)
            print(f"  identity g1 {e_id:.2e}, g1d sums {sd!r} {sds!r}")
            assert e_id <= 1e-12, tau1
            assert sd == sds, tau1
            # a zero offset gives the values of the kernel without one
            assert np.array_equal(d.denoise_bin(p, tau1, m_cov=np.zeros(N))[0], z0)


@pytest.mark.parametrize("N,Cn,seed", SAFE_FITS)
def test_newton_cov_matches_restatement(N, Cn, seed):
    Z, y, _ = R.probit_problem(N, Cn, seed)
    eta_r, tr = R.newton(Z, y)
    assert R.trace_is_safe(tr), tr  # no borderline decision on the CPU side
    with _ctx(N, y, Z) as d:
        eta, iters, bt, rel = d.newton_cov()
        eta2, iters2, bt2, rel2 = d.newton_cov(gg=np.zeros(N), eta0=np.zeros(Cn))
    e = relerr(eta, eta_r)
    print(f"newton_cov N={N} C={Cn}: iters {iters} (ref {tr['iters']}), backtracks {bt.tolist()} "
          f"(ref {tr['backtracks']}), eta {e:.2e}, rel_err {rel.tolist()}")
    assert iters == tr["iters"]
    nonfinal = [k for k in range(iters) if k != tr["final"]]
    assert [int(bt[k]) for k in nonfinal] == [tr["backtracks"][k] for k in nonfinal]
    assert e <= 1e-10
    assert np.allclose(rel[nonfinal], np.array(tr["rel_err"])[nonfinal], rtol=1e-8)
    assert np.array_equal(eta, eta2) and iters == iters2 and np.array_equal(bt, bt2) and np.array_equal(rel, rel2)


def test_newton_cov_constant_column_gives_exact_zeros():
    Z, y, _ = R.probit_problem(301, 3, 11)
    Z[:, 1] = 2.5
    with _ctx(301, y, Z, standardize=True) as d:
        assert np.all(d.get_covariates()[:, 1] == 0.0)
        eta, iters, bt, rel = d.newton_cov()
    assert np.all(eta == 0.0) and eta.shape == (3,) and iters == 1


# ---- whole runs ---------------------------------------------------------------
N_RUN, MT_RUN, ITS = 301, 500, 6
EFF = np.array([0.9, -0.7, 0.5])


def _run_problem():
    """A case/control phenotype whose liability has a genetic part and a
    covariate part of comparable size."""
    X, liab, beta = make_problem(N_RUN, MT_RUN)
    rng = np.random.default_rng(77)
    Z = rng.standard_normal((N_RUN, 3)) * [3.0, 0.5, 10.0] + [40.0, 0.0, -5.0]  # raw: age-, sex-, batch-like scales
    y = (liab + R.standardize(Z) @ EFF > 0).astype(np.float64)
    return X, y, beta, Z


def _staged_run(d, X, y, beta, Z, batch_rhs, check=True):
    """Steps a bin_class run; per iteration the z-side stage against the
    restatement: beta1 = (sum of g1d, set to N - 1 when it reaches N) / N, as
    src/vamp_probit.cpp:226-236 has it (R.beta1_of; the sum exceeds N - 1 without
    reaching N in some iterations of this problem, and stays unclipped there)."""
    d.load_meth(X[d.S:d.S + d.M])
    d.set_phen(y, standardize=False)
    if Z is not None:
        d.set_covariates(Z)
    v = va.Vamp(d, va.VampOptions(model="bin_class", max_iter=ITS, stop_criteria_thr=0.0, batch_rhs=batch_rhs),
                true_signal=beta[d.S:d.S + d.M])
    v.begin(keep_hist=True)
    eff = v.cov_eff
    m = d.get_covariates() @ eff if Z is not None else np.zeros(d.N)
    rows = []
    for it in range(ITS):
        p1, tau1 = v.probit_state()
        v.step()
        b_ref = R.beta1_of(R.g1d_bin_cov(p1, tau1, y, m).sum(), d.N)
        b_no = R.beta1_of(R.g1d_bin_cov(p1, tau1, y, 0 * m).sum(), d.N)
        b, t = v.params[it][1], v.params[it][3]
        rows.append((abs(b - b_ref) / abs(b_ref), abs(b - b_no) / abs(b_no), t == tau1))
    v.end()
    s = v.summary()
    s["x1_hist"], s["r1_hist"] = v.x1_hist[:ITS, :d.M].copy(), v.r1_hist[:ITS, :d.M].copy()
    s["cov_eff"], s["stage"] = eff.copy(), rows
    if check:
        for it, (e, miss, same_tau) in enumerate(rows):
            print(f"  it {it + 1}: beta1 vs restatement {e:.2e}, vs no offset {miss:.2e}, tau1 equal {same_tau}")
        for it, (e, miss, same_tau) in enumerate(rows):
            assert e <= 1e-12, it + 1
            assert same_tau, it + 1
            assert miss > 1e-6, it + 1
    return s


@pytest.mark.parametrize("batch_rhs", [4, 0])
def test_every_iterations_z_stage_uses_the_offset(batch_rhs):
    X, y, beta, Z = _run_problem()
    with va.Data(N_RUN, MT_RUN) as d:
        s = _staged_run(d, X, y, beta, Z, batch_rhs)
        eta, *_ = d.newton_cov()
    assert s["iterations"] == ITS
    assert np.array_equal(s["cov_eff"], eta)  # the run's fit is newton_cov from gg = 0, eta0 = 0
    assert np.linalg.norm(s["cov_eff"]) > 0.3
    assert relerr(s["cov_eff"], R.newton(R.standardize(Z), y)[0]) <= 1e-8


@pytest.mark.parametrize("batch_rhs", [4, 0])
def test_constant_covariates_are_transparent(batch_rhs):
    X, y, beta, _ = _run_problem()
    const = np.tile([1.0, -2.5, 40.0], (N_RUN, 1))
    with va.Data(N_RUN, MT_RUN) as d:
        a = _staged_run(d, X, y, beta, const, batch_rhs, check=False)
    with va.Data(N_RUN, MT_RUN) as d:
        b = _staged_run(d, X, y, beta, None, batch_rhs, check=False)
    assert np.all(a["cov_eff"] == 0.0) and a["cov_eff"].shape == (3,) and b["cov_eff"].shape == (0,)
    for key in ("x1_hist", "r1_hist"):
        assert np.array_equal(a[key], b[key]), key
    for key in ("params", "metrics"):  # (x1's correlation of iteration 1 is 0/0 in both)
        assert np.array_equal(np.array(a[key]), np.array(b[key]), equal_nan=True), key
    for key in ("cg_iters", "ons_iters", "L", "iterations"):
        assert a[key] == b[key], key


def test_cov_eff_needs_a_bin_class_run():
    X, y, beta, Z = _run_problem()
    with va.Data(N_RUN, MT_RUN) as d:
        d.load_meth(X)
        d.set_phen(y, standardize=False)
        d.set_covariates(Z)
        v = va.Vamp(d, va.VampOptions(max_iter=2, stop_criteria_thr=0.0), true_signal=beta)
        with pytest.raises(va.VampomiError) as e:
            v.cov_eff
        assert e.value.status == 6
        with pytest.raises(va.VampomiError) as e:
            v.probit_state()
        assert e.value.status == 6
        v.infere()  # the linear model ignores the table
        with pytest.raises(va.VampomiError) as e:
            v.cov_eff
        assert e.value.status == 6


def test_two_loopback_ranks_fit_the_same_effects(monkeypatch):
    from test_gpu_sharded import run_ranks

    X, y, beta, Z = _run_problem()
    with va.Data(N_RUN, MT_RUN) as d:
        one = _staged_run(d, X, y, beta, Z, 4, check=False)
    parts = run_ranks(monkeypatch, 2, N_RUN, MT_RUN, lambda r, d: _staged_run(d, X, y, beta, Z, 4, check=False))
    assert np.array_equal(parts[0]["cov_eff"], parts[1]["cov_eff"])
    assert np.array_equal(parts[0]["cov_eff"], one["cov_eff"])
    for it, (e, miss, same_tau) in enumerate(parts[0]["stage"]):
        print(f"  rank 0 it {it + 1}: beta1 vs restatement {e:.2e}, vs no offset {miss:.2e}, tau1 equal {same_tau}")
    for it, (e, miss, same_tau) in enumerate(parts[0]["stage"]):
        assert e <= 1e-12 and same_tau and miss > 1e-6, it + 1


def _cli(tmp_path, name, *extra):
    out = tmp_path / name
    out.mkdir()
    cmd = [va.CLI_PATH, "--meth-file", str(tmp_path / "ex.bin"), "--phen-file", str(tmp_path / "ex.phen"),
           "--N", str(N_RUN), "--Mt", str(MT_RUN), "--out-dir", str(out), "--out-name", "ex", "--iterations", "4",
           "--stop-criteria-thr", "0", "--true-signal-file", str(tmp_path / "ex_ts.bin"), *extra]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return out, r.stdout


def test_cli_covariates(tmp_path):
    X, y, beta, Z = _run_problem()
    X.astype("<f8").tofile(tmp_path / "ex.bin")
    (tmp_path / "ex.phen").write_text("".join("%d %d %d\n" % (i, i, v) for i, v in enumerate(y)))
    beta.astype("<f8").tofile(tmp_path / "ex_ts.bin")
    cov = tmp_path / "ex.cov"
    write_table(cov, Z, sep="\t")
    out_c, txt = _cli(tmp_path, "cov", "--model", "bin_class", "--C", "3", "--cov-file", str(cov))
    out_0, _ = _cli(tmp_path, "c0", "--model", "bin_class", "--C", "0", "--cov-file", str(cov))
    out_l = tmp_path / "lib"
    out_l.mkdir()
    with va.Data(N_RUN, MT_RUN) as d:
        d.read_methylation_data(str(tmp_path / "ex.bin"))
        d.read_phen(str(tmp_path / "ex.phen"), standardize=False)
        d.read_covariates(str(cov), 3)
        assert np.array_equal(d.get_covariates(), R.parse_covariates(str(cov), N_RUN, 3))
        v = va.Vamp(d, va.VampOptions(model="bin_class", max_iter=4, stop_criteria_thr=0.0, out_dir=str(out_l),
                                      out_name="ex"), true_signal=beta)
        v.infere()
        eff = v.cov_eff
    assert (out_c / "ex_cov_eff.bin").read_bytes() == eff.astype("<f8").tobytes()
    assert (out_c / "ex_params.csv").read_bytes() == (out_l / "ex_params.csv").read_bytes()
    assert (out_c / "ex_params.csv").read_bytes() != (out_0 / "ex_params.csv").read_bytes()
    assert not (out_0 / "ex_cov_eff.bin").exists()
    # the reference's print (src/vamp_probit.cpp:84-91): four per row
    assert "cov_eff[0] = %g, cov_eff[1] = %g, cov_eff[2] = %g, \n" % tuple(eff) in txt
    # the linear model ignores the table: the same files with and without it
    out_a, txt_a = _cli(tmp_path, "lin_c", "--model", "linear", "--C", "3", "--cov-file", str(cov))
    out_b, txt_b = _cli(tmp_path, "lin", "--model", "linear")
    assert "covariates are used by --model bin_class only" in txt_a and "covariates are used" not in txt_b
    names = sorted(os.listdir(out_b))
    assert names == sorted(os.listdir(out_a)) and "ex_params.csv" in names
    for n in names:
        assert (out_a / n).read_bytes() == (out_b / n).read_bytes(), n
