"""Covariates of the probit model without a device: the ingest
(vampomi_parse_covariates, data::read_covariates src/data.cpp:159-227) against
the numpy restatement bit for bit, its error paths, the restatement's own fit
against an independent probit maximum likelihood, the ABI, and the CLI's exit."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import vampomi_amd as va
from vampomi_amd import _lib

import _cov_ref as R

NEW_SYMBOLS = ["vampomi_parse_covariates", "vampomi_read_covariates", "vampomi_set_covariates",
               "vampomi_get_covariates", "vampomi_cov_eval", "vampomi_newton_cov", "vampomi_denoise_bin_cov",
               "vampomi_get_cov_eff", "vampomi_get_probit_state"]

# (N, C, seed) of R.probit_problem whose Newton traces keep every borderline
# decision away from its threshold (R.trace_is_safe, asserted where they are used)
SAFE_FITS = [(64, 2, 8), (301, 3, 11), (1000, 5, 3), (4099, 8, 3)]


def parse(path, N, Cn, standardize=1):
    out = np.full((max(Cn, 1), N), np.nan)
    st = va.load().vampomi_parse_covariates(str(path).encode(), N, Cn, standardize,
                                            out.ctypes.data_as(C.c_void_p))
    return st, out[:Cn].T  # (N, C)


def write_table(path, Z, sep=" ", lead=""):
    with open(path, "w") as f:
        f.write("FID IID " + " ".join("c%d" % j for j in range(Z.shape[1])) + "\n")
        for i, row in enumerate(Z):
            f.write(lead + sep.join(["f%d" % i, "i%d" % i] + [repr(float(v)) for v in row]) + "\n")


@pytest.mark.parametrize("Cn,sep,lead", [(3, " ", ""), (3, "\t", ""), (3, "  \t ", ""), (1, " ", ""), (64, " ", "")],
                         ids=["blank", "tab", "runs", "C1", "C64"])
def test_parse_matches_restatement_bitwise(tmp_path, Cn, sep, lead):
    N = 37
    rng = np.random.default_rng(5 + Cn)
    Z = rng.standard_normal((N, Cn)) * rng.uniform(0.1, 30, Cn) + rng.uniform(-50, 50, Cn)
    if Cn >= 3:
        Z[:, 1] = 4.25  # a constant column becomes zeros
    p = tmp_path / "cov.txt"
    write_table(p, Z, sep, lead)
    for std in (1, 0):
        st, got = parse(p, N, Cn, std)
        assert st == 0, va.load().vampomi_last_error()
        ref = R.parse_covariates(str(p), N, Cn, bool(std))
        assert np.array_equal(got, ref)
    st, got = parse(p, N, Cn, 1)
    if Cn >= 3:
        assert np.all(got[:, 1] == 0.0)
    assert np.allclose(got[:, 0].mean(), 0, atol=1e-14) and np.allclose((got[:, 0] ** 2).mean(), 1, atol=1e-13)


def test_crlf_and_trailing_blanks(tmp_path):
    p = tmp_path / "cov.txt"
    p.write_bytes(b"FID IID a b\r\n0 0 1.5 2 \r\n1 1 -3e-1 4\t\r\n2 2 7 8.125")
    st, got = parse(p, 3, 2, 0)
    assert st == 0 and np.array_equal(got, [[1.5, 2], [-0.3, 4], [7, 8.125]])
    assert np.array_equal(got, R.parse_covariates(str(p), 3, 2, False))
    # the "\\s+" split gives an empty first token after a leading blank run, which counts as an ID
    p.write_text("FID IID a b\n  7 1.5 2.5\n\t8 -1 0.25\n")
    st, got = parse(p, 2, 2, 0)
    assert st == 0 and np.array_equal(got, [[1.5, 2.5], [-1, 0.25]])
    assert np.array_equal(got, R.parse_covariates(str(p), 2, 2, False))


def test_wrong_field_count_is_err_io_with_the_fatal_text(tmp_path, capfd):
    p = tmp_path / "cov.txt"
    write_table(p, np.arange(12.0).reshape(4, 3))
    st, _ = parse(p, 4, 2)
    assert st == 4
    assert R.FATAL % (3, 2) in capfd.readouterr().out  # the library's own stdout (file descriptor 1)
    assert (R.FATAL % (3, 2)).encode() in va.load().vampomi_last_error()
    with pytest.raises(R.CovFormatError, match="number of covariates = 3"):
        R.parse_covariates(str(p), 4, 2)


def test_wrong_row_count_is_err_io(tmp_path):
    p = tmp_path / "cov.txt"
    write_table(p, np.arange(12.0).reshape(4, 3))
    assert parse(p, 5, 3)[0] == 4
    assert parse(p, 3, 3)[0] == 4
    assert parse(p, 4, 3)[0] == 0
    assert parse(tmp_path / "absent.txt", 4, 3)[0] == 4


def test_too_many_covariates_is_err_arg_and_zero_is_a_no_op(tmp_path):
    assert parse(tmp_path / "absent.txt", 4, 65)[0] == 1
    assert parse(tmp_path / "absent.txt", 4, -1)[0] == 1
    st, got = parse(tmp_path / "absent.txt", 4, 0)
    assert st == 0 and got.shape == (4, 0)
    assert _lib.MAX_C == 64


@pytest.mark.parametrize("N,Cn,seed", SAFE_FITS)
def test_restatement_fit_is_the_probit_mle(N, Cn, seed):
    """The restated Newton loop ends at the maximum of the probit likelihood: an
    independent optimiser on the same likelihood agrees to 1e-4 relative, the
    tolerance at which the fit itself stops.  The trace is one of those whose
    decisions are not borderline."""
    from scipy.optimize import minimize
    from scipy.special import log_ndtr

    Z, y, _ = R.probit_problem(N, Cn, seed)
    eta, tr = R.newton(Z, y)
    assert R.trace_is_safe(tr), tr
    assert tr["final"] == tr["iters"] - 1 and tr["iters"] >= 3
    s = 2 * y - 1

    def nll(e):
        return -np.mean(log_ndtr(s * (Z @ e)))

    def grad(e):
        a = s * (Z @ e)
        return -(Z * (s * np.exp(-0.5 * a * a - log_ndtr(a)) / np.sqrt(2 * np.pi))[:, None]).mean(axis=0)

    best = minimize(nll, np.zeros(Cn), jac=grad, method="BFGS", options={"gtol": 1e-10})
    assert np.linalg.norm(eta - best.x) <= 1e-4 * np.linalg.norm(best.x)


def test_restatement_constant_column_gives_zero_effects():
    Z, y, _ = R.probit_problem(301, 3, 11)
    Z[:, 1] = R.standardize(np.full((301, 1), 2.5))[:, 0]
    eta, tr = R.newton(Z, y)
    assert np.all(eta == 0.0) and tr["iters"] == 1 and tr["final"] == 0


def test_offset_denoiser_identities_of_the_restatement():
    rng = np.random.default_rng(2)
    p, m = rng.standard_normal(50), rng.standard_normal(50)
    y = (rng.random(50) < 0.5).astype(float)
    for tau1 in (1e-6, 0.7, 40.0):
        assert np.array_equal(R.g1d_bin_cov(p, tau1, y, m), R.g1d_bin_cov(p + m, tau1, y, 0 * m))
        a, b = R.g1_bin_cov(p, tau1, y, m), R.g1_bin_cov(p + m, tau1, y, 0 * m) - m
        assert np.max(np.abs(a - b) / np.maximum(np.abs(a), np.abs(p) + np.abs(m))) < 1e-12
        z0 = np.array([va_g1(pp, tau1, yy) for pp, yy in zip(p, y)])
        assert np.array_equal(R.g1_bin_cov(p, tau1, y, 0 * m), z0)


def va_g1(p, tau1, y):
    from oracle import pyoracle as O
    return O.g1_bin(p, tau1, y)


def test_abi_version_and_new_symbols():
    lib = va.load()
    assert lib.vampomi_abi_version() == 3
    raw = C.CDLL(_lib.LIB_PATH)
    for n in NEW_SYMBOLS:
        assert hasattr(raw, n) and n in _lib.SIGNATURES, n
    assert lib.vampomi_set_covariates(None, None, 0, 0, 0) == 1
    assert lib.vampomi_get_cov_eff(None, None) == 1
    assert lib.vampomi_get_probit_state(None, None, None) == 1


def test_cli_wrong_field_count_exits_1_before_any_device_call(tmp_path):
    p = tmp_path / "cov.txt"
    write_table(p, np.arange(30.0).reshape(10, 3))
    r = subprocess.run([va.CLI_PATH, "--meth-file", "m.bin", "--phen-file", "y.phen", "--N", "10", "--Mt", "20",
                        "--model", "bin_class", "--C", "2", "--cov-file", str(p)], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 1 and R.FATAL % (3, 2) in r.stdout
    r = subprocess.run([va.CLI_PATH, "--meth-file", "m.bin", "--phen-file", "y.phen", "--N", "10", "--Mt", "20",
                        "--model", "bin_class", "--C", "65", "--cov-file", str(p)], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 1 and "covariates" in r.stdout
